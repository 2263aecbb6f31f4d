"""Live streams without a GPU: cvae_stream_move and stream.StreamConverter on the host-fiber emulator, CPU tensors as "device"
tensors (cases, yardstick and the utterance-to-offline-row mapping: tests/stream_util.py).  Every comparison is bit for bit
against the unbroken offline path (stage6.convert_pairs) in the same kernel class."""
import ctypes

import numpy as np
import pytest
import torch

import _cabi
import stream_util as S
from emu_util import bind_emulator, emu_lib

CPU = torch.device("cpu")


@pytest.fixture
def gv(monkeypatch):
    return bind_emulator(monkeypatch)


def test_abi_stays_10_and_the_export_is_bound():
    lib = emu_lib()
    assert _cabi.ABI_VERSION == 10 and lib.lib.cvae_abi_version() == 10
    assert "cvae_stream_move" in _cabi.EXPORTS and "cvae_stream_move" in _cabi.ADDITIVE and hasattr(lib.lib, "cvae_stream_move")
    assert ctypes.sizeof(_cabi.MoveJob) == 40      # 96 jobs + a count under the 4 KiB of kernel arguments


# ---- 1. cvae_stream_move alone ----

def test_move_widths_strides_rows_and_misaligned_pointers():
    S.check_move_shapes(emu_lib(), CPU)


@pytest.mark.parametrize("njobs", [1, 96, 97])
def test_move_job_counts_around_the_split(njobs):
    S.check_move_split(emu_lib(), CPU, njobs)


def test_move_refusals_enqueue_nothing():
    S.check_move_refusals(emu_lib(), CPU, pytest.raises)


# ---- 2. chunking invariance, word-exchange class ----

@pytest.mark.parametrize("how", ["all at once", "single frames", "random 1..20", "larger than hop"])
def test_chunking_does_not_change_a_bit(gv, how):
    """One session, 61 frames, hop 8: cv and lat concatenated equal the offline pair however the frames arrive."""
    su = S.setup(gv, CPU, (61,))
    got = S.one_session(su, S.chunkings(61, 8, "c61")[how], what=how)
    assert got["steps"] >= 8      # (61 frames at 8 per step)


# ---- 3. edges of the reach ----

@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9])
def test_utterances_around_the_reach(gv, n):
    """Reach 4: closed before the first step, and closed between steps with fewer than `reach` frames pending (all but the last two
    frames pushed, a step, the rest, a step, close)."""
    su = S.setup(gv, CPU, (1, 3, 4, 5, 8, 9), tag="edges")
    utt = su.lens.index(n)
    assert su.converter(max_sessions=1).reach_enc == 4
    S.one_session(su, [n], utt=utt, what="closed before the first step")
    if n > 2:
        S.one_session(su, [n - 2, 2], utt=utt, close_after=1, what="closed between steps")


# ---- 4. compaction ----

def test_three_hundred_frames_through_small_buffers(gv):
    """max_pending 24, hop 8, 300 frames in chunks of 5: the input and latent halves swap at least 37 times."""
    su = S.setup(gv, CPU, (300,), tag="long")
    sc = su.converter(max_sessions=4, hop=8, max_pending=24)      # (one live session of a dataflow converter: idle cells beside it)
    swaps = [0, None]

    def on_step(step, out):
        s = next(iter(sc._sessions.values()), None)
        if s is not None:
            swaps[0] += s.in_half != swaps[1]
            swaps[1] = s.in_half
    got = S.run(sc, su, [dict(utt=0, open=0, chunks=[5] * 60)], on_step=on_step)[0]
    S.same(got, su.offline(dataflow=True)[0], "300 frames")
    assert swaps[0] >= 37, swaps


# ---- 5. / 6. many sessions, dataflow class; slot reuse ----

def test_sessions_that_come_and_go_get_their_offline_rows(gv):
    """max_sessions 6, five utterances opened at steps 0, 0, 1, 3, 3, random chunkings, closed at different steps (the live count
    crosses 3 <-> 4); then a sixth utterance in a slot a finished session freed.  Each session alone in a max_sessions = 6 converter
    gives the bits it got in the mix."""
    su = S.setup(gv, CPU, S.MIX_LENS + (14,), tag="mix")
    want = su.offline(dataflow=True)
    sc = su.converter(max_sessions=6, hop=8)
    live = []
    plan = S.mix_plan()
    got = S.run(sc, su, plan, on_step=lambda step, out: live.append(len(sc._sessions)))
    for i, g in enumerate(got):
        S.same(g, want[i], "mix, utterance %d" % i)
    assert max(live) >= 4 and any(a >= 4 > b for a, b in zip(live, live[1:])) and any(a < 4 <= b for a, b in zip(live, live[1:])), live
    # 6. the converter has seen five sessions end: the sixth utterance takes a freed slot
    assert not sc._sessions and sorted(sc._free) == list(range(6))
    again = S.run(sc, su, [dict(utt=5, open=0, chunks=[3, 7, 4])])[0]
    S.same(again, want[5], "a reused slot")
    for i in range(5):
        alone = S.run(su.converter(max_sessions=6, hop=8), su, [plan[i]])[0]
        assert np.array_equal(alone["cv"], got[i]["cv"]) and np.array_equal(alone["lat"], got[i]["lat"]), i


# ---- 7. two decoder rows ----

def test_two_decoder_rows_share_one_sampling(gv):
    su = S.setup(gv, CPU, (21,), tag="rows")
    S.one_session(su, [6, 9, 6], src_row=True, n=3)


# ---- 8. other parameters ----

@pytest.mark.parametrize("n,posterior", [(1, "laplace"), (3, "gauss"), (3, "laplace")])
def test_draw_counts_and_posteriors(gv, n, posterior):
    su = S.setup(gv, CPU, (21,), tag="rows")
    S.one_session(su, [6, 9, 6], n=n, posterior=posterior, max_sessions=4)


@pytest.mark.parametrize("ds,reach", [(1, 1), (3, 13)])
def test_front_ends_of_other_depths(gv, ds, reach):
    su = S.setup(gv, CPU, (37,), tag="fe%d" % ds, enc_ds=ds, dec_ds=ds)
    sc = su.converter(max_sessions=1, hop=8)
    assert (sc.reach_enc, sc.reach_dec, sc.latency_frames) == (reach, reach, 2 * reach)
    S.one_session(su, [10, 3, 20, 4], hop=8, max_sessions=4)


def test_encoder_and_decoder_of_different_reach(gv):
    su = S.setup(gv, CPU, (29,), tag="mixed", enc_ds=2, dec_ds=1)
    sc = su.converter(max_sessions=1, hop=8)
    assert (sc.reach_enc, sc.reach_dec, sc.latency_frames) == (4, 1, 5)
    S.one_session(su, [7, 7, 7, 8], hop=8, max_sessions=4)
    su = S.setup(gv, CPU, (29,), tag="mixed", enc_ds=1, dec_ds=2)
    assert su.converter(max_sessions=1, hop=8).latency_frames == 5
    S.one_session(su, [7, 7, 7, 8], hop=8, max_sessions=4)


# ---- 9. failure handling ----

def test_push_past_max_pending_raises(gv):
    su = S.setup(gv, CPU, (61,))
    sc = su.converter(max_sessions=1, hop=8, max_pending=16)
    sid = sc.open(torch.tensor([S.TRG_CODE]))
    sc.push(sid, torch.from_numpy(su.utts[0][:16]))
    with pytest.raises(ValueError, match="max_pending"):
        sc.push(sid, torch.from_numpy(su.utts[0][16:17]))
    sc.step()
    sc.push(sid, torch.from_numpy(su.utts[0][16:24]))      # (the step consumed 8)
    with pytest.raises(RuntimeError, match="closed"):
        sc.close(sid)
        sc.push(sid, torch.from_numpy(su.utts[0][24:25]))
    with pytest.raises(KeyError):
        sc.push(sid + 1, torch.from_numpy(su.utts[0][:1]))


def test_a_step_that_fails_leaves_the_sessions_as_they_were(gv, monkeypatch):
    S.check_failed_step(gv, CPU, monkeypatch)


def test_range_policy_retry_and_raise(gv, monkeypatch):
    sink = torch.zeros(4, dtype=torch.int32)
    gv._lib().set_status_sink(sink.data_ptr())
    monkeypatch.setattr(gv, "_sink", lambda: sink)
    S.check_range_policy(gv, CPU, sink, pytest.raises)


def test_pushes_and_steps_without_a_wait_in_between(gv):
    """(On the emulator every call is synchronous: this runs the host-staging bookkeeping -- two buffers, alternated -- and the
    device-side collection of the outputs; the race itself is a GPU case.)"""
    S.check_host_runs_ahead(gv, CPU, lens=(30, 25, 20, 25, 20))


# ---- 10. launch count ----

def test_library_calls_per_step_do_not_depend_on_the_live_sessions(gv):
    su = S.setup(gv, CPU, S.MIX_LENS + (14,), tag="mix")
    counts = {}
    for live in (1, 5):
        sc = su.converter(max_sessions=6, hop=4, max_pending=16)
        sids = [sc.open(torch.tensor([S.TRG_CODE]), draw_id=i) for i in range(live)]
        for step in range(2):      # steady state: frames pushed, consumed frames to compact, both passes running
            for i, sid in enumerate(sids):
                sc.push(sid, torch.from_numpy(su.utts[i][6 * step:6 * step + 6]))
            calls, copies, out = S.count_calls(sc.step)
        assert len(out) == live and all(v["cv"].shape[1] > 0 and v["lat"].shape[0] > 0 for v in out.values())
        counts[live] = (calls, copies)
    assert counts[1] == counts[5], counts
    calls, copies = counts[1]
    assert calls["stream_move"] == 3 and calls["gru_rnn_forward_stacked_carry"] == 2 and copies <= 1, counts[1]
    assert set(calls) <= {"stream_move", "gru_rnn_forward_stacked_carry", "pass_input", "get_option", "set_option"}, calls


# ---- 11. refusals, without a device (the real gru_vae: no emulator binding) ----

def test_refusals_before_anything_touches_the_device():
    import gru_vae
    import stream
    P = S.synth.CycleVAEProblem(B=1, T=4, in_dim=10, out_dim=6, lat_dim=4, hidden=64, tag="refuse")
    enc, dec = S.module(gru_vae, P.enc, 10, 8, 64, True, CPU), S.module(gru_vae, P.dec, 6, 6, 64, False, CPU)
    y = (torch.zeros(1, 1, 8), torch.zeros(1, 1, 6))
    with pytest.raises(RuntimeError, match="HIP device only"):
        stream.StreamConverter(enc, dec, y[0], y[1], 4)
    with pytest.raises(ValueError, match="posterior"):
        stream.StreamConverter(enc, dec, y[0], y[1], 4, posterior="gmm")
    deep = gru_vae.GRU_RNN(in_dim=10, out_dim=8, hidden_units=64, hidden_layers=2)
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        stream.StreamConverter(deep, dec, y[0], y[1], 4)
    with pytest.raises(ValueError, match="CVAE_MAX_CELLS"):
        stream.StreamConverter(enc, dec, y[0], y[1], 4, max_sessions=17, rows=2)
    with pytest.raises(ValueError, match="CVAE_MAX_CELLS"):
        stream.StreamConverter(enc, dec, y[0], y[1], 4, max_sessions=33)
