"""Live streams on the MI355X: the cases of tests/test_stream_cpu.py on the device (cases, yardstick and the utterance-to-offline-row
mapping: tests/stream_util.py), the recipe's dimensions, and a long session whose buffer halves swap a hundred times.  Every
comparison is bit for bit against the unbroken offline path (stage6.convert_pairs) in the same kernel class."""
import numpy as np
import pytest
import torch

import stream_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    assert torch.cuda.is_available()
    return gru_vae


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- 1. cvae_stream_move alone ----

def test_move_widths_strides_rows_and_misaligned_pointers(gv, dev):
    S.check_move_shapes(gv._lib(), dev)


@pytest.mark.parametrize("njobs", [1, 96, 97])
def test_move_job_counts_around_the_split(gv, dev, njobs):
    S.check_move_split(gv._lib(), dev, njobs)


def test_move_refusals_enqueue_nothing(gv, dev):
    S.check_move_refusals(gv._lib(), dev, pytest.raises)


# ---- 2. - 8. on the device ----

@pytest.mark.parametrize("how", ["all at once", "single frames", "random 1..20", "larger than hop"])
def test_chunking_does_not_change_a_bit(gv, dev, how):
    su = S.setup(gv, dev, (61,))
    S.one_session(su, S.chunkings(61, 8, "c61")[how], what=how)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9])
def test_utterances_around_the_reach(gv, dev, n):
    su = S.setup(gv, dev, (1, 3, 4, 5, 8, 9), tag="edges")
    utt = su.lens.index(n)
    S.one_session(su, [n], utt=utt, what="closed before the first step")
    if n > 2:
        S.one_session(su, [n - 2, 2], utt=utt, close_after=1, what="closed between steps")


def test_three_hundred_frames_through_small_buffers(gv, dev):
    su = S.setup(gv, dev, (300,), tag="long")
    sc = su.converter(max_sessions=4, hop=8, max_pending=24)
    got = S.run(sc, su, [dict(utt=0, open=0, chunks=[5] * 60)])[0]
    S.same(got, su.offline(dataflow=True)[0], "300 frames")


def test_sessions_that_come_and_go_get_their_offline_rows(gv, dev):
    su = S.setup(gv, dev, S.MIX_LENS + (14,), tag="mix")
    want = su.offline(dataflow=True)
    sc = su.converter(max_sessions=6, hop=8)
    plan = S.mix_plan()
    got = S.run(sc, su, plan)
    for i, g in enumerate(got):
        S.same(g, want[i], "mix, utterance %d" % i)
    again = S.run(sc, su, [dict(utt=5, open=0, chunks=[3, 7, 4])])[0]
    S.same(again, want[5], "a reused slot")
    for i in range(5):
        alone = S.run(su.converter(max_sessions=6, hop=8), su, [plan[i]])[0]
        assert np.array_equal(alone["cv"], got[i]["cv"]) and np.array_equal(alone["lat"], got[i]["lat"]), i


@pytest.mark.parametrize("n,posterior,src_row", [(3, "gauss", True), (1, "laplace", False), (3, "laplace", False)])
def test_rows_draw_counts_and_posteriors(gv, dev, n, posterior, src_row):
    su = S.setup(gv, dev, (21,), tag="rows")
    S.one_session(su, [6, 9, 6], n=n, posterior=posterior, src_row=src_row)


@pytest.mark.parametrize("enc_ds,dec_ds", [(1, 1), (3, 3), (2, 1)])
def test_front_ends_of_other_depths(gv, dev, enc_ds, dec_ds):
    su = S.setup(gv, dev, (37,), tag="fe%d%d" % (enc_ds, dec_ds), enc_ds=enc_ds, dec_ds=dec_ds)
    sc = su.converter(max_sessions=1, hop=8)
    assert sc.latency_frames == (3 ** enc_ds - 1) // 2 + (3 ** dec_ds - 1) // 2
    S.one_session(su, [10, 3, 20, 4], hop=8)


def test_library_calls_per_step_do_not_depend_on_the_live_sessions(gv, dev):
    su = S.setup(gv, dev, S.MIX_LENS + (14,), tag="mix")
    counts = {}
    for live in (1, 5):
        sc = su.converter(max_sessions=6, hop=4, max_pending=16)
        sids = [sc.open(torch.tensor([S.TRG_CODE]), draw_id=i) for i in range(live)]
        for step in range(2):
            for i, sid in enumerate(sids):
                sc.push(sid, torch.from_numpy(su.utts[i][6 * step:6 * step + 6]))
            calls, copies, out = S.count_calls(sc.step)
        assert len(out) == live
        counts[live] = (calls, copies)
    torch.cuda.synchronize()
    assert counts[1] == counts[5] and counts[1][0]["stream_move"] == 3 and counts[1][1] <= 1, counts


# ---- 9. failure handling ----

def test_a_step_that_fails_leaves_the_sessions_as_they_were(gv, dev, monkeypatch):
    S.check_failed_step(gv, dev, monkeypatch)


def test_range_policy_retry_and_raise(gv, dev):
    gv._lib()
    S.check_range_policy(gv, dev, gv._sink(), pytest.raises)


def test_pushes_and_steps_without_a_wait_in_between(gv, dev):
    """The host enqueues every push and step of five sessions while the stream is still busy with a spin kernel (about 0.1 s): the
    pinned staging buffers must not be rewritten before the copies that read them have run."""
    st = torch.cuda.current_stream().cuda_stream
    S.check_host_runs_ahead(gv, dev, lag=lambda: gv._lib().selftest_occupy(1, 1024, 200000000, st))


# ---- 12. the recipe's dimensions ----

@pytest.fixture(scope="module")
def recipe(gv, dev):
    return S.setup(gv, dev, (30, 45, 37, 41, 33), tag="hu1024", in_dim=54, out_dim=50, lat_dim=32, hidden=1024)


def test_recipe_dimensions_five_sessions(recipe):
    """hu1024 (54 -> 64, 34 -> 50, lat 32), five sessions of 30 .. 45 frames, hop 16, some pushed from the host and some from the device:
    convert_pairs of the same utterances bit for bit."""
    want = recipe.offline(dataflow=True)
    plan = [dict(utt=i, open=i % 2, chunks=c, close_after=i % 2)
            for i, c in enumerate(([16, 14], [20, 20, 5], [7, 30], [16, 16, 9], [33]))]
    got = S.run(recipe.converter(max_sessions=5, hop=16), recipe, plan)
    for i, g in enumerate(got):
        S.same(g, want[i], "hu1024, utterance %d" % i)


def test_recipe_dimensions_one_session(recipe):
    got = S.run(recipe.converter(max_sessions=1, hop=16), recipe, [dict(utt=1, open=0, chunks=[20, 20, 5])])[0]
    S.same(got, recipe.offline()[1], "hu1024, one session against a single pair")


# ---- 13. half-swap aliasing ----

def test_two_thousand_frames_in_chunks_of_forty(gv, dev):
    """A 2000-frame session at hidden 64, chunks of 40, hop 16: every step reads the half the step before wrote and writes the other
    one, with nothing but stream order between them."""
    su = S.setup(gv, dev, (2000,), tag="long2000")
    sc = su.converter(max_sessions=4, hop=16, max_pending=64)
    got = S.run(sc, su, [dict(utt=0, open=0, chunks=[40] * 50)])[0]
    S.same(got, su.offline(dataflow=True)[0], "2000 frames")
    assert got["steps"] >= 125
