"""The training loop's per-window monitoring on the MI355X: tests/test_trainlog_cpu.py's cases on the device -- there the end-to-end
case drives the monitor with stand-in trajectories, here stage4.Stage4Step itself runs between before() and after() -- and one
H = 1024 window sequence with a step that never waits (sync=False).  Yardstick and tolerances as in the CPU file (PARITY UNPINNED for
the DTW / calc_mcd halves)."""
import numpy as np
import pytest

import _cabi
import trainlog_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    import gru_vae
    assert torch.cuda.is_available()
    return U.TorchBackend(gru_vae._lib(), torch.device("cuda:0"))


def test_abi_version_and_export(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10
    assert "cvae_trainlog_window" in _cabi.EXPORTS and hasattr(be.lib.lib, "cvae_trainlog_window")


def test_window_kernel_against_the_restatement(be):
    U.check_kernel_alone(be)


def test_window_kernel_index_outside_the_window(be):
    U.check_bad_index(be)


def test_window_kernel_grid_independence(be):
    U.check_grid_independence(be)


def test_window_kernel_refuses_bad_arguments(be):
    U.check_refusals(be)


@pytest.mark.parametrize("with_sentinel", [True, False], ids=["sentinel_between_batches", "two_batches_one_pass"])
def test_trainlog_end_to_end(be, with_sentinel):
    """(b) on the device, around the real Stage4Step (injected eps and dropout masks): figures against trainlog_ref on the library's
    own last_trajs at 1e-10 relative, text lines equal, parameters bit-identical to the same run without a monitor."""
    U.check_e2e(be.dev, with_sentinel)


def test_trainlog_h1024_lagged_step(be):
    """(c) H = 1024, B = 2, T = 80: the two windows of a 130-frame pair around Stage4Step(sync=False), three passes over them.
    Finite figures; utterance 0's records bit-identical when the kernel is given row 0 alone; lines() called only at the end returns
    every window's line once and in order; and the host is back from after() before the step's end event has completed at least
    once -- nothing between before() and after() waited for the device."""
    import torch
    import stage4
    import synth
    import trainlog
    import trainlog_ref as tref
    from validation_util import modules
    dev, tag, T, F, B = be.dev, "tl/h1024", 80, 130, 2
    P = synth.CycleVAEProblem(B=B, T=T, tag=tag, bias_scale=0.05)
    enc, dec = modules(P, dev)
    enc.train()
    dec.train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.RandomState(7)
    spc_rows = [np.sort(rng.choice(n, size=n * 2 // 3, replace=False)) for n in (F, 117)]
    batch = dict(feat=synth.features(tag + "/feat", B, F, P.mu, P.sigma), par=synth.features(tag + "/par", B, 120, P.mu, P.sigma),
                 cv=synth.features(tag + "/cv", B, F, P.mu[:P.stdim], P.sigma[:P.stdim]), files=["/d/SF1/a.h5", "/d/SF1/b.h5"],
                 files_trg=["/d/TF1/a.h5", "/d/TF1/b.h5"], flens=np.array([F, 117]), flens_trg=np.array([120, 111]),
                 ns=np.array([len(r) for r in spc_rows]), ns_trg=np.array([70, 60]))
    batch["own"], batch["other"] = synth.onehot_codes(B, F)
    batch["spc"] = np.zeros((B, max(batch["ns"])), np.int64)
    for j, r in enumerate(spc_rows):
        batch["spc"][j, :len(r)] = r
    batch["spc_trg"] = np.stack([np.arange(70), np.concatenate([np.arange(60), np.zeros(10, np.int64)])])
    gv = np.ones(P.out_dim - 1)
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=2, lr=1e-5, sync=False)
    tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, gv, gv, n_cyc=2, spk_src="SF1")
    ref = tref.RefTrainLog(P.lat_dim, P.stdim, gv, gv, n_cyc=2, spk_src="SF1")
    y_pp, y_dec = t(P.y_in_enc), t(P.y_in_dec)
    wins = list(U.yields(batch, T, t))
    assert [(w[5], w[6]) for w in wins] == [(0, 79), (80, 129)]
    early = 0
    for rep in range(3):
        carry = None
        for items in wins:
            s, e = items[5], items[6]
            tl.before(items, y_pp)
            ref.before(U.host_items(items), None if tl.last_lat_srctrg is None else tl.last_lat_srctrg.cpu().numpy())
            loss, carry = step(items[0][:, s:e + 1], items[4][:, s:e + 1], items[1], items[2], y_pp, y_dec, None,
                               flen_acc=[int(v) for v in items[20]], select_utt_idx=list(items[19]), carry=carry, return_state=True)
            done = torch.cuda.Event()
            done.record()
            tl.after(items, step.last_trajs, loss)
            early += 0 if done.query() else 1
            trajs, got = step.last_trajs, tl.last_record.cpu().numpy()
            ref.after(U.host_items(items), [{k: v.detach().cpu().numpy() for k, v in tr.items()} for tr in trajs], float(loss))
            sel = list(items[19])
            assert np.all(np.isfinite(got[:, sel, :5])), got
            # row 0 alone
            a = _cabi.TrainlogWindowArgs()
            keep = [tr[k].detach()[:1].contiguous() for tr in trajs for k in U.SLOTS]
            for i in range(2):
                for k in range(5):
                    a.traj[i][k] = keep[i * 5 + k].data_ptr()
            s, e = items[5], items[6]
            host = [np.ascontiguousarray(np.asarray(items[k])[:1], np.int32) for k in (20, 7, 8)] + [np.array([1 if 0 in sel else 0], np.uint8)]
            out = torch.empty(2, 1, 9, dtype=torch.float64, device=dev)
            a.x_win, a.x_row_stride, a.x_utt_stride = items[0].data_ptr() + 4 * s * P.in_dim, P.in_dim, F * P.in_dim
            a.spcidx, a.spc_ld = items[11].data_ptr(), items[11].shape[1]
            a.flen_acc, a.s_idx, a.e_idx, a.selected = (h.ctypes.data for h in host)
            a.n_cyc, a.B, a.T, a.D, a.L, a.stdim, a.src_idx_s = 2, 1, e - s + 1, P.out_dim, P.lat_dim, P.stdim, s
            a.rec_out = out.data_ptr()
            be.lib.trainlog_window(a, be.stream)
            assert np.array_equal(out.cpu().numpy()[:, 0], got[:, 0], equal_nan=True)
    step.finish()
    tl.before(U.sentinel(), y_pp)
    ref.before(U.sentinel(), tl.last_lat_srctrg.cpu().numpy())
    lines = tl.lines()                      # the first call of the run: everything arrives late, once, in the script's order
    assert tl.lines() == []
    assert lines == ref.lines, "\n".join(lines + ref.lines)
    assert [l.split(" = ")[0] for l in lines if l.startswith("batch loss")] == ["batch loss [1]"] * 6
    s, r = tl.epoch_end(), ref.epoch_end()
    assert s["line"] == r["line"]
    assert np.isfinite(s["loss"]) and np.isfinite(s["mcdpow_src_trg"]) and np.isfinite(s["lat_dist_srctrg1"]) and np.isfinite(s["eval_gv_src_trg"])
    assert all(np.isnan(s[k]) == np.isnan(r[k]) for k in r if k != "line"), (s, r)
    print("after() returned before the step's end event had completed in %d of 6 windows" % early)
    assert early >= 1
