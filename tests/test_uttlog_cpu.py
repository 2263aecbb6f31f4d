"""The training loop's monitoring on utterance-length mini-batches (batch_size == 0) without a GPU: trainlog.UttLog end to end on the
host-fiber emulator.  As in tests/test_trainlog_cpu.py the emulated stage4.Stage4Step would take minutes, so the step is stand-in
trajectories and a stand-in loss (uttlog_util.drive); the encoder pass of before(), the window launch and the metric plan are the
emulated library's.  The real step drives the same body in tests/test_uttlog_gpu.py.

Yardstick: tests/uttlog_ref.py (numpy float64 restatement of train_gru_cyclevae_gauss_batch.py:1476-1665 and the shared :719-739).
PARITY UNPINNED for the dtw_org_to_trg / calc_mcd halves.  Tolerance: 1e-10 relative on every figure, NaN where the ref is NaN, as
tests/test_trainlog_cpu.py states for its end-to-end case (both sides float64 on the same fp32 values; sums differ in order only)."""
import numpy as np
import pytest

import uttlog_util as U
from emu_util import bind_emulator


@pytest.fixture
def emu_gru_vae(monkeypatch):
    return bind_emulator(monkeypatch)


def test_uttlog_end_to_end(emu_gru_vae):
    """Two utterance batches (source speaker, then target speaker; 23 / 17 / 9 frames against parallel 19 / 21 / 12) and the
    sentinel: figures, every line and the epoch line against the restatement; the six eval_gv_* figures are finite."""
    import torch
    U.check_e2e(torch.device("cpu"))


def test_uttlog_one_utterance_and_short_last_batch(emu_gru_vae):
    """A batch of ONE utterance, a full batch, and a last batch of two utterances under a y_in_pp of three rows (the script's
    `_mod` tensors): the same figures and lines as the restatement."""
    import torch
    got = U.drive(torch.device("cpu"), seq=U.SMALL, tag="ul/small")
    U.assert_figures(got, "one utterance / short last batch")
    assert [r.shape[1] for r in got["records"]] == [1, 3, 2]
    assert got["ul"].last_lat_srctrg.shape[0] == 2
    assert [l.split(" = ")[0] for l in got["lines"] if l.startswith("batch loss")] == ["batch loss [%d]" % k for k in (1, 2, 3)]


def _problem(dev, tag="ul/refuse"):
    import torch
    import synth
    import trainlog
    from validation_util import modules
    P = synth.CycleVAEProblem(B=3, T=8, tag=tag, **U.H64)
    enc, dec = modules(P, dev)
    ul = trainlog.UttLog(enc, dec, P.lat_dim, P.stdim, np.ones(25), np.ones(25), spk_src=U.SPK_SRC)
    items = U.utt_yield(U.e2e_batches(P, tag)[0], 0, None, torch.from_numpy)
    return P, enc, dec, ul, items


def test_uttlog_refuses_windows_and_cpu_tensors():
    import torch
    import trainlog_util
    P, enc, dec, ul, items = _problem(torch.device("cpu"))
    win = next(trainlog_util.yields(U.e2e_batches(P, "ul/refuse")[0], 8, torch.from_numpy))
    with pytest.raises(NotImplementedError, match="22-field"):
        ul.before(win, torch.from_numpy(P.y_in_enc))
    with pytest.raises(NotImplementedError, match="22-field"):
        ul.after(win, [], None)
    with pytest.raises(ValueError, match="expected 16"):
        ul.before(items[:15], None)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ul.before(items, torch.from_numpy(P.y_in_enc))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ul.after(items, [], None)
    ul.before(U.sentinel(), None)                              # the sentinel touches nothing: no tensor is looked at
    assert ul.last_lat_srctrg is None and ul.epoch_end()["line"].startswith("(EPOCH:1) average optimization loss = nan ;; [1] nan")


def test_uttlog_refuses_bad_trajectories_and_empty_speech(emu_gru_vae):
    import torch
    import synth
    P, enc, dec, ul, items = _problem(torch.device("cpu"), "ul/refuse2")
    B, T = items[0].shape[:2]
    good = [{s: torch.from_numpy(synth.normal("ul/refuse2/%d%s" % (i, s), (B, T, 2 * P.lat_dim if s in ("lat", "latcv") else P.out_dim)))
             for s in U.SLOTS} for i in range(P.n_cyc)]
    loss = torch.tensor(1.0)
    with pytest.raises(ValueError, match="before\\(\\) has not been given this yield"):
        ul.after(items, good, loss)
    ul.before(items, torch.from_numpy(P.y_in_enc))
    with pytest.raises(ValueError, match="1 cycles of trajectories, n_cyc = 2"):
        ul.after(items, good[:1], loss)
    bad = [dict(tr) for tr in good]
    bad[1]["cv"] = bad[1]["cv"][:, :T - 1]
    with pytest.raises(ValueError, match="trajectory cv of cycle 1 has shape"):
        ul.after(items, bad, loss)
    for field in (13, 14):                                     # flens_spc_src / flens_spc_src_trg of 0: dtw and calc_mcd of nothing
        z = list(items)
        z[field] = np.array(items[field]).copy()
        z[field][1] = 0
        z = tuple(z)
        ul.before(z, torch.from_numpy(P.y_in_enc))
        with pytest.raises(ValueError, match="flens_spc of utterance 1"):
            ul.after(z, good, loss)
    assert ul.lines() == [] and ul.iter_count == 0             # nothing was queued by a refused call


def test_trainlog_still_refuses_utterance_length_batches():
    """The pinned behaviour from this side: TrainLog keeps refusing a 16-field yield with NotImplementedError naming batch_size."""
    import torch
    import trainlog
    P, enc, dec, ul, items = _problem(torch.device("cpu"), "ul/refuse3")
    tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, np.ones(25), np.ones(25), spk_src=U.SPK_SRC)
    with pytest.raises(NotImplementedError, match="batch_size"):
        tl.before(items, None)
    with pytest.raises(NotImplementedError, match="UttLog"):
        tl.before(U.sentinel(), None)


def test_utterance_step_args_mapping():
    import torch
    import stage4
    P, enc, dec, ul, items = _problem(torch.device("cpu"), "ul/args")
    kw = stage4.utterance_step_args(items)
    assert sorted(kw) == ["carry", "code_src", "code_trg", "cvx", "flen_acc", "list_quirk", "select_utt_idx", "x"] and kw["list_quirk"] is False
    assert kw["x"] is items[0] and kw["cvx"] is items[4] and kw["code_src"] is items[1] and kw["code_trg"] is items[2]
    assert kw["flen_acc"] == [23, 17, 9] and kw["select_utt_idx"] == [0, 1, 2] and kw["carry"] is None
    w, last, n_sel = stage4.frame_weights(3, 23, kw["flen_acc"], kw["select_utt_idx"])
    assert n_sel == 3 and [sum(1 for v in r if v > 0) for r in w] == [23, 17, 9] and last == [0.0, 0.0, 1.0]
    assert stage4.frame_weights(3, 23, kw["flen_acc"], kw["select_utt_idx"], list_quirk=False) == (w, [1.0, 1.0, 1.0], 3)
    # the branch's loss (:1567-1643) is the plain sum of the four per-utterance terms, every list its own (:1589-1590): loss_terms
    # in that form against the restatement's figures on stand-in trajectories; the window form (:1393) differs for three utterances
    import synth
    import trainlog_ref as tref
    B, T = items[0].shape[:2]
    trajs = [{s: synth.normal("ul/args/%d%s" % (i, s), (B, T, 2 * P.lat_dim if s in ("lat", "latcv") else P.out_dim)) * 0.5 for s in U.SLOTS}
             for i in range(2)]
    R = tref.window_record(trajs, items[0].numpy(), P.stdim, P.lat_dim, items[7].numpy(), [0, 1, 2], kw["flen_acc"], np.zeros(3), np.array(items[13]) - 1, 0)
    want = float(np.sum(R[:, :, [0, 1, 3, 4]]))
    tt = [{s: torch.from_numpy(v).double() for s, v in tr.items()} for tr in trajs]
    form = lambda q: float(stage4.loss_terms(tt, items[0].double(), P.stdim, P.lat_dim, kw["flen_acc"], kw["select_utt_idx"], list_quirk=q))
    assert abs(form(False) - want) <= 1e-6 * abs(want), (form(False), want)      # (the weights are fp32 1/n: ~6e-8 relative)
    assert abs(form(True) - want) > 1e-3 * abs(want)
    import trainlog_util
    with pytest.raises(ValueError, match="22-field"):
        stage4.utterance_step_args(next(trainlog_util.yields(U.e2e_batches(P, "ul/args")[0], 8, torch.from_numpy)))
    with pytest.raises(ValueError, match="sentinel"):
        stage4.utterance_step_args(U.sentinel())
    z = list(items)
    z[11] = np.array([23, 24, 9])
    with pytest.raises(ValueError, match="do not fit the 23 padded frames"):
        stage4.utterance_step_args(tuple(z))
