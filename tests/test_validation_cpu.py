"""The validation pass without a GPU: the batched DTW and statistics entry points (cvae_dtw_batch, cvae_eval_stats) of the real
library on the host-fiber emulator, and validation.ValidationPass end to end on it.

Yardsticks: cvae_dtw_org_to_trg (bit identity), oracle.dtw_org_to_trg (twf equal, costs to 1e-12 relative; PARITY UNPINNED --
dtw_c is not in the reference tree, the oracle's written definition stands in), numpy float64 (statistics jobs, 1e-12 relative),
tests/validation_ref.py (the restatement of train_gru_cyclevae_gauss_batch.py:837-1139)."""
import numpy as np
import pytest

import _cabi
import validation_util as U
from emu_util import bind_emulator, emu_lib


@pytest.fixture(scope="module")
def be():
    return U.NpBackend(emu_lib())


@pytest.fixture(params=[1, 0], ids=["cost_slab", "cost_on_the_fly"])
def cost_mode(request, be):
    be.lib.set_option("dtw_batch_cost", request.param)
    yield request.param
    be.lib.reset_options()


def test_abi_version_and_exports(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10
    for name in ("cvae_dtw_batch_work_bytes", "cvae_dtw_batch", "cvae_eval_stats"):
        assert name in _cabi.EXPORTS and hasattr(be.lib.lib, name)


def test_dtw_batch_mixed_shapes_bit_identical_and_oracle(be, cost_mode):
    """(a) 24 problems of mixed shape, dimension and cost kind in ONE call: every output is the one-problem entry point's bit for
    bit, and the oracle's (twf equal, costs 1e-12 relative)."""
    problems = U.mixed_problems()
    res = U.run_dtw_batch(be, problems)
    for r, (a, b, mcd) in zip(res, problems):
        what = "T1=%d T2=%d D=%d mcd=%d" % (a.shape[0], b.shape[0], a.shape[1], mcd)
        U.assert_bit_identical(r, U.run_dtw_single(be, a, b, mcd), what)
        U.assert_matches_oracle(r, a, b, mcd, what)


def test_dtw_batch_ties(be, cost_mode):
    """(b) exact ties: the oracle's path of this fixture passes through a tie of each of the three kinds, and twf is the oracle's."""
    a, b, mcd = U.tie_problem()
    assert U.oracle_ties(a, b) == {"diag=up", "diag=left", "up=left"}
    r = U.run_dtw_batch(be, [(a, b, mcd), (b, a, mcd)])
    U.assert_matches_oracle(r[0], a, b, mcd, "ties")
    U.assert_matches_oracle(r[1], b, a, mcd, "ties, transposed")
    U.assert_bit_identical(r[0], U.run_dtw_single(be, a, b, mcd), "ties")


def test_dtw_batch_global_diagonals_chunks_and_no_aligned(be, cost_mode):
    """The other paths of the entry point: T1 above CVAE_DTW_LDS_ROWS keeps the diagonals in the work buffer; a work buffer that
    holds one problem at a time runs the list in chunks; aligned = NULL is allowed; a strided operand (a column window)."""
    tall = U.dtw_problem(2100, 3, 4, -1, "tall")
    small = U.dtw_problem(9, 14, 5, 0, "small")
    res = U.run_dtw_batch(be, [tall, small], want_aligned=False)
    for r, (a, b, mcd) in zip(res, (tall, small)):
        single = U.run_dtw_single(be, a, b, mcd)
        U.assert_bit_identical(r[1:], single[1:], "T1=%d" % a.shape[0])
        assert np.all(r[0] == -77)                       # (never written)
    U.assert_matches_oracle((U.run_dtw_single(be, *tall)[0],) + res[0][1:], tall[0], tall[1], tall[2], "tall")
    # chunks: three problems through a buffer sized for one
    ps = [U.dtw_problem(20, 17, 6, -1, "c%d" % k) for k in range(3)]
    keep, probs = [], []
    for a, b, mcd in ps:
        o = (be.empty((17, 6), np.float64), be.empty((17,), np.int64), be.empty((17,), np.float64), be.empty((1,), np.float64))
        keep.append(o)
        # operands as column windows 1.. of a wider matrix: row stride 7, D = 6
        wa, wb = np.zeros((20, 7)), np.zeros((17, 7))
        wa[:, 1:], wb[:, 1:] = a, b
        keep.append((wa, wb))
        probs.append(_cabi.DtwProblem(wa.ctypes.data + 8, wb.ctypes.data + 8, 7, 7, 20, 17, 6, mcd, o[0].ctypes.data, o[1].ctypes.data,
                                      o[2].ctypes.data, o[3].ctypes.data))
    nb = be.lib.dtw_batch_work_bytes(1, 20, 17)
    assert nb < be.lib.dtw_batch_work_bytes(3, 20, 17)
    work = np.zeros(nb, np.uint8)
    be.lib.dtw_batch(probs, work.ctypes.data, nb)
    for k, (a, b, mcd) in enumerate(ps):
        o = keep[2 * k]
        U.assert_bit_identical((o[0], o[1], o[3][0], o[2]), U.run_dtw_single(be, a, b, mcd), "chunk %d" % k)
    with pytest.raises(_cabi.CvaeError):
        be.lib.dtw_batch(probs, work.ctypes.data, 64)
    bad = _cabi.DtwProblem(probs[0].org, probs[0].trg, 7, 7, 0, 17, 6, -1, None, probs[0].twf, probs[0].frames, probs[0].mean_out)
    with pytest.raises(_cabi.CvaeError):
        be.lib.dtw_batch([bad], work.ctypes.data, nb)


def test_eval_stats_jobs(be):
    """(c) every job kind against numpy float64 at 1e-12 relative, all in one launch."""
    arrays, cases = U.stat_cases()
    U.assert_stats(U.run_stats(be, arrays, cases), cases)


# ---- (d) end to end ------------------------------------------------------------------------------------------------------------

@pytest.fixture
def emu_gru_vae(monkeypatch):
    return bind_emulator(monkeypatch)


def test_validation_pass_end_to_end(emu_gru_vae):
    """(d) ValidationPass on the H = 64 synthetic problem.

    Network-derived quantities (the ten loss terms and the batch loss) against the restatement on the ORACLE network.  The project's
    pass bound is max|d| <= 5e-6 on a trajectory (TIGHT_PASS); with delta = 5e-6 on every pass output
        loss_mcd_* = mean_t K sqrt2 sum_d |x_d - y_d|             moves by <= K sqrt2 D delta       (D = 26: 8.0e-4 dB)
        loss_lat_* = mean_t 0.5 sum_l (exp(s) + mu^2 - s - 1)     moves by <= 0.5 L delta (exp(s_max + delta) + 2 |mu|_max + delta + 1)
    per utterance and therefore per batch mean (validation_util.loss_bounds evaluates these on the reference's own arrays), plus the
    fp32 rounding of the reference's own reductions, 1e-6 relative; the batch loss is allowed the sum over its eight terms.

    Metric-derived quantities (dB figures, their stds, latent distances, eval_gv_*, the checkpoint decision) against the restatement
    run with trajectories= the library's own pass outputs, at 1e-10 relative: the new metric code and its yardstick see identical
    inputs, so a path flip from a 1e-6 difference upstream can neither hide nor fake a failure.  PARITY UNPINNED for the DTW and
    calc_mcd halves (validation_ref)."""
    import torch
    U.run_e2e(torch.device("cpu"), 5e-6)


def test_validation_pass_refuses_cpu_tensors():
    import torch
    import validation
    P, batches, (y_pp, y_src, y_trg), (gv_src, gv_trg) = U.e2e_problem()
    enc, dec = U.modules(P, torch.device("cpu"))
    src, trg, eps = batches[1]
    vp = validation.ValidationPass(enc, dec, P.lat_dim, P.stdim, gv_src, gv_trg)
    t = torch.from_numpy
    with pytest.raises(RuntimeError, match="HIP device only"):
        vp.batch(U.side_to_torch(src, "cpu"), U.side_to_torch(trg, "cpu"), t(y_pp), t(y_src), t(y_trg))
