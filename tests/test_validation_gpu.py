"""The validation pass on the MI355X: tests/test_validation_cpu.py's cases (a)-(d) on the device, one alignment size whose
diagonals are wider than a block, and one ValidationPass.batch at H = 1024.  Yardsticks as in the CPU file (PARITY UNPINNED for
the DTW / calc_mcd halves: the oracle's written definition stands in for dtw_c)."""
import numpy as np
import pytest

import _cabi
import validation_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    import gru_vae
    assert torch.cuda.is_available()
    return U.TorchBackend(gru_vae._lib(), torch.device("cuda:0"))


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
    """(a) on the device: 24 mixed problems in one call, bit for bit the one-problem kernel's outputs, and the oracle's."""
    problems = U.mixed_problems()
    res = U.run_dtw_batch(be, problems)
    for r, (a, b, mcd) in zip(res, problems):
        what = "T1=%d T2=%d D=%d mcd=%d" % (a.shape[0], b.shape[0], a.shape[1], mcd)
        U.assert_bit_identical(r, U.run_dtw_single(be, a, b, mcd), what)
        U.assert_matches_oracle(r, a, b, mcd, what)


def test_dtw_batch_ties(be, cost_mode):
    """(b) on the device."""
    a, b, mcd = U.tie_problem()
    assert U.oracle_ties(a, b) == {"diag=up", "diag=left", "up=left"}
    r = U.run_dtw_batch(be, [(a, b, mcd), (b, a, mcd)])
    U.assert_matches_oracle(r[0], a, b, mcd, "ties")
    U.assert_matches_oracle(r[1], b, a, mcd, "ties, transposed")
    U.assert_bit_identical(r[0], U.run_dtw_single(be, a, b, mcd), "ties")


@pytest.fixture(scope="module")
def wide_oracle():
    """The largest oracle run of the file (its double loop takes a few seconds), shared by both cost modes."""
    from oracle import cyclevae_oracle as orc
    ps = [U.dtw_problem(300, 270, 26, -1, "wide_a"), U.dtw_problem(270, 300, 4, 0, "wide_b")]
    return ps, [orc.dtw_org_to_trg(a, b, mcd=m) for a, b, m in ps]


def test_dtw_batch_diagonals_wider_than_a_block(be, cost_mode, wide_oracle):
    """(300, 270) at D = 26 and (270, 300) at D = 4 cosine in one call: up to 270 cells per diagonal on 256 threads, rows in LDS."""
    ps, want = wide_oracle
    res = U.run_dtw_batch(be, ps)
    for r, (a, b, mcd), w in zip(res, ps, want):
        U.assert_bit_identical(r, U.run_dtw_single(be, a, b, mcd), "wide")
        assert np.array_equal(r[1], w[1]), "twf differs from the oracle's"
        assert np.max(np.abs(r[3] - w[3])) <= 1e-12 * np.max(np.abs(w[3]))


def test_dtw_batch_global_diagonals_and_no_aligned(be, cost_mode):
    """T1 above CVAE_DTW_LDS_ROWS (the diagonals live in the work buffer) beside a small problem, aligned = NULL."""
    tall = U.dtw_problem(2100, 3, 4, -1, "tall")
    small = U.dtw_problem(9, 14, 5, 0, "small")
    res = U.run_dtw_batch(be, [tall, small], want_aligned=False)
    for r, (a, b, mcd) in zip(res, (tall, small)):
        single = U.run_dtw_single(be, a, b, mcd)
        U.assert_bit_identical(r[1:], single[1:], "T1=%d" % a.shape[0])
        assert np.all(r[0] == -77)                       # (never written)
        U.assert_matches_oracle((single[0],) + r[1:], a, b, mcd, "T1=%d" % a.shape[0])


def test_dtw_many_wrapper(be):
    """stage6.dtw_many is stage6.dtw_org_to_trg per problem, bit for bit."""
    import torch
    import stage6
    ps = U.mixed_problems()[4:12]
    t = lambda a: torch.from_numpy(a).to(be.dev)
    got = stage6.dtw_many([(t(a), t(b), m) for a, b, m in ps])
    for g, (a, b, m) in zip(got, ps):
        w = stage6.dtw_org_to_trg(t(a), t(b), mcd=m)
        for x, y in zip(g, w):
            assert torch.equal(x, y)


def test_eval_stats_jobs(be):
    """(c) on the device: every job kind against numpy float64 at 1e-12 relative."""
    arrays, cases = U.stat_cases()
    U.assert_stats(U.run_stats(be, arrays, cases), cases)


def test_validation_pass_end_to_end(be):
    """(d) on the device: bounds and their derivation in tests/test_validation_cpu.py::test_validation_pass_end_to_end."""
    U.run_e2e(be.dev, 5e-6)


def test_validation_pass_h1024_finite_and_row_independent(be):
    """One ValidationPass.batch at H = 1024 (the recipe's dimensions), B = 2, T about 60.  Finite outputs, and row independence:
    utterance 0's figures do not depend on what else is in the batch.
      (i) the metric code on IDENTICAL trajectories -- the B = 2 pass outputs, and their row 0 alone -- gives utterance 0 the same
          figures bit for bit (every figure, the DTW-derived ones included).
      (ii) a B = 1 call of batch() on utterance 0.  Its passes have other row counts and may take another recurrence kernel (two or
          three rows: the word-exchange kernel); each kernel is within the project's pass bound of 5e-6 of the exact trajectory, so
          two of them are within delta = 1e-5 of each other.  Figures that are continuous in the trajectories are held to that:
          the loss terms to validation_util.loss_bounds(delta) and the speech-frame MCDs (no alignment) to K sqrt2 sqrt(D) delta
          (a frame's K sqrt(2 |e|^2) moves by at most K sqrt2 |de|_2).  The DTW-derived figures are covered by (i): a path may
          legitimately flip on a 1e-5 difference."""
    import torch
    import validation
    lens = ((((60, 55), (52, 58)), ((57, 60), (60, 49))),)
    P, batches, (y_pp, y_src, y_trg), (gv_src, gv_trg) = U.e2e_problem(tag="val1024", batches=lens, in_dim=54, out_dim=50, lat_dim=32,
                                                                       hidden=1024, bias_scale=0.05)
    dev = be.dev
    enc, dec = U.modules(P, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    src, trg, eps = batches[0]
    ts, tt, te = U.side_to_torch(src, dev), U.side_to_torch(trg, dev), {k: t(v) for k, v in eps.items()}
    vp = validation.ValidationPass(enc.eval(), dec.eval(), P.lat_dim, P.stdim, gv_src, gv_trg)
    got = vp.batch(ts, tt, t(y_pp), t(y_src), t(y_trg), eps=te)
    assert all(np.isfinite(v) for v in got.values()), got
    assert all(np.isfinite(v) for v in vp.summary().values())
    both = vp.metrics(ts, tt, vp.last_passes)
    row0 = lambda d: {k: (v[:1] if hasattr(v, "shape") and getattr(v, "ndim", 0) >= 1 else v) for k, v in d.items()}
    s0, t0, e0 = row0(ts), row0(tt), {k: v[:1] for k, v in te.items()}
    alone = vp.metrics(s0, t0, {k: v[:1].contiguous() for k, v in vp.last_passes.items()})
    for k, v in both.items():
        assert np.array_equal(v[:1], alone[k]), k                       # (i)
    vp1 = validation.ValidationPass(enc, dec, P.lat_dim, P.stdim, gv_src, gv_trg)
    one = vp1.batch(s0, t0, t(y_pp), t(y_src), t(y_trg), eps=e0)         # (ii)
    delta = 1e-5
    o_host = {k: v.cpu().numpy() for k, v in vp.last_passes.items()}
    bound = U.loss_bounds(o_host, src, trg, P.lat_dim, P.stdim, delta)
    for n in validation.LOSS_TERMS:
        d = abs(one[n] - float(both[n][0]))
        print("h1024 row 0 %-22s B=2 %.6f  B=1 %.6f  |d| %.2e  allowed %.2e" % (n, both[n][0], one[n], d, bound[n]))
        assert d <= bound[n], n
    for n in ("mcdpow_trg_trg", "mcd_trg_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg", "mcdpow_src_src", "mcd_src_src", "mcdpow_src_trg_src",
              "mcd_src_trg_src"):
        d = abs(one[n] - float(both[n][0]))
        assert d <= U.K * np.sqrt(2.0 * P.out_dim) * delta, (n, d)
