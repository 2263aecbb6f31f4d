"""TEST INFRASTRUCTURE shared by tests/test_decode_cpu.py (emulator build, numpy / CPU-tensor memory) and tests/test_decode_gpu.py
(the device): fixtures of cvae_mc2e_batch, cvae_decode_jobs and the end-to-end stage-6 problem, and runners that take a `backend`
(validation_util.NpBackend / TorchBackend) or a torch device so that one body serves both."""
import numpy as np

import _cabi
import synth
import validation_util as VU
import stage5_util as S
import decode_ref as dref
from oracle import cyclevae_oracle as orc

ALPHA = 0.455
TIGHT_PASS = S.TIGHT_PASS
MC2E_REL = 1e-11           # the project's bound for cvae_mc2e (tests/test_gpu_parity.py::test_mc2e_and_mod_pow_on_device)
GUARD = 2

# ---- cvae_mc2e_batch -----------------------------------------------------------------------------------------------------------

_MC2E_REF = {}


def mc2e_matrix(tag, T, D, f64, pad):
    """[T, D + pad] in float32 or float64: the first D columns are a frame's coefficients (the decay of test_mc2e_and_mod_pow_on_device),
    the others poison that no kernel may read into a result."""
    m = np.full((T, D + pad), 1e30, np.float64 if f64 else np.float32)
    m[:, :D] = synth.normal("dec/mc2e/" + tag, (T, D)) * np.linspace(1.5, 0.05, D)
    return m


def mc2e_ref(tag, m, D, irlen):
    """oracle.mc2e of a fixture matrix: computed once, shared, never changed."""
    key = (tag, m.shape, str(m.dtype), D, irlen)
    if key not in _MC2E_REF:
        _MC2E_REF[key] = orc.mc2e(m[:, :D], ALPHA, irlen)
    return _MC2E_REF[key]


def run_mc2e_batch(be, mats, D, irlen, alpha=ALPHA):
    """ONE cvae_mc2e_batch call over the matrices (job q reads the first D[q] columns).  Every job's e_out is followed by GUARD
    poisoned values (the next job's starts right behind them).  Returns the list of (e [T], guard [GUARD])."""
    Ds = D if isinstance(D, (list, tuple)) else [D] * len(mats)
    rows = [m.shape[0] for m in mats]
    out = be.empty((sum(rows) + GUARD * len(rows),), np.float64)      # (poisoned with -77)
    keep, jobs, at = [], [], 0
    for m, d in zip(mats, Ds):
        dm = be.put(m)
        keep.append(dm)
        jobs.append(_cabi.Mc2eJob(be.ptr(dm), int(m.dtype == np.float64), m.shape[0], d, 0, m.shape[1], be.ptr(out) + 8 * at))
        at += m.shape[0] + GUARD
    nb = be.lib.mc2e_batch_work_bytes(len(jobs), max(Ds), irlen)
    assert nb > 0
    work = be.empty((nb,), np.uint8)
    be.lib.mc2e_batch(jobs, alpha, irlen, be.ptr(work), nb, be.stream)
    host, res, at = be.get(out), [], 0
    for r in rows:
        res.append((host[at:at + r], host[at + r:at + r + GUARD]))
        at += r + GUARD
    return res


def check_mc2e_batch(be, irlen, D, frames=(1, 7, 33), tag=None):
    """Jobs of `frames` frames in one call, fp32 and f64 alternating, ld = D + 3, against oracle.mc2e at MC2E_REL relative."""
    tag = tag or "%d_%d" % (irlen, D)
    mats = [mc2e_matrix("%s/%d" % (tag, q), T, D, q % 2 == 1, 3) for q, T in enumerate(frames)]
    got = run_mc2e_batch(be, mats, D, irlen)
    worst = 0.0
    for q, ((e, guard), m) in enumerate(zip(got, mats)):
        assert np.all(guard == -77), "values behind job %d's energies were written" % q
        ref = mc2e_ref("%s/%d" % (tag, q), m, D, irlen)
        assert np.all(np.isfinite(e)) and np.all(e > 0)
        worst = max(worst, float(np.max(np.abs(e / ref - 1.0))))
    print("mc2e_batch irlen=%d D=%d jobs=%d rel|d| vs the oracle = %.3e" % (irlen, D, len(frames), worst))
    assert worst <= MC2E_REL, (irlen, D, worst)
    return mats, got


def check_mc2e_many_jobs(be, n_jobs=24, irlen=64):
    """24 jobs of 1 .. 3 frames and of D = 2 .. 25 in one call: every job finds its own frames, coefficients and output."""
    Ds = [2 + (7 * q) % 24 for q in range(n_jobs)]
    mats = [mc2e_matrix("many/%d" % q, 1 + q % 3, Ds[q], q % 2 == 0, q % 4) for q in range(n_jobs)]
    got = run_mc2e_batch(be, mats, Ds, irlen)
    for q, ((e, guard), m) in enumerate(zip(got, mats)):
        assert np.all(guard == -77), q
        ref = mc2e_ref("many/%d" % q, m, Ds[q], irlen)
        assert float(np.max(np.abs(e / ref - 1.0))) <= MC2E_REL, (q, Ds[q], e, ref)


def check_mc2e_refusals(be):
    """irlen outside 2 .. 4000, D < 2, ld < D, no frames, no jobs: status -1 with a message, nothing launched."""
    m = mc2e_matrix("bad", 3, 4, True, 0)
    out = np.zeros(3)
    ok = _cabi.Mc2eJob(m.ctypes.data, 1, 3, 4, 0, 4, out.ctypes.data)
    work = np.zeros(1 << 20, np.uint8)
    for jobs, irlen in (([ok], 1), ([ok], 4001), ([], 64), ([_cabi.Mc2eJob(m.ctypes.data, 1, 3, 1, 0, 4, out.ctypes.data)], 64),
                        ([_cabi.Mc2eJob(m.ctypes.data, 1, 3, 4, 0, 3, out.ctypes.data)], 64), ([_cabi.Mc2eJob(m.ctypes.data, 1, 0, 4, 0, 4, out.ctypes.data)], 64),
                        ([_cabi.Mc2eJob(None, 1, 3, 4, 0, 4, out.ctypes.data)], 64), ([_cabi.Mc2eJob(m.ctypes.data, 1, 3, 4, 0, 4, None)], 64)):
        try:
            be.lib.mc2e_batch(jobs, ALPHA, irlen, work.ctypes.data, work.nbytes)
        except _cabi.CvaeError as err:
            assert "cvae_mc2e_batch" in str(err) and "(-1)" in str(err), str(err)
        else:
            raise AssertionError("cvae_mc2e_batch accepted irlen=%d with %d jobs" % (irlen, len(jobs)))
    assert be.lib.mc2e_batch_work_bytes(1, 4, 1) == 0 and be.lib.mc2e_batch_work_bytes(1, 4, 4001) == 0
    try:
        be.lib.mc2e_batch([ok], ALPHA, 64, work.ctypes.data, 8)
    except _cabi.CvaeError as err:
        assert "(-2)" in str(err)
    else:
        raise AssertionError("cvae_mc2e_batch accepted a work buffer of 8 bytes")
    assert np.all(out == 0)


# ---- cvae_decode_jobs ----------------------------------------------------------------------------------------------------------

def modpow_inputs(T, D=50):
    """The inputs of test_mc2e_and_mod_pow_on_device, for T frames."""
    cv = (synth.normal("mc2e/cv", (37, D)) * np.linspace(1.5, 0.05, D)).astype(np.float32)[:T]
    rf = (cv + 0.1 * synth.normal("mc2e/rf", (37, D))[:T] * np.linspace(1.0, 0.05, D)).astype(np.float64)
    gv_t = (0.05 + synth.uniform01("mc2e/gv", (D - 1,))).astype(np.float64)
    cg = (0.02 + 0.5 * synth.uniform01("mc2e/cg", (D - 1,))).astype(np.float64)
    return cv, rf, gv_t, cg


def run_decode_jobs(be, jobs):
    n = len(jobs) * _cabi.C.sizeof(_cabi.DecodeJob)
    work = be.empty((n,), np.uint8)
    be.lib.decode_jobs(jobs, be.ptr(work), n, be.stream)


def check_decode_jobs(be, T, irlen=64):
    """The two rounds of a trajectory in stage 6 against the oracle: (A) mod_pow + post-filter + variance + difference of an fp32
    trajectory and, in the same launch, a mod_pow without post-filter of an f64 one with ld > D; (B) mod_pow in place of A's
    post-filtered array, with its difference.  dpow at 1e-11 absolute, arrays and variances at 1e-10 absolute
    (test_mc2e_and_mod_pow_on_device's bounds); GUARD rows behind every output keep their fill."""
    cv, rf, gv_t, cg = modpow_inputs(T)
    D = cv.shape[1]
    wide = np.full((T, D + 5), 1e30, np.float64)
    wide[:, :D] = cv
    (e_cv, _), (e_rf, _) = run_mc2e_batch(be, [cv, rf], D, irlen)
    d = {k: be.put(v) for k, v in (("cv", cv), ("rf", rf), ("gv", gv_t), ("cg", cg), ("wide", wide), ("e_cv", e_cv), ("e_rf", e_rf))}
    o = {k: be.empty(shape, np.float64) for k, shape in (("x", (T + GUARD, D)), ("g", (T + GUARD, D)), ("diff", (T + GUARD, D)),
                                                         ("var", (D - 1 + GUARD,)), ("dpow", (T + GUARD,)), ("x2", (T + GUARD, D)))}
    p = lambda k: be.ptr(d[k]) if k in d else be.ptr(o[k])
    A = _cabi.DecodeJob(_cabi.DEC_MODPOW, T, D, 0, 1, 0, 0, 0, p("cv"), D, p("e_rf"), p("e_cv"), p("gv"), p("cg"), p("x"), p("g"), p("var"),
                        p("dpow"), p("rf"), D, p("diff"), None)
    A2 = _cabi.DecodeJob(_cabi.DEC_MODPOW, T, D, 1, 0, 0, 0, 0, p("wide"), D + 5, p("e_rf"), p("e_cv"), None, None, p("x2"), None, None, None,
                         None, 0, None, None)
    run_decode_jobs(be, [A, A2])
    h = {k: be.get(v) for k, v in o.items()}
    dp = orc.mod_pow_dpow(cv, rf, ALPHA, irlen)
    x_ref = cv.astype(np.float64)
    x_ref[:, 0] += dp
    g_ref, var_ref = orc.gv_postfilter(cv, gv_t, cg, dp)
    for k in o:
        assert np.all(h[k][-GUARD:] == -77), "rows behind %s were written" % k
    err = {"dpow": np.max(np.abs(h["dpow"][:T] - dp)), "x": np.max(np.abs(h["x"][:T] - x_ref)), "x2": np.max(np.abs(h["x2"][:T] - x_ref)),
           "g": np.max(np.abs(h["g"][:T] - g_ref)), "var": np.max(np.abs(h["var"][:D - 1] - var_ref)),
           "diff": np.max(np.abs(h["diff"][:T] - (x_ref - rf)))}
    print("decode_jobs T=%d round A: %s" % (T, "  ".join("%s %.2e" % kv for kv in err.items())))
    assert err["dpow"] <= 1e-11 and max(err.values()) <= 1e-10, err
    # round B: the post-filtered array's own mod_pow, in place (its energies from the array the job wrote)
    g_own = h["g"][:T].copy()
    (e_g, _), = run_mc2e_batch(be, [g_own], D, irlen)
    d["e_g"] = be.put(e_g)
    o2 = {"diff2": be.empty((T + GUARD, D), np.float64)}
    B = _cabi.DecodeJob(_cabi.DEC_MODPOW, T, D, 1, 1, 0, 0, 0, be.ptr(o["g"]), D, p("e_rf"), p("e_g"), None, None, be.ptr(o["g"]), None, None,
                        None, p("rf"), D, be.ptr(o2["diff2"]), None)
    run_decode_jobs(be, [B])
    gb, diff2 = be.get(o["g"]), be.get(o2["diff2"])
    gb_ref = dref.mod_pow(g_own, rf, ALPHA, irlen)
    assert np.all(gb[-GUARD:] == -77) and np.all(diff2[-GUARD:] == -77)
    assert np.array_equal(gb[:T, 1:], g_own[:, 1:]), "mod_pow moved a coefficient other than 0"
    eb = (float(np.max(np.abs(gb[:T] - gb_ref))), float(np.max(np.abs(diff2[:T] - (gb_ref - rf)))))
    print("decode_jobs T=%d round B: out %.2e  diff %.2e" % ((T,) + eb))
    assert max(eb) <= 1e-10, eb


def check_decode_gather(be):
    """The gather kind: f64 and fp32 sources wider than the window, an index outside the source gives a NaN row."""
    src64 = synth.normal("dec/gather/a", (9, 7)).astype(np.float64)
    src32 = synth.normal("dec/gather/b", (9, 7)).astype(np.float32)
    idx = np.array([0, 8, 3, 3, 9, -1, 5], np.int64)
    d64, d32, di = be.put(src64), be.put(src32), be.put(idx)
    o64, o32 = be.empty((len(idx) + GUARD, 4), np.float64), be.empty((len(idx) + GUARD, 7), np.float64)
    G = lambda src, f64, c0, c1, dst: _cabi.DecodeJob(_cabi.DEC_GATHER, len(idx), 7, f64, 0, 9, c0, c1, be.ptr(src), 7, None, None, None, None,
                                                      be.ptr(dst), None, None, None, None, 0, None, be.ptr(di))
    run_decode_jobs(be, [G(d64, 1, 2, 6, o64), G(d32, 0, 0, 7, o32)])
    ok = (idx >= 0) & (idx < 9)
    for got, want in ((be.get(o64), src64[:, 2:6]), (be.get(o32), src32.astype(np.float64))):
        assert np.all(got[-GUARD:] == -77)
        assert np.array_equal(got[:len(idx)][ok], want[idx[ok]]) and np.all(np.isnan(got[:len(idx)][~ok]))


def check_decode_refusals(be):
    x = np.zeros((3, 4))
    bad = [_cabi.DecodeJob(7, 3, 4, 1, 0, 0, 0, 0, x.ctypes.data, 4, None, None, None, None, x.ctypes.data, None, None, None, None, 0, None, None),
           _cabi.DecodeJob(_cabi.DEC_MODPOW, 3, 1, 1, 0, 0, 0, 0, x.ctypes.data, 4, None, None, None, None, x.ctypes.data, None, None, None, None, 0, None, None),
           _cabi.DecodeJob(_cabi.DEC_MODPOW, 3, 4, 1, 0, 0, 0, 0, x.ctypes.data, 4, None, None, x.ctypes.data, None, x.ctypes.data, None, None, None, None, 0, None,
                           None),
           _cabi.DecodeJob(_cabi.DEC_GATHER, 3, 4, 1, 0, 3, 0, 4, x.ctypes.data, 4, None, None, None, None, x.ctypes.data, None, None, None, None, 0, None, None)]
    work = np.zeros(4096, np.uint8)
    for j in bad:
        try:
            be.lib.decode_jobs([j], work.ctypes.data, work.nbytes)
        except _cabi.CvaeError as err:
            assert "cvae_decode_jobs" in str(err) and "(-1)" in str(err)
        else:
            raise AssertionError("cvae_decode_jobs accepted a bad job")


# ---- the end-to-end problem ----------------------------------------------------------------------------------------------------

E2E_LENS = ((24, 30), (27, 20), (22, 38))          # (source, target) frames of the three pairs: ragged, 20..38
E2E_IRLEN, E2E_SMPL = 64, 2


def problem(tag="dec", lens=E2E_LENS, n_smpl=E2E_SMPL, **dims):
    """The synthetic stage-6 set: weights, per pair (feat_src, feat_trg, spcidx_src, spcidx_trg, mcep_src, mcep_trg) and (eps_src,
    eps_trg), the y_in vectors, the statistics (gv_mean_src, gv_mean_trg, cvgv_mean, cvgvsrc_mean, cvgvtrg_mean).  Speech frames: a
    non-contiguous increasing subset (about 70 %) of each utterance; mcep: the utterance's own spectral features plus analysis
    noise, in float64, for EVERY frame (the script analyses the waveform again, :259 and :272)."""
    d = dict(VU.H64)
    d.update(dims)
    P = synth.CycleVAEProblem(B=1, T=4, tag=tag, **d)
    sd = P.stdim
    items, eps = [], []
    for k, (ts, tt) in enumerate(lens):
        it = []
        for side, T in (("src", ts), ("trg", tt)):
            feat = synth.features("%s/p%d/%s" % (tag, k, side), 1, T, P.mu, P.sigma)[0]
            keep = np.nonzero(synth.uniform01("%s/p%d/%s/spc" % (tag, k, side), (T,)) < 0.7)[0]
            keep = keep if len(keep) > 1 else np.arange(2)
            mc = feat[:, sd:].astype(np.float64) + 0.1 * synth.normal("%s/p%d/%s/mc" % (tag, k, side), (T, P.out_dim)).astype(np.float64)
            it.append((feat, keep.astype(np.int64), mc))
        items.append((it[0][0], it[1][0], it[0][1], it[1][1], it[0][2], it[1][2]))
        eps.append((synth.normal("%s/p%d/eps_src" % (tag, k), (n_smpl, ts, P.lat_dim)), synth.normal("%s/p%d/eps_trg" % (tag, k), (n_smpl, tt, P.lat_dim))))
    y_pp, y_trg = P.y_in_enc[:1], P.y_in_dec[:1]
    y_src = (0.5 * P.y_in_dec[:1]).astype(np.float32)          # (the script passes one vector for both; two catch a swap)
    stats = tuple(synth.uniform("%s/%s" % (tag, n), (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
                  for n in ("gv_src", "gv_trg", "cvgv", "cvgvsrc", "cvgvtrg"))
    return P, items, eps, (y_pp, y_src, y_trg), stats


to_dev = S.to_dev
assert_close = S.assert_close


def make_pass(P, dev, stats, n_smpl=E2E_SMPL, irlen=E2E_IRLEN, like=None):
    """like: another pass whose modules (and prepared weight images) this one shares."""
    import decode
    enc, dec = (like.enc, like.dec) if like is not None else (m.eval() for m in VU.modules(P, dev))
    return decode.DecodePass(enc, dec, P.lat_dim, *stats, n_smpl_dec=n_smpl, mcep_alpha=ALPHA, irlen=irlen)


def host(r):
    """a per-pair result with its device tensors as numpy"""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def same_results(a, b, what):
    a, b = host(a), host(b)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k, a[k], b[k])


_ORACLE, _E2E = {}, {}


def oracle_passes():
    """The oracle network on the three pairs of problem(): computed once, shared, never changed."""
    if "o" not in _ORACLE:
        P, items, eps, (y_pp, y_src, y_trg), _ = problem()
        _ORACLE["o"] = [dref.network_passes(P.enc, P.dec, it[0], it[1], y_pp, y_src, y_trg, e[0], e[1], P.lat_dim) for it, e in zip(items, eps)]
    return _ORACLE["o"]


def run_e2e(dev):
    """Three pairs as a call of two and a call of one (H = 64, n_smpl_dec = 2, irlen = 64, eps injected).  The five trajectories and
    two latent means against the oracle network at TIGHT_PASS; every other output against decode_ref run on the call's OWN
    last_passes at 1e-10 relative to the array's scale (DTW path choices must not hang on the network's last bits); then the same
    pairs as one call of three: every per-pair output bit for bit.  Returns (the pass, the per-pair results, the RefDecode)."""
    key = str(dev)
    if key in _E2E:
        return _E2E[key]
    P, items, eps, y, stats = problem()
    ty = to_dev(y, dev)
    dp = make_pass(P, dev, stats)
    ref = dref.RefDecode(stats[0], stats[1])
    want_net = oracle_passes()
    results = []
    for lo, hi in ((0, 2), (2, 3)):
        got = dp.pairs([to_dev(it, dev) for it in items[lo:hi]], *ty, eps=[to_dev(e, dev) for e in eps[lo:hi]], first_pair_id=lo)
        assert len(got) == hi - lo and len(dp.last_passes) == hi - lo
        for q, r in enumerate(got):
            own = {k: v.cpu().numpy() for k, v in dp.last_passes[q].items()}
            assert set(own) == set(dref.PASS_NAMES)
            for k in dref.PASS_NAMES:
                d = float(np.max(np.abs(own[k] - want_net[lo + q][k])))
                print("e2e pair %d %-12s max|d| vs the oracle network = %.3e" % (lo + q, k, d))
                assert own[k].shape == want_net[lo + q][k].shape and d <= TIGHT_PASS, (lo + q, k, d)
            it = items[lo + q]
            want = dref.pair_results(own, it[2], it[3], it[4], it[5], *stats, alpha=ALPHA, irlen=E2E_IRLEN)
            ref.add(want)
            h = host(r)
            assert set(h) == set(want), set(h) ^ set(want)
            assert len(dref.TRAJ_NAMES) == 8 and len(dref.MCD_TERMS + dref.DIST_TERMS) == 22 and len(dref.GV_TERMS) == 6
            for k, v in want.items():
                assert_close(h[k], v, 1e-10, "pair %d %s" % (lo + q, k))
            results.append(r)
    s, s_ref = dp.summary(), ref.summary()
    assert set(s) == set(s_ref)
    for k, v in s_ref.items():
        assert_close(s[k], v, 1e-10, k)
    # grouping
    dp3 = make_pass(P, dev, stats, like=dp)
    got3 = dp3.pairs([to_dev(it, dev) for it in items], *ty, eps=[to_dev(e, dev) for e in eps])
    for q in range(3):
        same_results(results[q], got3[q], "pair %d, one call of three against 2 + 1" % q)
    _E2E[key] = (dp, [host(r) for r in results], ref)
    return _E2E[key]


def run_log_lines(dev):
    """log_lines() is the script's text of :606-644 for the three-pair case."""
    dp, _, ref = run_e2e(dev)
    got, want = dp.log_lines(), ref.log_lines()
    assert len(want) == 19 and want[3].startswith("mcd_cvGV: ") and want[-1].startswith("lat_dist_cosim_pri: ")
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b]


def run_launch_count(dev, monkeypatch):
    """A one-pair call and a three-pair call make the same library calls: one latent_mean, two eval_stats, one dtw_batch, two
    mc2e_batch, three decode_jobs."""
    import gru_vae
    P, items, eps, y, stats = problem(tag="dec/count", lens=((8, 9), (10, 8), (9, 10)))
    dp = make_pass(P, dev, stats)
    ty = to_dev(y, dev)
    dp.pairs([to_dev(items[0], dev)], *ty, eps=[to_dev(eps[0], dev)])       # (binds the library, prepares the images)
    count = S.CallCounter(monkeypatch, gru_vae._lib(), names=("latent_mean", "eval_stats", "dtw_batch", "mc2e_batch", "decode_jobs", "mc2e",
                                                              "gv_postfilter", "dtw_org_to_trg", "mcd_aligned"))
    for N in (1, 3):
        res = dp.pairs([to_dev(it, dev) for it in items[:N]], *ty, eps=[to_dev(e, dev) for e in eps[:N]])
        assert len(res) == N
        assert count.take() == {"latent_mean": 1, "eval_stats": 2, "dtw_batch": 1, "mc2e_batch": 2, "decode_jobs": 3, "mc2e": 0,
                                "gv_postfilter": 0, "dtw_org_to_trg": 0, "mcd_aligned": 0}, N


def run_closing_the_loop(dev):
    """cvgv*_mean taken from a CvgvPass over the same pairs: the post-filtered trajectory of pair q has the variance
    gv_mean_trg * cvgv_q / cvgv_mean, cvgv_q the pair's own raw GV."""
    import stage5
    P, items, eps, y, stats = problem()
    ty = to_dev(y, dev)
    enc, dec = (m.eval() for m in VU.modules(P, dev))
    cp = stage5.CvgvPass(enc, dec, P.lat_dim, stats[0], stats[1], n_smpl_dec=E2E_SMPL)
    s5 = [it[:4] + (it[4][it[2]], it[5][it[3]]) for it in items]
    cp.pairs([to_dev(it, dev) for it in s5], *ty, eps=[to_dev(e, dev) for e in eps])
    s = cp.summary()
    import decode
    dp = decode.DecodePass(enc, dec, P.lat_dim, stats[0], stats[1], s["cvgv_mean"], s["cvgvsrc_mean"], s["cvgvtrg_mean"], n_smpl_dec=E2E_SMPL,
                           irlen=E2E_IRLEN)
    got = dp.pairs([to_dev(it, dev) for it in items], *ty, eps=[to_dev(e, dev) for e in eps])
    for q, r in enumerate(got):
        assert np.array_equal(r["cvlist"], cp.acc["cvgv"][q])
        for name, raw, gv, mean in (("cvmcep_gv", "cvlist", stats[1], "cvgv_mean"), ("cvmcep_src_gv", "cvlist_src", stats[0], "cvgvsrc_mean"),
                                    ("cvmcep_trg_gv", "cvlist_trg", stats[1], "cvgvtrg_mean")):
            want = gv * r[raw] / s[mean]
            assert_close(np.var(r[name].cpu().numpy()[:, 1:], axis=0), want, 1e-10, "pair %d GV of %s" % (q, name))
            assert_close(r[name.replace("cvmcep", "cvgvlist").replace("_gv", "")], want, 1e-10, "pair %d the library's own variance" % q)
    # the mean over the pairs of the post-filtered GV is the target speaker's
    assert_close(dp.summary()["cvgvlist_mean"], stats[1], 1e-10, "mean GV after the post-filter")


def run_bad_spcidx(dev):
    """A speech-frame index >= frames in pair 1 of 3: NaN in that pair's 22 figures only; pairs 0 and 2 bit-equal to the clean run."""
    import decode
    P, items, eps, y, stats = problem()
    ty = to_dev(y, dev)
    dp = make_pass(P, dev, stats)
    te = [to_dev(e, dev) for e in eps]
    clean = dp.pairs([to_dev(it, dev) for it in items], *ty, eps=te)
    bad = list(items[1])
    bad[2] = bad[2].copy()
    bad[2][-1] = items[1][0].shape[0]             # one past the source utterance's last frame
    got = dp.pairs([to_dev(items[0], dev), to_dev(bad, dev), to_dev(items[2], dev)], *ty, eps=te)
    for q in (0, 2):
        same_results(clean[q], got[q], "pair %d beside the bad one" % q)
    for k in decode.MCD_TERMS + decode.DIST_TERMS:
        assert np.isnan(got[1][k]) and np.isfinite(clean[1][k]), k
    for k in decode.GV_TERMS + decode.TRAJ_NAMES:      # (these do not read the index lists)
        assert np.array_equal(host(got[1])[k], host(clean[1])[k]), k


def run_argument_checks(dev):
    """Refused before anything is launched: 0 or 11 items, a cvgv_mean of the wrong length, mcep of the wrong shape, irlen 1 / 4001."""
    import pytest
    import decode
    P, items, eps, y, stats = problem()
    ty = to_dev(y, dev)
    dp = make_pass(P, dev, stats)
    dp.last_passes = "untouched"
    one = to_dev(items[0], dev)
    with pytest.raises(ValueError, match="pairs per call"):
        dp.pairs([], *ty)
    with pytest.raises(ValueError, match="pairs per call"):
        dp.pairs([one] * 11, *ty)
    with pytest.raises(ValueError, match="mcep_src has shape"):
        dp.pairs([one[:4] + (one[4][:-1], one[5])], *ty)
    with pytest.raises(ValueError, match="mcep_trg has shape"):
        dp.pairs([one[:4] + (one[4], one[5][:, 1:])], *ty)
    assert dp.last_passes == "untouched"
    enc, dec = dp.enc, dp.dec
    with pytest.raises(ValueError, match="cvgv_mean has"):
        decode.DecodePass(enc, dec, P.lat_dim, stats[0], stats[1], stats[2][:-1], stats[3], stats[4])
    for irlen in (1, 4001):
        with pytest.raises(ValueError, match="irlen"):
            decode.DecodePass(enc, dec, P.lat_dim, *stats, irlen=irlen)
    with pytest.raises(RuntimeError, match="no pair seen"):
        dp.summary()
