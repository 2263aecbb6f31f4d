"""TEST INFRASTRUCTURE shared by tests/test_laplace_metrics_cpu.py (emulator build) and tests/test_laplace_metrics_gpu.py (the
device): the Laplace posterior in the metric passes -- CVAE_STAT_KL_LAPLACE, cvae_trainlog_window with L | CVAE_DRAW_LAPLACE, and
validation.ValidationPass, stage5.CvgvPass, decode.DecodePass, trainlog.TrainLog / UttLog with posterior="laplace".  One body per
case; a case takes a `be` (validation_util's NpBackend / TorchBackend) or a device.  Yardstick: tests/laplace_metrics_ref.py.

The end-to-end problems are the existing ones (validation_util.e2e_problem, stage5_util.problem, decode_util.problem,
trainlog_util.e2e_batches) under tags of their own, with two changes: the eps are the reference's uniforms in (-0.4999, 0.5) -- one
entry exactly 0, one within 1e-4 of each end -- and the encoder's last log-scale bias is -7.75, below the Laplace floor, so that some
log-scales sit on it (every case asserts that count)."""
import numpy as np

import _cabi
import synth
import decode_ref as dref
import decode_util as DU
import laplace_metrics_ref as R
import stage5_util as SU
import trainlog_util as TU
import uttlog_util as UU
import validation_util as VU
from laplace_chain_util import uniform_eps

FLOOR32 = np.float32(R.FLOOR)
LOW_BIAS = -7.75
BASE_DELTA = 5e-6          # what the Gaussian end-to-end tests of both backends allow a pass output (TIGHT_PASS)


def laplace_eps(tag, shape):
    e = uniform_eps(tag, shape)
    f = e.reshape(-1)
    f[0], f[1 % f.size], f[2 % f.size] = 0.0, -0.4999 + 5e-5, 0.5 - 5e-5
    return e


def lower_bias(P):
    P.enc["out_1.bias"][-1] = LOW_BIAS
    return P


def on_floor(*arrays_and_L):
    """number of log-scales equal to the floor in (array, L) pairs"""
    return sum(int(np.sum(np.asarray(a)[..., L:] == FLOOR32)) for a, L in arrays_and_L)


def delta_for(ref32, ref64, names, what):
    """frontend_util.bound_for's rule: BASE_DELTA, or four times the fp32 reference's distance to its float64 twin where that
    exceeds 1.25e-6."""
    d = max(float(np.max(np.abs(np.asarray(ref32[k], np.float64) - ref64[k]))) for k in names)
    delta = max(BASE_DELTA, 4.0 * d) if d > 1.25e-6 else BASE_DELTA
    print("%s: fp32 reference network vs its float64 twin max|d| = %.3e -> delta = %.3e" % (what, d, delta))
    return delta


def t_(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. the stat kind ----------------------------------------------------------------------------------------------------------

def kl_operand():
    """[300, 13] fp32 with L = 5: mu in columns 0..4 (some exactly 0), log-scales in 5..9 between the floor and +3 (some ON the floor),
    three columns of padding (a strided row)."""
    L, rows = 5, 300
    a = np.zeros((rows, 13), np.float32)
    a[:, :L] = synth.normal("lapm/kl/mu", (rows, L)) * 0.8
    s = synth.uniform("lapm/kl/s", (rows, L), -9.0, 3.0)
    a[:, L:2 * L] = np.maximum(s, FLOOR32)
    a[:, 2 * L:] = 1e6            # (never read)
    a[::7, 1] = 0.0
    a[0, 0] = 0.0
    a[0, L] = FLOOR32
    a[3, L + 2] = 3.0
    assert on_floor((a[:, :2 * L], L)) > 10 and np.sum(a[:, :L] == 0) > 10 and a[:, L:2 * L].max() == 3.0
    return a, L


def check_stat_kind(be):
    """CVAE_STAT_KL_LAPLACE at rows 1, 17 and 300 in ONE call beside jobs of every existing kind: 1e-12 of max(|ref|, the summand's
    condition); the existing kinds' results bit-identical to the call without the new jobs."""
    arrays, cases = VU.stat_cases()
    alone = VU.run_stats(be, arrays, cases)
    a, L = kl_operand()
    arrays = dict(arrays, lap=a)
    new, scales = [], []
    for rows in (1, 17, 300):
        ref, cond = R.kl_mean(a[:rows, :2 * L], L)
        new.append(("kl laplace rows=%d" % rows, dict(kind=_cabi.STAT_KL_LAPLACE, rows=rows, c0=0, c1=L, a=("lap", 0)), ref))
        scales.append(max(abs(ref), cond))
    both = cases[:5] + new[:1] + cases[5:] + new[1:]          # (the new jobs among the others, not behind them)
    got = dict(zip((c[0] for c in both), VU.run_stats(be, arrays, both)))
    for (name, _, _), r in zip(cases, alone):
        assert np.array_equal(got[name], r, equal_nan=True), "%s changed beside the new kind" % name
    VU.assert_stats([got[c[0]] for c in cases], cases)
    for (name, _, ref), scale in zip(new, scales):
        err = abs(float(got[name][0]) - ref)
        print("stats %-28s got %.15g ref %.15g |d| / scale = %.3e" % (name, float(got[name][0]), ref, err / scale))
        assert err <= 1e-12 * scale, (name, err, scale)


# ---- 2. the window kernel ------------------------------------------------------------------------------------------------------

def window_problem():
    """trainlog_util.kernel_problem (n_cyc 2, B 3, windows (0,7), (8,15), (16,22): utterance 2 unselected in the second, flen_acc 1 < T
    in the third) with latent trajectories whose log-scales reach from the floor to about +3 and some of whose means are 0."""
    d, x, spc, wins = TU.kernel_problem(tag="lapm/win")
    L = d["L"]
    for w in wins:
        for tr in w["trajs"]:
            for k in ("lat", "latcv"):
                tr[k][..., L:] = np.maximum(tr[k][..., L:] * np.float32(4.0) - np.float32(4.0), FLOOR32)
                tr[k][:, ::3, 1] = 0.0
    assert on_floor(*[(tr[k], L) for w in wins for tr in w["trajs"] for k in ("lat", "latcv")]) > 20
    return d, x, spc, wins


def run_windows(be, d, x, spc, wins, flag, rows=None, with_acc=True):
    """trainlog_util.run_kernel_windows with `flag` OR-ed into the argument block's L."""
    rows_ = list(range(x.shape[0])) if rows is None else rows
    B, F = len(rows_), x.shape[1]
    acc = [be.empty((B, F, d["D"]), np.float32) for _ in range(3)] + [be.empty((B, F, 2 * d["L"]), np.float32)] if with_acc else None
    recs, keep = [], []
    for w in wins:
        out = be.empty((d["n_cyc"], B, 9), np.float64)
        a = TU.window_args(be, d, None, x, spc, w, acc, out, keep, rows)
        a.L |= flag
        be.lib.trainlog_window(a, be.stream)
        recs.append(be.get(out))
    return recs, (None if acc is None else [be.get(t) for t in acc])


def require_kind_8(be):
    """A library from before this kind does not know the window's flag either and would take L | flag for a dimension of 2^30 + L:
    nothing is launched with the flag unless the library answers a one-row CVAE_STAT_KL_LAPLACE job (an unknown kind writes NaN)."""
    a = np.array([[0.5, -1.0]], np.float32)
    case = [("probe", dict(kind=_cabi.STAT_KL_LAPLACE, rows=1, c0=0, c1=1, a=("lap", 0)), R.kl_mean(a, 1)[0])]
    got = float(VU.run_stats(be, {"lap": a}, case)[0][0])
    assert np.isfinite(got) and abs(got - case[0][2]) <= 1e-12, "this library has no CVAE_STAT_KL_LAPLACE: the window's flag is not tried"


def check_window_kernel(be):
    import pytest
    require_kind_8(be)
    d, x, spc, wins = window_problem()
    plain, acc0 = run_windows(be, d, x, spc, wins, 0)
    got, acc1 = run_windows(be, d, x, spc, wins, _cabi.DRAW_LAPLACE)
    other = [0, 1, 2, 5, 6, 7, 8]
    for k, (g, p, w) in enumerate(zip(got, plain, wins)):
        want, scale = R.window_record(w["trajs"], x[:, w["s"]:w["e"] + 1], d["stdim"], d["L"], spc, w["sel"], w["flen_acc"], w["s_idx"],
                                      w["e_idx"], w["s"])
        assert np.array_equal(np.isnan(g), np.isnan(want)), "window %d: NaN pattern" % k
        m = ~np.isnan(want)
        err = np.abs(g[m] - want[m]) / scale[m]
        kl = np.abs(g[..., 3:5] - want[..., 3:5]) / scale[..., 3:5]
        print("window %d: %d figures, max |d| / scale %.3e (the two KL entries: %.3e)" % (k, int(m.sum()), float(err.max()), float(np.nanmax(kl))))
        assert np.all(err <= 1e-12), (k, float(err.max()))
        assert np.array_equal(g[..., other], p[..., other], equal_nan=True), "window %d: an entry besides [3], [4] changed" % k
        assert not np.array_equal(g[..., 3:5], p[..., 3:5], equal_nan=True)
    assert np.all(np.isnan(got[1][:, 2, :])) and np.all(np.isfinite(got[2][:, :2, :5])) and list(wins[2]["flen_acc"]) == [8, 1, 8]
    for a, b in zip(acc0, acc1):
        assert np.array_equal(a, b), "an accumulator changed with the flag"
    # grid independence: every utterance alone (nb = 1) against the launch of all B
    for j in range(x.shape[0]):
        one, _ = run_windows(be, d, x, spc, wins, _cabi.DRAW_LAPLACE, rows=[j], with_acc=False)
        for g, b in zip(one, got):
            assert np.array_equal(g, b[:, [j]], equal_nan=True), j
    # the flag alone is no dimension
    keep = []
    out = be.empty((d["n_cyc"], 3, 9), np.float64)
    a = TU.window_args(be, d, None, x, spc, wins[0], None, out, keep)
    a.L = _cabi.DRAW_LAPLACE
    with pytest.raises(_cabi.CvaeError):
        be.lib.trainlog_window(a, be.stream)


# ---- 3 / 4. validation.ValidationPass ------------------------------------------------------------------------------------------

def validation_problem(tag="lapm/val", **kw):
    P, batches, y, gv = VU.e2e_problem(tag=tag, **kw)
    lower_bias(P)
    out = []
    for k, (src, trg, eps) in enumerate(batches):
        out.append((src, trg, {n: laplace_eps("%s/b%d/u/%s" % (tag, k, n), e.shape) for n, e in eps.items()}))
    return P, out, y, gv


def run_validation_e2e(dev):
    """VU.run_e2e's body for posterior="laplace": loss terms against the restatement on the fp32 oracle network within
    validation_util.loss_bounds' bound for loss_mcd_* and laplace_metrics_ref.lat_bound for loss_lat_*, plus 1e-6 relative; the
    metric half on the library's own trajectories at 1e-10 relative."""
    import validation
    P, batches, (y_pp, y_src, y_trg), (gv_src, gv_trg) = validation_problem()
    enc, dec = VU.modules(P, dev)
    vp = validation.ValidationPass(enc.eval(), dec.eval(), P.lat_dim, P.stdim, gv_src, gv_trg, posterior="laplace")
    net, met = R.RefValidation(P, gv_src, gv_trg), R.RefValidation(P, gv_src, gv_trg)
    L, D, floor = P.lat_dim, P.out_dim, 0
    for src, trg, eps in batches:
        B = src["feat"].shape[0]
        got = vp.batch(VU.as_generator_yield(VU.side_to_torch(src, dev)), VU.as_generator_yield(VU.side_to_torch(trg, dev)), t_(y_pp, dev),
                       t_(y_src, dev), t_(y_trg, dev), eps={k: t_(v, dev) for k, v in eps.items()})
        rep = lambda y: np.repeat(y, B, 0)
        want_net, o_ref = net.batch(src, trg, rep(y_pp), rep(y_src), rep(y_trg), eps=eps)
        delta = delta_for(o_ref, R.validation_passes64(P, src, trg, rep(y_pp), rep(y_src), rep(y_trg), eps), R.vref.PASS_NAMES,
                          "validation B=%d" % B)
        own = {k: v.cpu().numpy() for k, v in vp.last_passes.items()}
        lats = [k for k in own if k.startswith("lat")]
        floor += on_floor(*[(own[k], L) for k in lats])
        assert all(float(own[k][..., L:].min()) >= FLOOR32 for k in lats)
        print("validation B=%d pass outputs max|d| vs the oracle network = %.3e" % (
            B, max(float(np.max(np.abs(own[k] - o_ref[k]))) for k in own)))
        want_met, _ = met.batch(src, trg, None, None, None, trajectories=own)
        tot = 0.0
        for n in R.vref.LOSS_TERMS:
            lat = {"loss_lat_trg": "lat_trg", "loss_lat_src": "lat_src", "loss_lat_trg_cv": "lat_trg_src", "loss_lat_src_cv": "lat_src_trg"}.get(n)
            bound = R.lat_bound(o_ref[lat], L, delta) if lat else VU.K * np.sqrt(2.0) * D * delta
            allow = bound + 1e-6 * abs(want_net[n])
            print("validation %-22s got %.6f  ref %.6f  |d| %.2e  allowed %.2e" % (n, got[n], want_net[n], abs(got[n] - want_net[n]), allow))
            assert abs(got[n] - want_net[n]) <= allow, n
            if n not in ("loss_mcd_trg_src", "loss_mcd_src_trg"):
                tot += allow
        assert abs(got["loss"] - want_net["loss"]) <= tot
        for n in R.vref.DB_TERMS + R.vref.DIST_TERMS:
            assert abs(got[n] - want_met[n]) <= 1e-10 * abs(want_met[n]), n
    assert floor > 0, "no log-scale on the Laplace floor"
    print("validation: %d log-scales on the floor" % floor)
    s, s_ref = vp.summary(), met.summary()
    assert set(s) == set(s_ref)
    for k, v in s_ref.items():
        if k.startswith(("eval_mcd", "eval_lat_dist", "eval_gv")):
            assert abs(s[k] - v) <= 1e-10 * abs(v), (k, s[k], v)
    assert validation.ValidationPass.better(s, None) and isinstance(validation.ValidationPass.log_line(s), str)


def check_validation_gauss_is_default(dev):
    import validation
    P, batches, y, gv = VU.e2e_problem(tag="lapm/valg", batches=((((22, 20),), ((25, 21),)),))      # (one utterance pair: the keyword is what is tested)
    enc, dec = (m.eval() for m in VU.modules(P, dev))
    src, trg, eps = batches[0]
    res = []
    for kw in ({}, {"posterior": "gauss"}):
        vp = validation.ValidationPass(enc, dec, P.lat_dim, P.stdim, gv[0], gv[1], **kw)
        got = vp.batch(VU.side_to_torch(src, dev), VU.side_to_torch(trg, dev), *(t_(v, dev) for v in y), eps={k: t_(v, dev) for k, v in eps.items()})
        res.append((got, {k: v.cpu().numpy() for k, v in vp.last_passes.items()}))
    assert res[0][0] == res[1][0]
    for k, v in res[0][1].items():
        assert np.array_equal(v, res[1][1][k]), k


# ---- 3 / 4. stage5.CvgvPass and decode.DecodePass ------------------------------------------------------------------------------

def pair_problem(util, tag, **kw):
    P, items, eps, y, stats = util.problem(tag=tag, **kw)
    lower_bias(P)
    eps = [tuple(laplace_eps("%s/p%d/u%d" % (tag, k, side), e.shape) for side, e in enumerate(pe)) for k, pe in enumerate(eps)]
    return P, items, eps, y, stats


def _pass_for(kind, P, dev, stats, n_smpl, like=None, **kw):
    import decode
    import stage5
    enc, dec = (like.enc, like.dec) if like is not None else (m.eval() for m in VU.modules(P, dev))
    if kind == "cvgv":
        return stage5.CvgvPass(enc, dec, P.lat_dim, stats[0], stats[1], n_smpl_dec=n_smpl, **kw)
    return decode.DecodePass(enc, dec, P.lat_dim, *stats, n_smpl_dec=n_smpl, mcep_alpha=DU.ALPHA, irlen=DU.E2E_IRLEN, **kw)


def _same(a, b, what):
    a, b = DU.host(a), DU.host(b)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


def run_pairs_e2e(kind, dev, layers=1, check_net=True):
    """CvgvPass (kind "cvgv") or DecodePass ("decode") with posterior="laplace" on the existing three-pair problem, as 2 + 1 pairs:
    the seven pass outputs against the fp32 oracle network within delta, the five trajectories bit for bit
    stage6.convert_pairs(posterior="laplace"), every figure against the existing restatement on the call's OWN pass outputs at
    1e-10, and the same pairs as one call of three: bit-identical per-pair results."""
    import stage6
    util, n_smpl = (SU, 3) if kind == "cvgv" else (DU, DU.E2E_SMPL)
    kw = dict(hidden_layers=layers) if layers > 1 else {}
    P, items, eps, y, stats = pair_problem(util, "lapm/%s%d" % (kind, layers), **kw)
    ty = SU.to_dev(y, dev)
    cp = _pass_for(kind, P, dev, stats, n_smpl, posterior="laplace")
    L, floor, results = P.lat_dim, 0, []
    # (ONE convert_pairs call of the three pairs: a call of one pair would take the word-exchange recurrence, where CvgvPass pads its
    # one-pair call up to the row-tile kernels so that a pair's figures do not depend on the call it lands in)
    all_items = [SU.to_dev(it, dev) for it in items]
    conv = stage6.convert_pairs(cp.enc, cp.dec, [(it[0], it[1]) for it in all_items], *ty, L, n_smpl_dec=n_smpl,
                                eps=[SU.to_dev(e, dev) for e in eps], posterior="laplace")
    for lo, hi in ((0, 2), (2, 3)):
        dev_items = [SU.to_dev(it, dev) for it in items[lo:hi]]
        dev_eps = [SU.to_dev(e, dev) for e in eps[lo:hi]]
        got = cp.pairs(dev_items, *ty, eps=dev_eps, first_pair_id=lo)
        for q, r in enumerate(got):
            own = {k: v.cpu().numpy() for k, v in cp.last_passes[q].items()}
            for k, v in zip(("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg"), conv[lo + q]):
                assert np.array_equal(own[k], v.cpu().numpy()), "pair %d %s differs from convert_pairs" % (lo + q, k)
            floor += on_floor((own["lat_src"], L), (own["lat_trg"], L))
            it, e = items[lo + q], eps[lo + q]
            if check_net:
                want = R.pair_passes(P, it[0], it[1], *y, e[0], e[1])
                delta = delta_for(want, R.pair_passes64(P, it[0], it[1], *y, e[0], e[1]), ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg"),
                                  "%s pair %d" % (kind, lo + q))
                for k in R.sref.PASS_NAMES:
                    d = float(np.max(np.abs(own[k] - want[k])))
                    print("%s pair %d %-12s max|d| vs the oracle network = %.3e" % (kind, lo + q, k, d))
                    assert own[k].shape == want[k].shape and d <= delta, (lo + q, k, d)
            if kind == "cvgv":
                fig = R.pair_metrics(own, it[2], it[3], it[4], it[5])
            else:
                fig = dref.pair_results(own, it[2], it[3], it[4], it[5], *stats, alpha=DU.ALPHA, irlen=DU.E2E_IRLEN)
            h = DU.host(r)
            assert set(h) == set(fig)
            for k, v in fig.items():
                SU.assert_close(h[k], v, 1e-10, "%s pair %d %s" % (kind, lo + q, k))
            results.append(r)
    assert floor > 0, "no log-scale on the Laplace floor"
    print("%s: %d log-scales on the floor" % (kind, floor))
    cp3 = _pass_for(kind, P, dev, stats, n_smpl, like=cp, posterior="laplace")
    got3 = cp3.pairs([SU.to_dev(it, dev) for it in items], *ty, eps=[SU.to_dev(e, dev) for e in eps])
    for q in range(3):
        _same(results[q], got3[q], "pair %d, one call of three against 2 + 1" % q)
    assert all(np.isfinite(v).all() for k, v in cp.summary().items())


def check_pairs_gauss_is_default(kind, dev):
    util, n_smpl = (SU, 3) if kind == "cvgv" else (DU, DU.E2E_SMPL)
    P, items, eps, y, stats = util.problem(tag="lapm/%sg" % kind)
    a = _pass_for(kind, P, dev, stats, n_smpl)
    b = _pass_for(kind, P, dev, stats, n_smpl, like=a, posterior="gauss")
    args = ([SU.to_dev(items[0], dev)],) + tuple(SU.to_dev(y, dev))
    ra, rb = a.pairs(*args, eps=[SU.to_dev(eps[0], dev)]), b.pairs(*args, eps=[SU.to_dev(eps[0], dev)])
    _same(ra[0], rb[0], kind)
    _same(a.last_passes[0], b.last_passes[0], kind + " passes")


# ---- 3 / 4. trainlog.TrainLog and UttLog ---------------------------------------------------------------------------------------

def _masks(P, tag, k, B, T, dev):
    masks = {"enc": [], "dec": []}
    for kind, n, cin in (("enc", 2 * P.n_cyc, P.in_dim), ("dec", 3 * P.n_cyc, P.lat_dim + 2)):
        for i in range(n):
            cm = (synth.uniform01("%s/m%d/%s%d/c" % (tag, k, kind, i), (B, T, 9 * cin)) >= 0.5).astype(np.float32) * 2.0
            gm = (synth.uniform01("%s/m%d/%s%d/g" % (tag, k, kind, i), (T, B, P.hidden)) >= 0.5).astype(np.float32) * 2.0
            masks[kind].append((t_(cm, dev), t_(gm, dev)))
    return masks


def _stand_in(P, tag, k, B, T, dev):
    """stand-in trajectories of the chain's shapes (as trainlog_util.drive's, under emulation), the latents clamped as the Laplace
    chain clamps them"""
    out = []
    for i in range(P.n_cyc):
        tr = {}
        for s in TU.SLOTS:
            lat = s in ("lat", "latcv")
            v = synth.normal("%s/trj%d/%d/%s" % (tag, k, i, s), (B, T, 2 * P.lat_dim if lat else P.out_dim)) * 0.5
            if lat:
                v[..., P.lat_dim:] = np.maximum(v[..., P.lat_dim:] * np.float32(6.0) - np.float32(3.0), FLOOR32)
            tr[s] = t_(v, dev)
        out.append(tr)
    return out


def _grab_trajs(step):
    """Stage4Step keeps last_trajs for device tensors only: under emulation the chain's trajectories are taken where the step
    forms them."""
    inner, box = step._forward_backward, []

    def forward_backward(*a):
        out = inner(*a)
        box[:] = [out[2]]
        return out
    step._forward_backward = forward_backward
    return box


def _log_problem(tag, T):
    P = lower_bias(synth.CycleVAEProblem(B=3, T=T, tag=tag, **TU.H64))
    gv = [synth.uniform(tag + "/gv_%s" % s, (P.out_dim - 1,), 0.5, 1.5).astype(np.float64) for s in ("src", "trg")]
    return P, gv


def _check_lat_par(P, enc, lat_par, feat_trg, y_pp, what):
    """the log's own encoder pass: Laplace clamp, against the fp32 oracle network within delta -- on the weights the module holds
    NOW (a real step has moved them since the problem was made)"""
    B = feat_trg.shape[0]
    y = np.repeat(y_pp[:1], B, 0)
    sd = {k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}
    want = R.orc.gru_rnn_forward(sd, feat_trg, y, clamp_vae_laplace=True, lat_dim=P.lat_dim)[0]
    enc64 = R.lref.Net64(sd, P.in_dim, 2 * P.lat_dim, P.hidden)
    w64 = enc64(R.lref.t64(feat_trg), R.lref.t64(y), None, P.lat_dim)[0].numpy()
    delta = delta_for({"lat": want}, {"lat": w64}, ("lat",), what)
    d = float(np.max(np.abs(lat_par - want)))
    print("%s: the log's encoder pass max|d| vs the oracle network = %.3e" % (what, d))
    assert d <= delta and float(lat_par[..., P.lat_dim:].min()) >= FLOOR32
    return on_floor((lat_par, P.lat_dim))


def _assert_summary(s, r):
    assert set(s) == set(r)
    for k, v in r.items():
        if k == "line":
            continue
        if np.isnan(v):
            assert np.isnan(s[k]), (k, s[k])
        else:
            assert abs(s[k] - v) <= 1e-10 * abs(v), (k, s[k], v)
    assert s["line"] == r["line"], "\n%s\n%s" % (s["line"], r["line"])


def drive_trainlog(dev, posterior="laplace", n_batches=2, real_step=None, fused=True, windows_per_batch=None, kw=None, close=True):
    """trainlog_util.drive's body (no sentinel between the batches) with a posterior: TrainLog(posterior=) around
    Stage4Step(posterior=) on the device, around stand-in trajectories under emulation unless real_step says otherwise."""
    import stage4
    import trainlog
    tag = "lapm/tl"
    laplace = posterior == "laplace"
    P, gv = _log_problem(tag, 8)
    if not laplace:
        P.enc["out_1.bias"][-1] = 0.0
    enc, dec = VU.modules(P, dev)
    enc.train()
    dec.train()
    real_step = dev.type == "cuda" if real_step is None else real_step
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-3, fused=fused, posterior=posterior) if real_step else None
    kw = {"posterior": posterior} if kw is None else kw
    tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, gv[0], gv[1], n_cyc=P.n_cyc, spk_src=TU.SPK_SRC, **kw)
    ref = (R.RefTrainLog if laplace else R.tref.RefTrainLog)(P.lat_dim, P.stdim, gv[0], gv[1], n_cyc=P.n_cyc, spk_src=TU.SPK_SRC)
    y_pp, y_dec = t_(P.y_in_enc, dev), t_(P.y_in_dec, dev)
    seq = []
    for b, batch in enumerate(TU.e2e_batches(P, tag)[:n_batches]):
        seq += list(TU.yields(batch, 8, lambda a: t_(a, dev)))[:windows_per_batch]
    if close:
        seq.append(TU.sentinel())
    box = _grab_trajs(step) if real_step else None
    out = dict(lines=[], records=[], losses=[], trajs=[], floor=0, lat_floor=0, tl=tl, ref=ref, P=P)
    carry = None
    for k, items in enumerate(seq):
        seen = tl.last_lat_srctrg
        tl.before(items, y_pp)
        lat_par = None if tl.last_lat_srctrg is None else tl.last_lat_srctrg.cpu().numpy()
        if laplace and tl.last_lat_srctrg is not seen:      # (this call closed the previous utterance batch: its encoder pass)
            out["lat_floor"] += _check_lat_par(P, enc, lat_par, TU.host_items(seq[k - 1])[3], P.y_in_enc, "TrainLog")
        ref.before(TU.host_items(items), lat_par)
        if items[9] < 0:
            out["lines"] += tl.lines()
            out["summary"], out["ref_summary"] = tl.epoch_end(), ref.epoch_end()
            break
        x, s, e = items[0], items[5], items[6]
        B, T = x.shape[0], e - s + 1
        if s == 0:
            carry = None
        if real_step:
            eps = t_((laplace_eps if laplace else synth.normal)("%s/eps%d" % (tag, k), (P.n_cyc, 3, B, T, P.lat_dim)), dev)
            loss, carry = step(x[:, s:e + 1], items[4][:, s:e + 1], items[1], items[2], y_pp, y_dec, eps, masks=_masks(P, tag, k, B, T, dev),
                               flen_acc=[int(v) for v in items[20]], select_utt_idx=list(items[19]), carry=carry, return_state=True)
            trajs = step.last_trajs or box[0]
        else:
            trajs, loss = _stand_in(P, tag, k, B, T, dev), t_(np.float32(100.0 + k), dev)
        tl.after(items, trajs, loss)
        host = [{n: v.detach().cpu().numpy() for n, v in tr.items()} for tr in trajs]
        ref.after(TU.host_items(items), host, float(loss))
        out["records"].append(tl.last_record.cpu().numpy().copy())
        out["losses"].append(float(loss))
        out["trajs"].append((host, TU.host_items(items)))
        out["floor"] += on_floor(*[(tr[n], P.lat_dim) for tr in host for n in ("lat", "latcv")])
        out["lines"] += tl.lines()
    if real_step:
        step.finish()
    out["lat_par"] = None if tl.last_lat_srctrg is None else tl.last_lat_srctrg.cpu().numpy()
    out["ref_lines"] = ref.lines
    return out


def run_trainlog_e2e(dev):
    got = drive_trainlog(dev)
    P = got["P"]
    _assert_summary(got["summary"], got["ref_summary"])
    assert len(got["lines"]) == len(got["ref_lines"]) > 0
    for a, b in zip(got["lines"], got["ref_lines"]):
        assert a == b, "\n%s\n%s" % (a, b)
    # the records' KL entries are the float64 Laplace KL of the trajectories handed in
    for rec, (host, items) in zip(got["records"], got["trajs"]):
        s, e = items[5], items[6]
        want, scale = R.window_record(host, items[0][:, s:e + 1], P.stdim, P.lat_dim, items[11], list(items[19]), items[20], items[7], items[8], s)
        m = ~np.isnan(want)
        assert np.array_equal(np.isnan(rec), ~m) and np.all(np.abs(rec[m] - want[m]) <= 1e-12 * scale[m])
    assert got["floor"] > 0 and got["lat_floor"] > 0, (got["floor"], got["lat_floor"])
    print("TrainLog: %d log-scales of the trajectories and %d of the log's encoder passes on the floor" % (got["floor"], got["lat_floor"]))
    return got


def check_window_loss_is_the_logged_sum(got, n_cyc=2):
    """The step's loss (fp32) against the logged terms (the record's float64 figures from the same trajectories): per cycle the
    selected utterances' rec, reccyc and KL(lat) figures and the lat_src_cv list as :1393 rebuilds it; 1e-5 relative."""
    for k, (rec, (host, items)) in enumerate(zip(got["records"], got["trajs"])):
        sel = list(items[19])
        want = 0.0
        for i in range(n_cyc):
            kl, klcv = [rec[i, j, 3] for j in sel], [rec[i, j, 4] for j in sel]
            want += sum(rec[i, j, 0] + rec[i, j, 1] for j in sel) + sum(kl) + (sum(klcv) if len(sel) == 1 else sum(kl) + klcv[-1])
        print("window %d: loss %.6f, sum of the logged terms %.6f" % (k, got["losses"][k], want))
        assert abs(got["losses"][k] - want) <= 1e-5 * abs(want), (k, got["losses"][k], want)


def drive_uttlog(dev, posterior="laplace", seq=UU.WHOLE, real_step=None, fused=True, kw=None):
    """uttlog_util.drive's body with a posterior."""
    import stage4
    import trainlog
    tag = "lapm/ul"
    laplace = posterior == "laplace"
    P, gv = _log_problem(tag, 8)
    if not laplace:
        P.enc["out_1.bias"][-1] = 0.0
    enc, dec = VU.modules(P, dev)
    enc.train()
    dec.train()
    real_step = dev.type == "cuda" if real_step is None else real_step
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-3, fused=fused, posterior=posterior) if real_step else None
    kw = {"posterior": posterior} if kw is None else kw
    ul = trainlog.UttLog(enc, dec, P.lat_dim, P.stdim, gv[0], gv[1], n_cyc=P.n_cyc, spk_src=TU.SPK_SRC, **kw)
    ref = (R.RefUttLog if laplace else R.uref.RefUttLog)(P.lat_dim, P.stdim, gv[0], gv[1], n_cyc=P.n_cyc, spk_src=TU.SPK_SRC)
    y_pp, y_dec = t_(P.y_in_enc, dev), t_(P.y_in_dec, dev)
    batches = TU.e2e_batches(P, tag)
    box = _grab_trajs(step) if real_step else None
    out = dict(lines=[], records=[], ref_records=[], losses=[], floor=0, lat_floor=0, P=P, ul=ul)
    for k, (b, rows) in enumerate(seq):
        items = UU.utt_yield(batches[b], k, rows, lambda a: t_(a, dev))
        B, T = items[0].shape[0], items[0].shape[1]
        ul.before(items, y_pp)
        lat_par = ul.last_lat_srctrg.cpu().numpy()
        out["lat_floor"] += _check_lat_par(P, enc, lat_par, items[3].cpu().numpy(), P.y_in_enc, "UttLog step %d" % k) if laplace else 0
        if real_step:
            eps = t_((laplace_eps if laplace else synth.normal)("%s/eps%d" % (tag, k), (P.n_cyc, 3, B, T, P.lat_dim)), dev)
            loss = step(y_in_enc=y_pp[:B], y_in_dec=y_dec[:B], eps=eps, masks=_masks(P, tag, k, B, T, dev), **stage4.utterance_step_args(items))
            trajs = step.last_trajs or box[0]
        else:
            trajs, loss = _stand_in(P, tag, k, B, T, dev), t_(np.float32(100.0 + k), dev)
        ul.after(items, trajs, loss)
        host = [{n: v.detach().cpu().numpy() for n, v in tr.items()} for tr in trajs]
        out["records"].append(ul.last_record.cpu().numpy().copy())
        out["ref_records"].append(ref.after(TU.host_items(items), host, float(loss), lat_par))
        out["losses"].append(float(loss))
        out["floor"] += on_floor(*[(tr[n], P.lat_dim) for tr in host for n in ("lat", "latcv")])
        out["lines"] += ul.lines()
    ul.before(UU.sentinel(), y_pp)
    ref.before(UU.sentinel())
    out["lines"] += ul.lines()
    out["summary"], out["ref_summary"] = ul.epoch_end(), ref.epoch_end()
    if real_step:
        step.finish()
    out["ref_lines"] = ref.lines
    return out


def run_uttlog_e2e(dev):
    got = drive_uttlog(dev)
    _assert_summary(got["summary"], got["ref_summary"])
    for a, b in zip(got["records"], got["ref_records"]):
        m = ~np.isnan(b)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), ~m) and np.all(np.abs(a[m] - b[m]) <= 1e-10 * np.abs(b[m]))
    assert len(got["lines"]) == len(got["ref_lines"]) > 0
    for a, b in zip(got["lines"], got["ref_lines"]):
        assert a == b, "\n%s\n%s" % (a, b)
    assert got["floor"] > 0 and got["lat_floor"] > 0, (got["floor"], got["lat_floor"])
    print("UttLog: %d log-scales of the trajectories and %d of the log's encoder passes on the floor" % (got["floor"], got["lat_floor"]))
    return got


def check_utt_loss_is_the_logged_sum(got):
    """test_uttlog_gpu.test_step_loss_is_the_sum_of_the_logged_terms for the Laplace step: 1e-5 relative."""
    for k, rec in enumerate(got["records"]):
        want = float(np.sum(rec[:, :, [0, 1, 3, 4]]))
        print("step %d: loss %.6f, sum of the logged terms %.6f" % (k, got["losses"][k], want))
        assert abs(got["losses"][k] - want) <= 1e-5 * abs(want), (k, got["losses"][k], want)


def check_logs_gauss_is_default(dev):
    """TrainLog and UttLog built with posterior="gauss" against the classes built without the keyword: the same records bit for bit,
    the same lines, the same encoder pass (stand-in trajectories on both backends: the step is not what differs)."""
    for drive, args in ((drive_trainlog, dict(n_batches=1)), (drive_uttlog, dict(seq=((0, None),)))):
        a = drive(dev, posterior="gauss", real_step=False, kw={}, **args)
        b = drive(dev, posterior="gauss", real_step=False, kw={"posterior": "gauss"}, **args)
        assert len(a["records"]) == len(b["records"]) > 0 and a["lines"] == b["lines"] and a["summary"]["line"] == b["summary"]["line"]
        for x, y in zip(a["records"], b["records"]):
            assert np.array_equal(x, y, equal_nan=True)
        la, lb = (g["lat_par"] if "lat_par" in g else g["ul"].last_lat_srctrg.cpu().numpy() for g in (a, b))
        assert la is not None and np.array_equal(la, lb)


def check_refusals():
    """posterior="cauchy" raises ValueError on all five classes, before anything is looked at."""
    import pytest
    import decode
    import stage5
    import trainlog
    import validation
    one = np.ones(25)
    for make in (lambda: validation.ValidationPass(None, None, 4, 4, one, one, posterior="cauchy"),
                 lambda: stage5.CvgvPass(None, None, 4, one, one, posterior="cauchy"),
                 lambda: decode.DecodePass(None, None, 4, one, one, one, one, one, posterior="cauchy"),
                 lambda: trainlog.TrainLog(None, None, 4, 4, one, one, posterior="cauchy"),
                 lambda: trainlog.UttLog(None, None, 4, 4, one, one, posterior="cauchy")):
        with pytest.raises(ValueError, match="posterior"):
            make()


# ---- 5. the device only --------------------------------------------------------------------------------------------------------

def run_validation_h1024(dev):
    """One ValidationPass(posterior="laplace").batch at H = 1024 (the recipe's dimensions) with Philox draws, B = 2, about 20 frames:
    finite figures, no log-scale below the floor, and row independence as test_validation_gpu's H = 1024 case checks it in (i) --
    the metric code on IDENTICAL trajectories, the B = 2 pass outputs and their row 0 alone, gives utterance 0 the same figures bit
    for bit.  ((ii) there repeats batch() at B = 1 with the same injected eps; Philox draws of another call are other draws.)"""
    import validation
    lens = ((((20, 18), (17, 21)), ((19, 20), (21, 16))),)
    P, batches, y, gv = VU.e2e_problem(tag="lapm/val1024", batches=lens, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05)
    lower_bias(P)
    enc, dec = (m.eval() for m in VU.modules(P, dev))
    src, trg, _ = batches[0]
    ts, tt = VU.side_to_torch(src, dev), VU.side_to_torch(trg, dev)
    vp = validation.ValidationPass(enc, dec, P.lat_dim, P.stdim, gv[0], gv[1], posterior="laplace")
    got = vp.batch(ts, tt, *(t_(v, dev) for v in y))
    assert all(np.isfinite(v) for v in got.values()), got
    assert all(np.isfinite(v) for v in vp.summary().values())
    own = {k: v.cpu().numpy() for k, v in vp.last_passes.items()}
    lats = [k for k in own if k.startswith("lat")]
    assert all(float(own[k][..., P.lat_dim:].min()) >= FLOOR32 for k in lats)
    floor = on_floor(*[(own[k], P.lat_dim) for k in lats])
    print("H1024: %d log-scales on the floor; loss %.6f" % (floor, got["loss"]))
    assert floor > 0
    both = vp.metrics(ts, tt, vp.last_passes)
    row0 = lambda d: {k: (v[:1] if hasattr(v, "shape") and getattr(v, "ndim", 0) >= 1 else v) for k, v in d.items()}
    alone = vp.metrics(row0(ts), row0(tt), {k: v[:1].contiguous() for k, v in vp.last_passes.items()})
    for k, v in both.items():
        assert np.array_equal(v[:1], alone[k]), k
    for n, t in (("loss_lat_trg", "lat_trg"), ("loss_lat_src", "lat_src")):      # and they ARE the Laplace KL of those rows
        nfr = int((trg if t == "lat_trg" else src)["flens"][0])
        ref, cond = R.kl_mean(own[t][0, :nfr], P.lat_dim)
        assert abs(float(both[n][0]) - ref) <= 1e-12 * max(abs(ref), cond), n
