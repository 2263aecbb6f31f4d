"""TEST INFRASTRUCTURE shared by tests/test_stage5_cpu.py (emulator build, numpy / CPU-tensor memory) and tests/test_stage5_gpu.py
(the device): fixtures of cvae_latent_mean, the two stage-5 statistics kinds and the end-to-end stage-5 problem, and runners that
take a `backend` (validation_util.NpBackend / TorchBackend) or a torch device so that one body serves both."""
import numpy as np

import _cabi
import synth
import validation_util as VU
import stage5_ref as sref
from oracle import cyclevae_oracle as orc

K = orc.MCD_K
TIGHT_PASS = 5e-6          # the project's pass bound: max|d| of a trajectory against the oracle network


# ---- cvae_latent_mean ----------------------------------------------------------------------------------------------------------

def latmean_inputs(tag, frames, L, n):
    """lat [frames, 2L] (means and log-variances of the size an encoder gives) and eps [n, frames, L]."""
    lat = np.concatenate([synth.normal("s5/lm/%s/mu" % tag, (frames, L)) * 0.5, synth.normal("s5/lm/%s/s" % tag, (frames, L)) * 0.5 - 1.0], 1)
    return lat.astype(np.float32), synth.normal("s5/lm/%s/eps" % tag, (n, frames, L))


def run_latent_mean(be, lats, epss, L, n, seed=0, draw_ids=None, guard=2):
    """ONE cvae_latent_mean launch over the job list.  Every job's `out` is followed by `guard` rows nobody may write (the next
    job's `out` starts right behind them); returns the list of (out [frames, L], guard rows [guard, L])."""
    rows = [l.shape[0] for l in lats]
    out = be.empty((sum(rows) + guard * len(rows), L), np.float32)      # (poisoned with -77)
    keep, jobs, at = [], [], 0
    for q, (lat, eps) in enumerate(zip(lats, epss)):
        dl = be.put(np.ascontiguousarray(lat, np.float32))
        de = None if eps is None else be.put(np.ascontiguousarray(eps, np.float32))
        keep += [dl, de]
        jobs.append(_cabi.LatMeanJob(be.ptr(dl), None if de is None else be.ptr(de), 0 if draw_ids is None else draw_ids[q], rows[q], 0,
                                     be.ptr(out) + 4 * at * L))
        at += rows[q] + guard
    be.lib.latent_mean(jobs, L, n, seed, be.stream)
    host, res, at = be.get(out), [], 0
    for r in rows:
        res.append((host[at:at + r], host[at + r:at + r + guard]))
        at += r + guard
    return res


def oracle_latent_mean(lat, eps, L):
    """calc_cvgv...:180-181 on the oracle: sampling_vae_batch over the repeated rows, then the mean over the draws."""
    return orc.sampling_vae_batch(np.repeat(lat[None], eps.shape[0], 0), eps, L).mean(0)


def check_latent_mean_injected(be, L, n, frames=(1, 7, 33), bound=2e-6):
    """Jobs of `frames` frames in one launch against the oracle at `bound`; the rows behind every job's frames keep their fill."""
    ins = [latmean_inputs("%d_%d_%d_%d" % (L, n, q, f), f, L, n) for q, f in enumerate(frames)]
    got = run_latent_mean(be, [i[0] for i in ins], [i[1] for i in ins], L, n)
    worst = 0.0
    for (out, guard), (lat, eps) in zip(got, ins):
        assert np.all(guard == -77), "rows behind a job's frames were written"
        worst = max(worst, float(np.max(np.abs(out - oracle_latent_mean(lat, eps, L)))))
    print("latent_mean L=%d n=%d jobs=%d max|d| vs the oracle = %.3e" % (L, n, len(frames), worst))
    assert worst <= bound, (L, n, worst)


def philox_draws(be, frames, L, n, seed, draw_id):
    """The draws (seed, draw_id + k, frame t, dim l) through an entry point that writes them out: cvae_sample_cat's eps_out at B = 1,
    which keys like the pass prologue keys a single-row cell (cvae_stage4.inc: (seed, draw, b * T + t, l))."""
    lat = be.put(np.zeros((frames, 2 * L), np.float32))
    code = be.put(np.zeros((frames, 2), np.float32))
    out, eo = be.empty((frames, 2 + L), np.float32), be.empty((n, frames, L), np.float32)
    for k in range(n):
        be.lib.sample_cat(be.ptr(lat), [be.ptr(code)], [None], seed, [draw_id + k], 1, frames, L, 2, be.ptr(out), be.ptr(eo) + 4 * k * frames * L,
                          be.stream)
    return be.get(eo)


def check_latent_mean_philox(be, L, n=5, frames=(1, 7, 33), seed=0x1234567890ABC, draw_ids=(0, 600, 900)):
    """Philox and injected draws agree bit for bit."""
    lats = [latmean_inputs("px%d_%d" % (L, q), f, L, 1)[0] for q, f in enumerate(frames)]
    eps = [philox_draws(be, f, L, n, seed, d) for f, d in zip(frames, draw_ids)]
    for e in eps:
        assert np.all(e != -77) and 0.5 < float(np.std(e)) < 1.5        # (every draw written, and they are draws)
    a = run_latent_mean(be, lats, [None] * len(lats), L, n, seed=seed, draw_ids=draw_ids)
    b = run_latent_mean(be, lats, eps, L, n)
    for (x, gx), (y, _) in zip(a, b):
        assert np.all(gx == -77)
        assert np.array_equal(x, y), "Philox and injected draws differ (L=%d)" % L
    # another seed or another draw id gives other values
    c = run_latent_mean(be, lats, [None] * len(lats), L, n, seed=seed + 1, draw_ids=draw_ids)
    assert not np.array_equal(a[-1][0], c[-1][0])


# ---- the two statistics kinds --------------------------------------------------------------------------------------------------

def stat_cases():
    """validation_util.stat_cases() (the existing kinds) plus the stage-5 kinds, for ONE launch: rows 1 (std 0), 2 and 1000, a
    column window with c0 = 1, operands wider than the window, rows beyond src_rows."""
    arrays, cases = VU.stat_cases()
    v = synth.normal("s5/st/v", (1000, 1)).astype(np.float64) * 3.0 + 7.0
    a = synth.normal("s5/st/a", (1000, 7)).astype(np.float64)
    b = (synth.normal("s5/st/b", (1000, 9)) * 0.9 + 0.05).astype(np.float64)
    arrays = dict(arrays, s5v=v, s5a=a, s5b=b)
    ms = lambda x: np.array([np.mean(x), np.std(x)])
    mcd = lambda rows, c0, c1: ms(K * np.sqrt(2.0 * np.sum((a[:rows, c0:c1] - b[:rows, c0:c1]) ** 2, 1)))
    J = lambda rows, **kw: dict(kind=_cabi.STAT_MEANSTD64, rows=rows, c0=0, c1=1, a=("s5v", 0), src_rows=rows, **kw)
    M = lambda rows, c0, c1, src_rows: dict(kind=_cabi.STAT_MCD64, rows=rows, c0=c0, c1=c1, a=("s5a", 0), b=("s5b", 0), src_rows=src_rows)
    new = [("meanstd rows=1", J(1), np.array([v[0, 0], 0.0])),
           ("meanstd rows=2", J(2), ms(v[:2, 0])),
           ("meanstd rows=1000", J(1000), ms(v[:, 0])),
           ("mcd64 rows=1000", M(1000, 0, 7, 1000), mcd(1000, 0, 7)),
           ("mcd64 rows=1000 c0=1", M(1000, 1, 7, 1000), mcd(1000, 1, 7)),
           ("mcd64 rows=2 c0=1", M(2, 1, 7, 1000), mcd(2, 1, 7)),
           ("mcd64 rows=1 c0=1", M(1, 1, 7, 1), np.array([mcd(1, 1, 7)[0], 0.0])),
           ("mcd64 is oracle.mcd_aligned", M(33, 1, 7, 33), np.array(orc.mcd_aligned(a[:33, :7], b[:33, :7], d0=1)[1:])),
           ("meanstd rows beyond the vector", dict(J(5), src_rows=4), np.array([np.nan, np.nan])),
           ("mcd64 rows beyond the operands", M(5, 0, 7, 4), np.array([np.nan, np.nan]))]
    return arrays, cases[:6] + new + cases[6:]


# ---- the end-to-end problem ----------------------------------------------------------------------------------------------------

E2E_LENS = ((24, 30), (27, 20), (22, 45))          # (source, target) frames of the three pairs: ragged, 20..45


def problem(tag="s5", lens=E2E_LENS, n_smpl=3, **dims):
    """The synthetic stage-5 set: weights, per pair (feat_src, feat_trg, spcidx_src, spcidx_trg, mcepspc_src, mcepspc_trg) and
    (eps_src, eps_trg), the y_in vectors, the speakers' GV statistics.  Speech frames: a non-contiguous increasing subset of each
    utterance; mcepspc: the utterance's own spectral features at those frames plus analysis noise, in float64."""
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
            mc = feat[keep, sd:].astype(np.float64) + 0.1 * synth.normal("%s/p%d/%s/mc" % (tag, k, side), (len(keep), P.out_dim)).astype(np.float64)
            it.append((feat, keep.astype(np.int64), mc))
        items.append((it[0][0], it[1][0], it[0][1], it[1][1], it[0][2], it[1][2]))
        eps.append((synth.normal("%s/p%d/eps_src" % (tag, k), (n_smpl, ts, P.lat_dim)), synth.normal("%s/p%d/eps_trg" % (tag, k), (n_smpl, tt, P.lat_dim))))
    y_pp, y_trg = P.y_in_enc[:1], P.y_in_dec[:1]
    y_src = (0.5 * P.y_in_dec[:1]).astype(np.float32)          # (the script passes one vector for both; two catch a swap)
    gv_src = synth.uniform(tag + "/gv_src", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    gv_trg = synth.uniform(tag + "/gv_trg", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    return P, items, eps, (y_pp, y_src, y_trg), (gv_src, gv_trg)


def to_dev(arrs, dev):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs)


def make_pass(P, dev, gv, n_smpl, like=None):
    """like: another CvgvPass whose modules (and prepared weight images) this one shares."""
    import stage5
    enc, dec = (like.enc, like.dec) if like is not None else (m.eval() for m in VU.modules(P, dev))
    return stage5.CvgvPass(enc, dec, P.lat_dim, gv[0], gv[1], n_smpl_dec=n_smpl)


def assert_close(got, want, rel, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.max(np.abs(want))), 1e-300)
    assert got.shape == want.shape and float(np.max(np.abs(got - want))) <= rel * scale, (what, got, want)


def same_figures(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k, a[k], b[k])


_ORACLE = {}


def oracle_passes():
    """The oracle network on the three pairs of problem(): computed once, shared, never changed."""
    if "o" not in _ORACLE:
        P, items, eps, (y_pp, y_src, y_trg), _ = problem()
        _ORACLE["o"] = [sref.network_passes(P.enc, P.dec, it[0], it[1], y_pp, y_src, y_trg, e[0], e[1], P.lat_dim) for it, e in zip(items, eps)]
    return _ORACLE["o"]


def run_e2e(dev):
    """Three pairs as a call of two and a call of one (H = 64, n_smpl_dec = 3, eps injected).  Network-derived outputs against the
    oracle network at TIGHT_PASS; metric-derived quantities against stage5_ref run on the library's OWN trajectories at 1e-10
    relative; then the same pairs as one call of three: the same per-pair figures bit for bit."""
    P, items, eps, y, gv = problem()
    ty = to_dev(y, dev)
    cp = make_pass(P, dev, gv, 3)
    ref = sref.RefCvgv(*gv)
    want_net = oracle_passes()
    figures = []
    for lo, hi in ((0, 2), (2, 3)):
        got = cp.pairs([to_dev(it, dev) for it in items[lo:hi]], *ty, eps=[to_dev(e, dev) for e in eps[lo:hi]], first_pair_id=lo)
        assert len(got) == hi - lo and len(cp.last_passes) == hi - lo
        for q, r in enumerate(got):
            own = {k: v.cpu().numpy() for k, v in cp.last_passes[q].items()}
            assert set(own) == set(sref.PASS_NAMES)
            for k in sref.PASS_NAMES:
                d = float(np.max(np.abs(own[k] - want_net[lo + q][k])))
                print("e2e pair %d %-12s max|d| vs the oracle network = %.3e" % (lo + q, k, d))
                assert own[k].shape == want_net[lo + q][k].shape and d <= TIGHT_PASS, (lo + q, k, d)
            it = items[lo + q]
            want = sref.pair_metrics(own, it[2], it[3], it[4], it[5])
            ref.add(want)
            assert set(r) == set(want)
            for k, v in want.items():
                assert_close(r[k], v, 1e-10, "pair %d %s" % (lo + q, k))
            figures.append(r)
    s, s_ref = cp.summary(), ref.summary()
    assert set(s) == set(s_ref)
    for k, v in s_ref.items():
        assert_close(s[k], v, 1e-10, k)
    lines = cp.log_lines()
    assert len(lines) == 13 and lines[0].startswith("mcdpow: %.6f dB (+- " % s["mcdpow_mean"]) and lines[-1].startswith("lat_dist_cosim_pri: ")
    # grouping
    cp3 = make_pass(P, dev, gv, 3, like=cp)
    got3 = cp3.pairs([to_dev(it, dev) for it in items], *ty, eps=[to_dev(e, dev) for e in eps])
    for q in range(3):
        same_figures(figures[q], got3[q], "pair %d, one call of three against 2 + 1" % q)
    return cp, figures


def run_closing_the_loop(dev):
    """One pair: with cvgv_mean taken from that same utterance, the post-filtered trajectory has the target speaker's GV."""
    import stage6
    P, items, eps, y, gv = problem()
    cp = make_pass(P, dev, gv, 3)
    cp.pairs([to_dev(items[0], dev)], *to_dev(y, dev), eps=[to_dev(eps[0], dev)])
    out, var = stage6.gv_postfilter(cp.last_passes[0]["cvmcep"], gv[1], cp.summary()["cvgv_mean"])
    assert_close(np.var(out.cpu().numpy()[:, 1:], axis=0), gv[1], 1e-10, "GV after the post-filter")
    assert_close(var.cpu().numpy(), gv[1], 1e-10, "cvae_gv_postfilter's own variance")


class CallCounter(object):
    """Counts the calls of the bound library's methods (monkeypatch restores them)."""

    def __init__(self, monkeypatch, lib, names=("latent_mean", "eval_stats", "dtw_batch")):
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(lib, k, self._wrap(k, getattr(lib, k)), raising=True)

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return counted

    def take(self):
        out, self.n = dict(self.n), {k: 0 for k in self.n}
        return out


def run_launch_count(dev, monkeypatch):
    """A one-pair call and a ten-pair call both make one latent_mean, two eval_stats and one dtw_batch."""
    import gru_vae
    lens = tuple((8 + k % 3, 9 + k % 2) for k in range(10))
    P, items, eps, y, gv = problem(tag="s5/count", lens=lens, n_smpl=2)
    cp = make_pass(P, dev, gv, 2)
    ty = to_dev(y, dev)
    cp.pairs([to_dev(items[0], dev)], *ty, eps=[to_dev(eps[0], dev)])       # (binds the library, prepares the images)
    count = CallCounter(monkeypatch, gru_vae._lib())
    for N in (1, 10):
        res = cp.pairs([to_dev(it, dev) for it in items[:N]], *ty, eps=[to_dev(e, dev) for e in eps[:N]])
        assert len(res) == N
        assert count.take() == {"latent_mean": 1, "eval_stats": 2, "dtw_batch": 1}, N


def run_bad_spcidx(dev):
    """An spcidx entry >= frames: NaN figures for that pair only (those that read through the index lists), others unchanged."""
    import stage5
    P, items, eps, y, gv = problem(tag="s5/bad", lens=((9, 11), (12, 8)))
    ty = to_dev(y, dev)
    cp = make_pass(P, dev, gv, 3)
    clean = cp.pairs([to_dev(it, dev) for it in items[:2]], *ty, eps=[to_dev(e, dev) for e in eps[:2]])
    bad = list(items[1])
    bad[2] = bad[2].copy()
    bad[2][-1] = items[1][0].shape[0]             # one past the source utterance's last frame
    got = cp.pairs([to_dev(items[0], dev), to_dev(bad, dev)], *ty, eps=[to_dev(e, dev) for e in eps[:2]])
    same_figures(clean[0], got[0], "the pair beside the bad one")
    for k in stage5.MCD_TERMS + stage5.DIST_TERMS:
        assert np.isnan(got[1][k]), k
    for k in stage5.GV_TERMS:
        assert np.array_equal(got[1][k], clean[1][k]), k


def run_files_and_write(dev, tmp_path):
    """write(): the six datasets read back equal to summary(); run_files on three small files equals pairs on the same arrays."""
    import hdf5io
    import stage5
    P, items, eps, y, gv = problem(tag="s5/files", lens=((9, 11), (12, 8), (10, 10)), n_smpl=2)
    ty = to_dev(y, dev)
    files = []
    for k, it in enumerate(items):
        pair = []
        for side, (feat, spc, mc) in (("src", (it[0], it[2], it[4])), ("trg", (it[1], it[3], it[5]))):
            path = str(tmp_path / ("%s%d.h5" % (side, k)))
            hdf5io.write_hdf5(path, "/feat_org_lf0", feat)
            hdf5io.write_hdf5(path, "/spcidx_range", spc[None, :])
            hdf5io.write_hdf5(path, "/mcepspc_range", mc)
            pair.append(path)
        files.append(tuple(pair))
    a = make_pass(P, dev, gv, 2)
    got = stage5.run_files(a, files, *ty, per_call=2, seed=77)
    b = make_pass(P, dev, gv, 2, like=a)
    want = b.pairs([to_dev(it, dev) for it in items[:2]], *ty, seed=77) + b.pairs([to_dev(items[2], dev)], *ty, seed=77, first_pair_id=2)
    assert len(got) == 3
    for q in range(3):
        same_figures(got[q], want[q], "run_files pair %d" % q)
    stats = str(tmp_path / "stats_src.h5")
    hdf5io.write_hdf5(stats, "/gv_range_mean", np.arange(P.out_dim, dtype=np.float64))      # (the file's other datasets stay)
    sfx = stage5.dataset_suffix("gru_cyclevae", 2, P.lat_dim, 1234, "TF1", 2)
    assert sfx == "gru_cyclevae-2-%d-1234-TF1-2" % P.lat_dim
    a.write(stats, sfx)
    s = a.summary()
    for g in ("cvgv", "cvgvsrc", "cvgvtrg"):
        for kind in ("mean", "var"):
            back = hdf5io.read_hdf5(stats, "/%s_%s_%s" % (g, kind, sfx))
            assert back.dtype == np.float64 and np.array_equal(back, s["%s_%s" % (g, kind)])
    assert np.array_equal(hdf5io.read_hdf5(stats, "/gv_range_mean"), np.arange(P.out_dim, dtype=np.float64))
