"""TEST INFRASTRUCTURE shared by tests/test_validation_cpu.py (emulator build, numpy memory) and tests/test_validation_gpu.py (the
device): fixtures of the batched DTW, the statistics jobs and the end-to-end validation problem, and runners that take a
`backend` so that one body serves both."""
import numpy as np

import _cabi
import synth
from oracle import cyclevae_oracle as orc
import validation_ref as vref

K = orc.MCD_K


class NpBackend(object):
    """ "Device" memory is numpy memory (the emulator build)."""

    def __init__(self, lib):
        self.lib, self.stream = lib, 0

    def put(self, a):
        return np.ascontiguousarray(a)

    def empty(self, shape, dtype):
        return np.full(shape, 0 if np.dtype(dtype) == np.uint8 else -77, dtype)      # (poisoned: an output nobody wrote shows)

    def ptr(self, a):
        return a.ctypes.data

    def get(self, a):
        return np.array(a)


class TorchBackend(object):
    def __init__(self, lib, device):
        import torch
        self.torch, self.lib, self.dev = torch, lib, device
        self.stream = torch.cuda.current_stream().cuda_stream

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def empty(self, shape, dtype):
        return self.put(np.full(shape, 0 if np.dtype(dtype) == np.uint8 else -77, dtype))

    def ptr(self, a):
        return a.data_ptr()

    def get(self, a):
        return a.cpu().numpy()


# ---- batched DTW ---------------------------------------------------------------------------------------------------------------

def dtw_problem(T1, T2, D, mcd, tag):
    a = synth.normal("val/dtw/%s/a" % tag, (T1, D)).astype(np.float64)
    b = (synth.normal("val/dtw/%s/b" % tag, (T2, D)) * 0.8 + 0.1).astype(np.float64)
    return a, b, mcd


def mixed_problems():
    """Every (T1, T2) x D x cost kind of the mixed-shape case, in one list."""
    out = []
    for T1, T2 in ((1, 1), (1, 7), (7, 1), (12, 12), (33, 20), (20, 33)):
        for D in (4, 26):
            for mcd in (-1, 0):
                out.append(dtw_problem(T1, T2, D, mcd, "%d_%d_%d_%d" % (T1, T2, D, mcd)))
    return out


def tie_problem():
    """Small-integer frames with repeated rows: every squared difference and every sum of them is an exact integer in any
    summation order, so the local cost K sqrt(2 s) is one function of s -- equal s give equal costs bit for bit -- and repeated
    rows make whole rows and columns of the cost matrix equal.  Accumulated costs then tie exactly (oracle_ties finds all three
    kinds on the oracle's path), and several org frames of a target frame share the smallest local cost ("<=" walking backwards)."""
    a = np.array([[0, 0], [0, 0], [1, 0], [1, 0], [1, 0], [2, 1], [2, 1], [0, 0], [3, 1]], np.float64)
    b = np.array([[0, 0], [1, 0], [1, 0], [2, 1], [2, 1], [2, 1], [0, 0], [0, 0], [3, 1], [3, 1]], np.float64)
    return a, b, -1


def oracle_ties(org, trg, mcd=-1):
    """The kinds of exact ties the ORACLE's path passes through: at a path cell, the chosen predecessor's accumulated cost equals
    another candidate's.  Returns a set of "diag=up", "diag=left", "up=left" (equalities among the candidates at the minimum)."""
    a, b = np.asarray(org, np.float64), np.asarray(trg, np.float64)
    T1, T2 = a.shape[0], b.shape[0]
    d = a[:, None, :] - b[None, :, :]
    cost = K * np.sqrt(2.0 * np.sum(d * d, 2))
    acc = np.full((T1, T2), np.inf)
    for i in range(T1):
        for j in range(T2):
            prev = [acc[i - 1, j - 1] if i and j else np.inf, acc[i - 1, j] if i else np.inf, acc[i, j - 1] if j else np.inf]
            acc[i, j] = cost[i, j] + (0.0 if i == 0 and j == 0 else min(prev))
    kinds = set()
    i, j = T1 - 1, T2 - 1
    while i or j:
        c = [acc[i - 1, j - 1] if i and j else np.inf, acc[i - 1, j] if i else np.inf, acc[i, j - 1] if j else np.inf]
        m = min(c)
        if c[0] == m and c[1] == m:
            kinds.add("diag=up")
        if c[0] == m and c[2] == m:
            kinds.add("diag=left")
        if c[1] == m and c[2] == m:
            kinds.add("up=left")
        k = c.index(m)          # diagonal, then (i-1, j), then (i, j-1)
        i, j = (i - 1, j - 1) if k == 0 else ((i - 1, j) if k == 1 else (i, j - 1))
    return kinds


def run_dtw_batch(be, problems, want_aligned=True):
    """cvae_dtw_batch over [(org, trg, mcd)]: list of (aligned, twf, mean, frames) numpy."""
    keep, probs = [], []
    for a, b, mcd in problems:
        da, db = be.put(a), be.put(b)
        T1, T2, D = a.shape[0], b.shape[0], a.shape[1]
        o = (be.empty((T2, D), np.float64), be.empty((T2,), np.int64), be.empty((T2,), np.float64), be.empty((1,), np.float64))
        keep.append((da, db) + o)
        probs.append(_cabi.DtwProblem(be.ptr(da), be.ptr(db), D, D, T1, T2, D, mcd, be.ptr(o[0]) if want_aligned else None, be.ptr(o[1]),
                                      be.ptr(o[2]), be.ptr(o[3])))
    nb = be.lib.dtw_batch_work_bytes(len(probs), max(p.T1 for p in probs), max(p.T2 for p in probs))
    assert nb > 0
    work = be.empty((nb,), np.uint8)
    be.lib.dtw_batch(probs, be.ptr(work), nb, be.stream)
    return [(be.get(k[2]), be.get(k[3]), float(be.get(k[5])[0]), be.get(k[4])) for k in keep]


def run_dtw_single(be, a, b, mcd):
    """cvae_dtw_org_to_trg (the existing one-problem entry point)."""
    da, db = be.put(a), be.put(b)
    T1, T2, D = a.shape[0], b.shape[0], a.shape[1]
    al, twf, fr, mean = be.empty((T2, D), np.float64), be.empty((T2,), np.int64), be.empty((T2,), np.float64), be.empty((1,), np.float64)
    nb = be.lib.dtw_work_bytes(T1, T2)
    work = be.empty((nb,), np.uint8)
    be.lib.dtw_org_to_trg(be.ptr(da), be.ptr(db), T1, T2, D, mcd, be.ptr(al), be.ptr(twf), be.ptr(fr), be.ptr(mean), be.ptr(work), nb, be.stream)
    return be.get(al), be.get(twf), float(be.get(mean)[0]), be.get(fr)


def assert_bit_identical(batched, single, what):
    for name, x, y in zip(("aligned", "twf", "mean", "frames"), batched, single):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "%s: %s differs from cvae_dtw_org_to_trg" % (what, name)


def assert_matches_oracle(res, a, b, mcd, what):
    al, twf, mean, fr = orc.dtw_org_to_trg(a, b, mcd=mcd)
    assert np.array_equal(res[1], twf), "%s: twf differs from the oracle's" % what
    scale = max(1e-300, float(np.max(np.abs(fr))))
    assert np.max(np.abs(res[3] - fr)) <= 1e-12 * scale, what
    assert abs(res[2] - mean) <= 1e-12 * max(abs(mean), scale), what
    assert np.array_equal(res[0], al), what


# ---- statistics jobs -----------------------------------------------------------------------------------------------------------

def stat_cases():
    """(name, kind, job fields, numpy f64 reference) over one set of arrays: flen < T, n_spc = 1, d0 0 and 1, a non-contiguous
    index list, strided operands (a column window of a wider matrix)."""
    T, Cin, sd, Co, L = 23, 9, 2, 7, 3
    feat = synth.normal("val/st/feat", (T, Cin))
    trj = synth.normal("val/st/trj", (T, Co)) * 0.7
    lat = synth.normal("val/st/lat", (T, 2 * L)) * 0.5
    idx = np.array([0, 2, 3, 7, 8, 15, 21, 22], np.int64)
    one = np.array([11], np.int64)
    al = synth.normal("val/st/al", (8, 2 * L)).astype(np.float64)
    tg = synth.normal("val/st/tg", (8, 2 * L)).astype(np.float64)
    f64 = lambda a: np.asarray(a, np.float64)
    mcd = lambda a, b: float(np.mean(K * np.sqrt(2.0 * np.sum((f64(a) - f64(b)) ** 2, 1))))
    arrays = {"feat": feat, "trj": trj, "lat": lat, "idx": idx, "one": one, "al": al, "tg": tg}
    flen = 17
    kl = lambda p: float(np.mean(0.5 * np.sum(np.exp(f64(p[:, L:])) + f64(p[:, :L]) ** 2 - f64(p[:, L:]) - 1.0, 1)))
    cases = [
        ("gv flen<T", dict(kind=_cabi.STAT_GV, rows=flen, c0=1, c1=Co, a=("trj", 0)), np.var(f64(trj[:flen, 1:]), axis=0)),
        ("gv whole", dict(kind=_cabi.STAT_GV, rows=T, c0=1, c1=Co, a=("trj", 0)), np.var(f64(trj[:, 1:]), axis=0)),
        ("gv one frame", dict(kind=_cabi.STAT_GV, rows=1, c0=1, c1=Co, a=("trj", 0)), np.zeros(Co - 1)),
        ("mcdpow spc", dict(kind=_cabi.STAT_MCD_SPC, rows=len(idx), c0=0, c1=Co, a=("feat", sd), b=("trj", 0), idx="idx", src_rows=T),
         mcd(feat[idx][:, sd:], trj[idx])),
        ("mcd spc d0=1", dict(kind=_cabi.STAT_MCD_SPC, rows=len(idx), c0=1, c1=Co, a=("feat", sd), b=("trj", 0), idx="idx", src_rows=T),
         mcd(feat[idx][:, sd + 1:], trj[idx][:, 1:])),
        ("mcd spc n_spc=1", dict(kind=_cabi.STAT_MCD_SPC, rows=1, c0=1, c1=Co, a=("feat", sd), b=("trj", 0), idx="one", src_rows=T),
         mcd(feat[one][:, sd + 1:], trj[one][:, 1:])),
        ("mcd l1", dict(kind=_cabi.STAT_MCD_L1, rows=flen, c0=0, c1=Co, a=("trj", 0), b=("feat", sd)),
         float(np.mean(K * np.sqrt(2.0) * np.sum(np.abs(f64(trj[:flen]) - f64(feat[:flen, sd:])), 1)))),
        ("kl", dict(kind=_cabi.STAT_KL, rows=flen, c0=0, c1=L, a=("lat", 0)), kl(lat[:flen])),
        ("kl one frame", dict(kind=_cabi.STAT_KL, rows=1, c0=0, c1=L, a=("lat", 0)), kl(lat[:1])),
        ("gather64", dict(kind=_cabi.STAT_GATHER64, rows=len(idx), c0=0, c1=Co, a=("feat", sd), idx="idx", src_rows=T, dst=(len(idx), Co)),
         f64(feat[idx][:, sd:])),
        ("gather64 columns 1..", dict(kind=_cabi.STAT_GATHER64, rows=1, c0=1, c1=Co, a=("trj", 0), idx="one", src_rows=T, dst=(1, Co - 1)),
         f64(trj[one][:, 1:])),
        ("latdist", dict(kind=_cabi.STAT_LATDIST, rows=8, c0=0, c1=2 * L, a=("al", 0), b=("tg", 0)),
         float(np.mean(np.sqrt(np.mean((al - tg) ** 2, axis=0))))),
        ("mcd spc index out of range", dict(kind=_cabi.STAT_MCD_SPC, rows=len(idx), c0=0, c1=Co, a=("feat", sd), b=("trj", 0), idx="idx",
                                              src_rows=20), float("nan")),
    ]
    return arrays, cases


def run_stats(be, arrays, cases):
    """All cases as ONE cvae_eval_stats launch.  Returns the list of results (arrays) in case order."""
    dev = {k: be.put(v) for k, v in arrays.items()}
    item = {k: v.dtype.itemsize for k, v in arrays.items()}

    def at(spec):
        name, col = spec
        return be.ptr(dev[name]) + col * item[name], arrays[name].shape[1]
    jobs, outs, off = [], [], 0
    for _, f, ref in cases:
        a, lda = at(f["a"])
        b, ldb = at(f["b"]) if "b" in f else (None, 0)
        dst = None
        if "dst" in f:
            dst = be.empty(f["dst"], np.float64)
            outs.append(("dst", dst))
        else:
            n = int(np.size(ref))
            outs.append(("out", off, n))
        jobs.append(_cabi.StatJob(f["kind"], f["rows"], f["c0"], f["c1"], f.get("src_rows", 0), 0, a, b, lda, ldb,
                                  be.ptr(dev[f["idx"]]) if "idx" in f else None, None if dst is None else be.ptr(dst), off))
        off += 0 if "dst" in f else int(np.size(ref))
    out = be.empty((off,), np.float64)
    raw = np.frombuffer(bytes((_cabi.StatJob * len(jobs))(*jobs)), np.uint8)
    jd = be.put(raw)
    be.lib.eval_stats(be.ptr(jd), len(jobs), be.ptr(out), be.stream)
    host = be.get(out)
    return [be.get(o[1]) if o[0] == "dst" else host[o[1]:o[1] + o[2]] for o in outs]


def assert_stats(results, cases):
    for (name, _, ref), got in zip(cases, results):
        ref = np.asarray(ref, np.float64)
        got = np.asarray(got, np.float64).reshape(ref.shape)
        if np.all(np.isnan(ref)):
            assert np.all(np.isnan(got)), name
            continue
        scale = max(float(np.max(np.abs(ref))), 1e-300)
        err = float(np.max(np.abs(got - ref)))
        print("stats %-28s max|d| / scale = %.3e" % (name, err / scale))
        assert err <= 1e-12 * scale, (name, err, scale)


# ---- the end-to-end problem ----------------------------------------------------------------------------------------------------

H64 = dict(in_dim=30, out_dim=26, lat_dim=4, hidden=64, n_cyc=1, bias_scale=0.1)          # (the dimensions of frontend_util.H64)
DRAWS = ("trg_trg", "trg_src", "src_src", "src_trg", "trg_src_trg", "src_trg_src")
# (own, parallel) lengths per utterance: ragged, 20..45 frames, counterpart lengths differ; two batches (2 + 1)
E2E_BATCHES = ((((24, 21), (30, 26)), ((27, 30), (20, 23))),
               (((22, 20),), ((45, 25),)))


def make_side(P, tag, lens, other_first):
    """One evaluation generator's yield for utterances of (own, parallel) lengths `lens`, zero-padded like the loader pads."""
    B = len(lens)
    T, Tp = max(l[0] for l in lens), max(l[1] for l in lens)
    sd = P.stdim
    feat = synth.features(tag + "/feat", B, T, P.mu, P.sigma)
    par = synth.features(tag + "/par", B, Tp, P.mu, P.sigma)
    cv = synth.features(tag + "/cv", B, T, P.mu[:sd], P.sigma[:sd])
    own, other = synth.onehot_codes(B, T, src_is_first=not other_first)
    S, Sp = T, Tp
    spc, spc_par = np.zeros((B, S), np.int64), np.zeros((B, Sp), np.int64)
    ns, nsp = [], []
    for j, (n, m) in enumerate(lens):
        for a in (feat, cv, own, other):
            a[j, n:] = 0
        par[j, m:] = 0
        # speech frames: a non-contiguous, increasing subset
        keep = np.nonzero(synth.uniform01("%s/spc%d" % (tag, j), (n,)) < 0.7)[0]
        keep_p = np.nonzero(synth.uniform01("%s/spcp%d" % (tag, j), (m,)) < 0.7)[0]
        keep = keep if len(keep) > 1 else np.arange(2)
        keep_p = keep_p if len(keep_p) > 1 else np.arange(2)
        spc[j, :len(keep)], spc_par[j, :len(keep_p)] = keep, keep_p
        ns.append(len(keep))
        nsp.append(len(keep_p))
    return {"feat": feat, "code_own": own, "code_other": other, "feat_par": par, "cv": cv, "spcidx": spc, "spcidx_par": spc_par,
            "flens": np.array([l[0] for l in lens]), "flens_par": np.array([l[1] for l in lens]), "flens_spc": np.array(ns),
            "flens_spc_par": np.array(nsp), "n_utt": B}


def e2e_problem(tag="val", batches=E2E_BATCHES, **dims):
    """The synthetic validation set: weights, per batch (src side, trg side, eps), y_in vectors, GV statistics."""
    d = dict(H64)
    d.update(dims)
    P = synth.CycleVAEProblem(B=1, T=4, tag=tag, **d)
    out = []
    for k, (ls, lt) in enumerate(batches):
        src, trg = make_side(P, "%s/b%d/src" % (tag, k), ls, False), make_side(P, "%s/b%d/trg" % (tag, k), lt, True)
        eps = {}
        for n in DRAWS:
            T = (trg if n.startswith("trg") else src)["feat"].shape[1]
            eps[n] = synth.normal("%s/b%d/eps/%s" % (tag, k, n), (len(ls), T, P.lat_dim))
        out.append((src, trg, eps))
    y_pp = P.y_in_enc[:1]
    y_trg = P.y_in_dec[:1]
    y_src = (0.5 * P.y_in_dec[:1]).astype(np.float32)
    gv_src = synth.uniform(tag + "/gv_src", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    gv_trg = synth.uniform(tag + "/gv_trg", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    return P, out, (y_pp, y_src, y_trg), (gv_src, gv_trg)


def side_to_torch(side, dev):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) and k not in (
        "flens", "flens_par", "flens_spc", "flens_spc_par") else v) for k, v in side.items()}


def as_generator_yield(side):
    """The 16-field tuple of loader.train_generator(batch_size=0)."""
    return (side["feat"], side["code_own"], side["code_other"], side["feat_par"], side["cv"], 0, 0, side["spcidx"], side["spcidx_par"],
            [], [], side["flens"], side["flens_par"], side["flens_spc"], side["flens_spc_par"], side["n_utt"])


def modules(P, dev):
    import torch
    import gru_vae

    def mod(sd, i, o, enc):
        m = gru_vae.GRU_RNN(in_dim=i, out_dim=o, hidden_units=P.hidden, kernel_size=P.kernel_size, dilation_size=P.dilation_size,
                            hidden_layers=P.hidden_layers, scale_in_flag=enc, scale_out_flag=not enc)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(dev)
    return mod(P.enc, P.in_dim, 2 * P.lat_dim, True), mod(P.dec, P.lat_dim + 2, P.out_dim, False)


def loss_bounds(o, src, trg, lat_dim, stdim, delta):
    """|difference| allowed on the per-batch loss terms when every trajectory is within `delta` (max-abs) of the reference's:
         loss_mcd_*: mean_t K sqrt2 sum_d |x - y|  moves by at most K sqrt2 D delta           (triangle inequality, D = out_dim)
         loss_lat_*: mean_t 0.5 sum_l (exp(s) + mu^2 - s - 1)  moves by at most 0.5 L delta (exp(s_max + delta) + 2 |mu|_max + delta + 1)
       per utterance, hence per batch mean; the batch loss is the sum of its terms' bounds.  Everything also carries fp32 rounding
       of the reference's own sums (relative 1e-6 of the value, added by the caller)."""
    D, L = o["trj_trg_trg"].shape[2], lat_dim
    b = {}
    for n in ("trg_trg", "trg_src_trg", "trg_src", "src_src", "src_trg_src", "src_trg"):
        b["loss_mcd_" + n] = K * np.sqrt(2.0) * D * delta
    for n, t in (("loss_lat_trg", "lat_trg"), ("loss_lat_src", "lat_src"), ("loss_lat_trg_cv", "lat_trg_src"), ("loss_lat_src_cv", "lat_src_trg")):
        mu, s = np.abs(o[t][..., :L]).max(), o[t][..., L:].max()
        b[n] = 0.5 * L * delta * (np.exp(s + delta) + 2.0 * mu + delta + 1.0)
    return b


def run_e2e(dev, delta):
    """ValidationPass over the synthetic validation set (3 utterance pairs as 2 + 1, ragged 20-45 frames, counterparts of other
    lengths, eps injected) against the restatement.  See test_validation_pass_end_to_end for the bounds."""
    import torch
    import validation
    P, batches, (y_pp, y_src, y_trg), (gv_src, gv_trg) = e2e_problem()
    enc, dec = modules(P, dev)
    enc.train()
    dec.eval()
    for p in dec.parameters():
        p.requires_grad = False
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vp = validation.ValidationPass(enc, dec, P.lat_dim, P.stdim, gv_src, gv_trg)
    net = vref.RefValidation(P.enc, P.dec, P.lat_dim, P.stdim, gv_src, gv_trg)       # the oracle network
    met = vref.RefValidation(P.enc, P.dec, P.lat_dim, P.stdim, gv_src, gv_trg)       # the metric half on the library's own pass outputs
    for src, trg, eps in batches:
        B = src["feat"].shape[0]
        ts, tt = side_to_torch(src, dev), side_to_torch(trg, dev)
        te = {k: t(v) for k, v in eps.items()}
        got = vp.batch(as_generator_yield(ts), as_generator_yield(tt), t(y_pp), t(y_src), t(y_trg), eps=te)
        assert enc.training and not dec.training
        assert all(p.requires_grad for p in enc.parameters()) and not any(p.requires_grad for p in dec.parameters())
        rep = lambda y: np.repeat(y, B, 0)
        want_net, o_ref = net.batch(src, trg, rep(y_pp), rep(y_src), rep(y_trg), eps=eps)
        own = {k: v.cpu().numpy() for k, v in vp.last_passes.items()}
        worst = max(float(np.max(np.abs(own[k] - o_ref[k]))) for k in vref.PASS_NAMES)
        print("e2e B=%d pass outputs max|d| vs the oracle network = %.3e" % (B, worst))
        want_met, _ = met.batch(src, trg, None, None, None, trajectories=own)
        bound = loss_bounds(o_ref, src, trg, P.lat_dim, P.stdim, delta)
        tot = 0.0
        for n in vref.LOSS_TERMS:
            allow = bound[n] + 1e-6 * abs(want_net[n])
            print("e2e %-22s got %.6f  ref %.6f  |d| %.2e  allowed %.2e" % (n, got[n], want_net[n], abs(got[n] - want_net[n]), allow))
            assert abs(got[n] - want_net[n]) <= allow, n
            if n not in ("loss_mcd_trg_src", "loss_mcd_src_trg"):
                tot += allow
        assert abs(got["loss"] - want_net["loss"]) <= tot
        for n in vref.DB_TERMS + vref.DIST_TERMS:
            print("e2e %-22s got %.12f  ref %.12f" % (n, got[n], want_met[n]))
            assert abs(got[n] - want_met[n]) <= 1e-10 * abs(want_met[n]), n
    s, s_ref = vp.summary(), met.summary()
    for k, v in s_ref.items():
        if k.startswith(("eval_mcd", "eval_lat_dist", "eval_gv")):
            assert abs(s[k] - v) <= 1e-10 * abs(v), (k, s[k], v)
    assert set(s) == set(s_ref)
    # :1153 -- the decision, against a "best so far" on either side of this epoch's score
    score = validation.ValidationPass.score(s)
    for shift in (-1e-3, 1e-3):
        best = dict(s_ref)
        best["eval_mcd_src_trg"] += shift
        assert validation.ValidationPass.better(s, best) == vref.better(s_ref, best) == (shift > 0.0)
    assert validation.ValidationPass.better(s, dict(s)) and vref.better(s_ref, dict(s_ref))      # "<=": a tie replaces
    assert validation.ValidationPass.better(s, None) and np.isfinite(score)
    assert isinstance(validation.ValidationPass.log_line(s), str)
