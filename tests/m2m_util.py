"""Many-to-many chains (per-cycle target codes and converted excitation): the problems, the float64 reference and the checks shared by
tests/test_m2m_cpu.py (host-fiber emulator, CPU tensors) and tests/test_m2m_gpu.py (device).

The float64 reference is oracle/torch_stock (StockGRURNN, train_forward_t), unchanged, fed float64 weights and inputs and composed per
cycle as the many-to-many training scripts compose it (the way tests/laplace_chain_ref.py composes the Laplace chain):

    lat_i   = E(x)  or  E([x[:,:,:stdim] ; rec_cyc_{i-1}])
    rec_i   = D([code_src ; z1]),   cv_i = D([code_trg[i] ; z2]),   latcv_i = E([cvx[i] ; cv_i]),   rec_cyc_i = D([code_src ; z3])

Bounds are the project's own: chain trajectories 5e-6 on the device (TIGHT_CHAIN) and EMU_CHAIN on the emulator (tests/stacked_util.py),
passes TIGHT_PASS / EMU_PASS, kernel against kernel TIGHT_KERNELS; Stage4Step loss 2e-6 relative and gradients 8e-6 relative to the
tensor's largest entry (tests/test_gpu_train.py)."""
import numpy as np
import torch

import laplace_chain_ref as R
import synth
from laplace_chain_util import N, T as TT, maxdiff, module
from oracle import torch_stock as ts

KEYS = R.KEYS
LOSS_REL, GRAD_REL = 2e-6, 8e-6        # tests/test_gpu_train.py: loss (window test), TIGHT_REL


class Problem(object):
    """One synthetic many-to-many workload: n_spk-wide one-hot codes, a source code per ROW, a target code per CYCLE and ROW (never the
    row's own speaker, and not the one of the cycle before), a converted excitation per cycle."""

    def __init__(self, B, T, in_dim, out_dim, lat_dim, hidden, ncode, n_cyc, tag, bias_scale=0.1, laplace=False):
        self.B, self.T, self.in_dim, self.out_dim, self.lat_dim, self.hidden = B, T, in_dim, out_dim, lat_dim, hidden
        self.ncode, self.n_cyc, self.stdim = ncode, n_cyc, in_dim - out_dim
        mu, sg = synth.feature_stats(tag + "/stats", in_dim)
        self.mu, self.sigma = mu, sg
        mu_t, sg_t = mu[self.stdim:], sg[self.stdim:]
        self.enc = synth.gru_rnn_state(tag + "/enc", in_dim, 2 * lat_dim, hidden, scale_in=(mu, sg), bias_scale=bias_scale)
        self.dec = synth.gru_rnn_state(tag + "/dec", ncode + lat_dim, out_dim, hidden, scale_out=(mu_t, sg_t), bias_scale=bias_scale)
        self.x = synth.features(tag + "/x", B, T, mu, sg)
        self.cvx = np.stack([synth.features(tag + "/cvx%d" % i, B, T, mu[:self.stdim], sg[:self.stdim]) for i in range(n_cyc)])
        src = np.arange(B) % ncode
        self.src_idx = src
        self.trg_idx = np.stack([(src + 1 + (i + np.arange(B)) % (ncode - 1)) % ncode for i in range(n_cyc)]) if ncode > 1 else np.zeros((n_cyc, B), int)
        self.code_src = np.zeros((B, T, ncode), np.float32)
        self.code_src[np.arange(B), :, src] = 1
        self.code_trg = np.zeros((n_cyc, B, T, ncode), np.float32)
        for i in range(n_cyc):
            self.code_trg[i, np.arange(B), :, self.trg_idx[i]] = 1
        self.y_in_enc = np.zeros((B, 1, 2 * lat_dim), np.float32)
        self.y_in_dec = np.broadcast_to(((0.0 - mu_t) / sg_t).astype(np.float32)[None, None, :], (B, 1, out_dim)).copy()
        shape = (n_cyc, 3, B, T, lat_dim)
        self.eps = synth.uniform(tag + "/ueps", shape, -0.4999, 0.5) if laplace else synth.normal(tag + "/eps", shape)


def problem_h64(n_cyc=2, laplace=False):
    """B 5, T 12, encoder in_dim 10, five speakers, lat_dim 4 (decoder in_dim 9)."""
    return Problem(5, 12, 10, 6, 4, 64, 5, n_cyc, "m2m64/%d" % n_cyc, laplace=laplace)


def problem_h1024(laplace=False):
    """B 4, T 8, the recipe's encoder (54 -> 64), twelve speakers at lat_dim 32: decoder in_dim 44 (KFW 7)."""
    return Problem(4, 8, 54, 50, 32, 1024, 12, 2, "m2m1024", bias_scale=0.05, laplace=laplace)


def modules(gv, P, dev, train=False):
    return (module(gv, P.enc, P.in_dim, 2 * P.lat_dim, P.hidden, True, dev, train=train),
            module(gv, P.dec, P.ncode + P.lat_dim, P.out_dim, P.hidden, False, dev, train=train))


def chain_args(P, dev, cvx=None, code_trg=None):
    """(x, cvx, code_src, code_trg, y_in_enc, y_in_dec) as device tensors; cvx / code_trg: other arrays than the problem's."""
    return [TT(a, dev) for a in (P.x, P.cvx if cvx is None else cvx, P.code_src, P.code_trg if code_trg is None else code_trg,
                                 P.y_in_enc, P.y_in_dec)]


def make_masks(P, tag):
    """Inverted-dropout masks (p = 0.5) of every pass of the chain: {"enc": [(cmask [B,T,9C], gmask [T,B,H])] * 2 n_cyc, "dec": * 3 n_cyc}
    (train_util.make_masks with the decoder's many-to-many width)."""
    out = {"enc": [], "dec": []}
    for kind, n, cin in (("enc", 2 * P.n_cyc, P.in_dim), ("dec", 3 * P.n_cyc, P.ncode + P.lat_dim)):
        for i in range(n):
            cm = (synth.uniform01("%s/%s%d/c" % (tag, kind, i), (P.B, P.T, 9 * cin)) >= 0.5).astype(np.float32) * 2.0
            gm = (synth.uniform01("%s/%s%d/g" % (tag, kind, i), (P.T, P.B, P.hidden)) >= 0.5).astype(np.float32) * 2.0
            out[kind].append((cm, gm))
    return out


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
def _draw(lat, eps, L, laplace):
    return R.draw(lat, eps, L) if laplace else lat[..., :L] + torch.exp(lat[..., L:] / 2) * eps


def _cyc(a, i):
    return a[i] if a.dim() == 4 else a


def ref_chain(P, posterior="gauss", cvx=None, code_trg=None, eps=None):
    """The eval chain in float64: {key: [n_cyc,B,T,C] numpy}."""
    lap, L = posterior == "laplace", P.lat_dim
    enc = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in P.enc.items()}, P.in_dim, 2 * L, P.hidden).double()
    dec = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in P.dec.items()}, P.ncode + L, P.out_dim, P.hidden).double()
    E = lambda x, y: R.clamp(enc(x, y)[0], L) if lap else enc(x, y, clamp_lat_dim=L)[0]
    X, CS, ye, yd = (R.t64(a) for a in (P.x, P.code_src, P.y_in_enc, P.y_in_dec))
    CVX, CT, EPS = R.t64(P.cvx if cvx is None else cvx), R.t64(P.code_trg if code_trg is None else code_trg), R.t64(P.eps if eps is None else eps)
    out = {k: [] for k in KEYS}
    prev = None
    for i in range(P.n_cyc):
        lat = E(X if i == 0 else torch.cat((X[:, :, :P.stdim], prev), 2), ye)
        rec = dec(torch.cat((CS, _draw(lat, EPS[i, 0], L, lap)), 2), yd)[0]
        cv = dec(torch.cat((_cyc(CT, i), _draw(lat, EPS[i, 1], L, lap)), 2), yd)[0]
        latcv = E(torch.cat((_cyc(CVX, i), cv), 2), ye)
        prev = dec(torch.cat((CS, _draw(latcv, EPS[i, 2], L, lap)), 2), yd)[0]
        for k, v in zip(KEYS, (lat, rec, cv, latcv, prev)):
            out[k].append(v.numpy())
    return {k: np.stack(v) for k, v in out.items()}


def _kl_gauss(par, L):
    return 0.5 * (par[..., L:].exp() + par[..., :L] ** 2 - par[..., L:] - 1.0).sum(-1)


def ref_loss(trajs, x, stdim, L, laplace, flen_acc=None):
    """train...:1363-1410 on float64 tensors, every utterance selected (the :1393 list quirk included)."""
    B, T_ = x.shape[0], x.shape[1]
    nfr = [T_] * B if flen_acc is None else [min(int(n), T_) for n in flen_acc]
    kl = R.kl if laplace else _kl_gauss
    tot = 0.0
    for tr in trajs:
        kls, kl_cv = [], None
        for j in range(B):
            n = nfr[j]
            tgt = x[j, :n, stdim:]
            tot = tot + (R.K_MCD_L1 * (tr["rec"][j, :n] - tgt).abs().sum(1)).mean() + (R.K_MCD_L1 * (tr["reccyc"][j, :n] - tgt).abs().sum(1)).mean()
            kls.append(kl(tr["lat"][j, :n], L).mean())
            kl_cv = kl(tr["latcv"][j, :n], L).mean()
        tot = tot + sum(kls) + (sum(kls) if B > 1 else 0.0) + kl_cv
    return tot


def ref_step(P, masks, posterior="gauss", lr=1e-4):
    """One stage-4 step in float64 (train-mode chain with the supplied masks and eps, loss, backward, Adam):
    (loss, {kind: {name: gradient}}, {kind: {name: weight after the step}})."""
    import stage4
    lap, L = posterior == "laplace", P.lat_dim
    leaf = {k: {n: R.t64(v).requires_grad_(n in stage4.TRAINABLE) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}
    X, CVX, CS, CT, E = (R.t64(a) for a in (P.x, P.cvx, P.code_src, P.code_trg, P.eps))
    ye, yd = R.t64(P.y_in_enc), R.t64(P.y_in_dec)
    cnt = {"enc": 0, "dec": 0}

    def run(kind, xin, y, cl):
        cm, gm = masks[kind][cnt[kind]]
        cnt[kind] += 1
        h0 = torch.zeros(1, xin.shape[0], P.hidden, dtype=torch.float64)
        if cl >= 0 and lap:
            return R.clamp(ts.train_forward_t(leaf[kind], xin, y, R.t64(cm), R.t64(gm), -1, h_in=h0), cl)
        return ts.train_forward_t(leaf[kind], xin, y, R.t64(cm), R.t64(gm), cl, h_in=h0)

    trajs, prev = [], None
    for i in range(P.n_cyc):
        lat = run("enc", X if i == 0 else torch.cat((X[:, :, :P.stdim], prev), 2), ye, L)
        rec = run("dec", torch.cat((CS, _draw(lat, E[i, 0], L, lap)), 2), yd, -1)
        cv = run("dec", torch.cat((CT[i], _draw(lat, E[i, 1], L, lap)), 2), yd, -1)
        latcv = run("enc", torch.cat((CVX[i], cv), 2), ye, L)
        prev = run("dec", torch.cat((CS, _draw(latcv, E[i, 2], L, lap)), 2), yd, -1)
        trajs.append({"lat": lat, "rec": rec, "cv": cv, "latcv": latcv, "reccyc": prev})
    loss = ref_loss(trajs, X, P.stdim, L, lap)
    params = [p for k in ("enc", "dec") for p in leaf[k].values() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    opt.zero_grad()
    loss.backward()
    grads = {k: {n: p.grad.numpy().copy() for n, p in leaf[k].items() if p.requires_grad} for k in leaf}
    opt.step()
    after = {k: {n: p.detach().numpy().copy() for n, p in leaf[k].items() if p.requires_grad} for k in leaf}
    return float(loss.item()), grads, after


def ref_pass(sd, in_dim, out_dim, hidden, x, y_in):
    """One eval pass in float64 (no clamp): [B,T,out_dim] numpy."""
    net = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in sd.items()}, in_dim, out_dim, hidden).double()
    return net(R.t64(x), R.t64(y_in))[0].numpy()


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def require_feature(gv):
    """Every test asks before it launches: on a tree without the feature a 4-D tensor would be read as its first slice."""
    import _cabi
    assert getattr(gv.CycleChain, "per_cycle_inputs", False) is True, "CycleChain.per_cycle_inputs is absent: no per-cycle inputs in this tree"
    assert "cvae_cycle_forward_m2m" in _cabi.EXPORTS and hasattr(gv._lib().lib, "cvae_cycle_forward_m2m"), "cvae_cycle_forward_m2m is not exported"


def same(a, b, what):
    a, b = (v if isinstance(v, np.ndarray) else N(v) for v in (a, b))
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s differs (max|d| %.3e)" % (what, float(np.max(np.abs(a - b))))


def repeat_cycles(a, n):
    return np.ascontiguousarray(np.broadcast_to(a[None], (n,) + a.shape))


def check_chain_identity(gv, dev, P, posterior):
    """1. equal cycle slices give the 3-D call's outputs bit for bit: fresh form (both arguments 4-D) and carry form (two windows, the
    state handed on, each argument 4-D on its own in one of them)."""
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior=posterior)
    cvx3, trg3 = P.cvx[0], P.code_trg[0]
    cvx4, trg4 = repeat_cycles(cvx3, P.n_cyc), repeat_cycles(trg3, P.n_cyc)
    eps = TT(P.eps, dev)
    base = chain(*chain_args(P, dev, cvx3, trg3), eps=eps)
    out = chain(*chain_args(P, dev, cvx4, trg4), eps=eps)
    for k in KEYS:
        same(out[k], base[k], "fresh chain (%s, both 4-D) %s" % (posterior, k))
    # carry form: window 0 with cvx alone 4-D, window 1 with code_trg alone 4-D (either argument on its own)
    h = P.T // 2
    win = lambda args, a, b: [v[..., a:b, :].contiguous() for v in args[:4]] + args[4:]
    res = []
    for (c0, t0), (c1, t1) in (((cvx3, trg3), (cvx3, trg3)), ((cvx4, trg3), (cvx3, trg4))):
        oa, st = chain(*win(chain_args(P, dev, c0, t0), 0, h), eps=eps[:, :, :, :h].contiguous(), return_state=True)
        ob, st2 = chain(*win(chain_args(P, dev, c1, t1), h, P.T), eps=eps[:, :, :, h:].contiguous(), state=st, return_state=True)
        res.append((oa, ob, st, st2))
    for q in (0, 1):
        for k in KEYS:
            same(res[1][q][k], res[0][q][k], "carry chain (%s) window %d %s" % (posterior, q, k))
    for q in (2, 3):
        for k in res[0][q]:
            same(res[1][q][k], res[0][q][k], "carry chain (%s) state %d %s" % (posterior, q - 2, k))


def check_entry_identity(gv, dev, P):
    """1. the C entry point with both strides 0 against cvae_cycle_forward: the same bits in every output."""
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    lib = gv._lib()
    x, cvx, cs, ct, ye, yd = chain_args(P, dev, P.cvx[0], P.code_trg[0])
    eps = TT(P.eps, dev)
    de, ie = enc.prepared(dev)
    dd, idd = dec.prepared(dev)
    n, B, T_, L, Co = P.n_cyc, P.B, P.T, P.lat_dim, P.out_dim
    ws = torch.empty(lib.cycle_workspace_bytes(de, dd, B, T_, n), dtype=torch.uint8, device=dev)
    res = []
    for m2m in (False, True):
        out = {k: torch.full((n, B, T_, c), float("nan"), dtype=torch.float32, device=dev)
               for k, c in (("lat", 2 * L), ("rec", Co), ("cv", Co), ("latcv", 2 * L), ("reccyc", Co))}
        a = (de, ie.data_ptr(), dd, idd.data_ptr(), x.data_ptr(), cvx.data_ptr(), P.stdim, cs.data_ptr(), ct.data_ptr(), P.ncode,
             ye.reshape(B, -1).data_ptr(), yd.reshape(B, -1).data_ptr(), B, T_, n, L, eps.data_ptr(), 0) + \
            tuple(out[k].data_ptr() for k in KEYS[:1] + ("rec", "cv", "latcv", "reccyc")) + (ws.data_ptr(), ws.numel(), gv._flags(), gv._stream())
        if m2m:
            lib.cycle_forward_m2m(*a, None, None, 0, 0)
        else:
            lib.cycle_forward(*a)
        res.append(out)
    for k in KEYS:
        assert np.all(np.isfinite(N(res[0][k])))
        same(res[1][k], res[0][k], "cvae_cycle_forward_m2m(strides 0) " + k)


def check_bad_strides(gv, dev, P):
    """4. a negative stride, or a positive one shorter than a cycle's block, gives status -1 and launches nothing (the outputs keep
    their fill)."""
    import _cabi
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    lib = gv._lib()
    x, cvx, cs, ct, ye, yd = chain_args(P, dev)
    de, ie = enc.prepared(dev)
    dd, idd = dec.prepared(dev)
    n, B, T_, L, Co = P.n_cyc, P.B, P.T, P.lat_dim, P.out_dim
    ws = torch.zeros(lib.cycle_workspace_bytes(de, dd, B, T_, n), dtype=torch.uint8, device=dev)
    out = {k: torch.full((n, B, T_, c), 7.0, dtype=torch.float32, device=dev)
           for k, c in (("lat", 2 * L), ("rec", Co), ("cv", Co), ("latcv", 2 * L), ("reccyc", Co))}
    C = _cabi.C
    ye, yd = ye.reshape(B, -1), yd.reshape(B, -1)
    full_c, full_t = B * T_ * P.stdim, B * T_ * P.ncode
    for sc, st in ((-1, full_t), (full_c, -full_t), (full_c - 1, full_t), (full_c, full_t - 1), (1, 0), (0, 1)):
        raw = lib.lib.cvae_cycle_forward_m2m(C.byref(de), ie.data_ptr(), C.byref(dd), idd.data_ptr(), x.data_ptr(), cvx.data_ptr(), P.stdim,
                                             cs.data_ptr(), ct.data_ptr(), P.ncode, ye.data_ptr(), yd.data_ptr(), B, T_, n, L, None, 5,
                                             out["lat"].data_ptr(), out["rec"].data_ptr(), out["cv"].data_ptr(), out["latcv"].data_ptr(),
                                             out["reccyc"].data_ptr(), ws.data_ptr(), ws.numel(), gv._flags(), gv._stream() or None,
                                             None, None, sc, st)
        assert raw == -1, (sc, st, raw)
        with torch.no_grad():
            for k in out:
                assert bool((out[k] == 7.0).all()), (sc, st, k)
        assert not bool(ws.any()), (sc, st)


def check_chain_parity(gv, dev, P, posterior, bound, what):
    """2. / 9. distinct per-cycle inputs: every trajectory of the fresh chain against the float64 reference, and the carry form (two
    windows) against the same."""
    require_feature(gv)
    assert not np.array_equal(P.code_trg[0], P.code_trg[1]) and not np.array_equal(P.cvx[0], P.cvx[1])
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior=posterior)
    eps = TT(P.eps, dev)
    args = chain_args(P, dev)
    out = chain(*args, eps=eps)
    ref = ref_chain(P, posterior)
    worst = {k: maxdiff(N(out[k]), ref[k]) for k in KEYS}
    print("%s %s fresh: %s (bound %.1e)" % (what, posterior, " ".join("%s %.3e" % kv for kv in worst.items()), bound))
    assert max(worst.values()) <= bound, worst
    return out, ref


def check_chain_carry_parity(gv, dev, P, posterior, bound, what):
    """2. the carry form with per-cycle inputs: two windows, each pass continuing from its own state; the windows' frames against the
    float64 reference's windowed composition (every window re-pads its front-end, as the reference's loop does)."""
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior=posterior)
    eps = TT(P.eps, dev)
    args = chain_args(P, dev)
    h = P.T // 2
    win = lambda a, b: [v[..., a:b, :].contiguous() for v in args[:4]] + args[4:]
    oa, st = chain(*win(0, h), eps=eps[:, :, :, :h].contiguous(), return_state=True)
    ob = chain(*win(h, P.T), eps=eps[:, :, :, h:].contiguous(), state=st)
    ref = ref_chain_windows(P, posterior, [(0, h), (h, P.T)])
    worst = {k: maxdiff(np.concatenate((N(oa[k]), N(ob[k])), 2), ref[k]) for k in KEYS}
    print("%s %s carry: %s (bound %.1e)" % (what, posterior, " ".join("%s %.3e" % kv for kv in worst.items()), bound))
    assert max(worst.values()) <= bound, worst


def ref_chain_windows(P, posterior, windows):
    """ref_chain over frame windows, every pass continuing from its own (y_last, h) of the window before."""
    lap, L = posterior == "laplace", P.lat_dim
    enc = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in P.enc.items()}, P.in_dim, 2 * L, P.hidden).double()
    dec = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in P.dec.items()}, P.ncode + L, P.out_dim, P.hidden).double()
    X, CS, CVX, CT, EPS = (R.t64(a) for a in (P.x, P.code_src, P.cvx, P.code_trg, P.eps))
    ye, yd = R.t64(P.y_in_enc), R.t64(P.y_in_dec)
    out = {k: [[] for _ in range(P.n_cyc)] for k in KEYS}
    state = {}

    def one(net, slot, i, xin, y0, cl):
        y, hh = state.get((i, slot), (y0, None))
        o, y1, h1 = net(xin, y, hh) if (lap or cl < 0) else net(xin, y, hh, clamp_lat_dim=cl)
        if lap and cl >= 0:
            o = R.clamp(o, cl)
        state[(i, slot)] = (y1, h1)
        out[slot][i].append(o)
        return o

    for a, b in windows:
        x, cs, e = X[:, a:b], CS[:, a:b], EPS[:, :, :, a:b]
        prev = None
        for i in range(P.n_cyc):
            lat = one(enc, "lat", i, x if i == 0 else torch.cat((x[:, :, :P.stdim], prev), 2), ye, L)
            one(dec, "rec", i, torch.cat((cs, _draw(lat, e[i, 0], L, lap)), 2), yd, -1)
            cv = one(dec, "cv", i, torch.cat((CT[i][:, a:b], _draw(lat, e[i, 1], L, lap)), 2), yd, -1)
            latcv = one(enc, "latcv", i, torch.cat((CVX[i][:, a:b], cv), 2), ye, L)
            prev = one(dec, "reccyc", i, torch.cat((cs, _draw(latcv, e[i, 2], L, lap)), 2), yd, -1)
    return {k: np.stack([torch.cat(v, 1).numpy() for v in out[k]]) for k in KEYS}


def check_cycle_selection(gv, dev, P):
    """3. changing only code_trg[1] changes cv of cycle 1 and no bit of cycle 0 (nor lat / rec of cycle 1, which do not read it); the
    same for cvx[1] and latcv."""
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc)
    eps = TT(P.eps, dev)
    base = chain(*chain_args(P, dev), eps=eps)
    trg = P.code_trg.copy()
    trg[1] = np.roll(trg[1], 1, axis=-1)                 # another speaker for every row
    assert not np.array_equal(trg[1], P.code_trg[1]) and not np.array_equal(trg[1], trg[0])
    a = chain(*chain_args(P, dev, code_trg=trg), eps=eps)
    for k in KEYS:
        same(a[k][0], base[k][0], "cycle 0 %s after a change of code_trg[1]" % k)
    same(a["lat"][1], base["lat"][1], "cycle 1 lat")
    same(a["rec"][1], base["rec"][1], "cycle 1 rec")
    assert not np.array_equal(N(a["cv"][1]), N(base["cv"][1])), "cv of cycle 1 does not read code_trg[1]"
    cvx = P.cvx.copy()
    cvx[1] = cvx[1] + 0.25
    b = chain(*chain_args(P, dev, cvx=cvx), eps=eps)
    for k in KEYS:
        same(b[k][0], base[k][0], "cycle 0 %s after a change of cvx[1]" % k)
    for k in ("lat", "rec", "cv"):
        same(b[k][1], base[k][1], "cycle 1 " + k)
    assert not np.array_equal(N(b["latcv"][1]), N(base["latcv"][1])), "latcv of cycle 1 does not read cvx[1]"


def check_shape_errors(gv, dev, P):
    """4. a cycle axis that is not n_cyc, or trailing shapes that do not fit, raise ValueError in CycleChain, stage4.chain_forward and
    Stage4Step before any pass runs."""
    import pytest
    import stage4
    require_feature(gv)
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc)
    n = P.n_cyc
    bad = [dict(code_trg=repeat_cycles(P.code_trg[0], n + 1)), dict(cvx=repeat_cycles(P.cvx[0], n - 1)),
           dict(code_trg=P.code_trg[:, :, :, :-1]), dict(code_trg=P.code_trg[:, :-1]), dict(cvx=P.cvx[:, :, :-1]),
           dict(cvx=P.cvx[None])]
    calls = []

    def run_pass(*a):
        calls.append(a)
        raise AssertionError("a pass ran")

    for kw in bad:
        args = chain_args(P, dev, **{k: np.ascontiguousarray(v) for k, v in kw.items()})
        with pytest.raises(ValueError):
            chain(*args, eps=TT(P.eps, dev))
        with pytest.raises(ValueError):
            stage4.chain_forward(run_pass, *args, TT(P.eps, dev), P.lat_dim, n)
    assert not calls
    # Stage4Step refuses at the top of the call: the gradient buffer is not even zeroed, no weight moves
    step, enc_t, dec_t = step_of(gv, P, dev, fused=None)
    step.grads.flat.fill_(7.0)
    before = [N(p).copy() for m in (enc_t, dec_t) for p in m.parameters()]
    for kw in bad:
        args = chain_args(P, dev, **{k: np.ascontiguousarray(v) for k, v in kw.items()})
        with pytest.raises(ValueError):
            step(*args, TT(P.eps, dev))
    assert bool((step.grads.flat == 7.0).all()) and step.step_no == 0
    for b, p in zip(before, [p for m in (enc_t, dec_t) for p in m.parameters()]):
        assert np.array_equal(b, N(p))


def step_of(gv, P, dev, fused, posterior="gauss", stack=True):
    import stage4
    enc, dec = modules(gv, P, dev, train=True)
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-4, fused=fused, posterior=posterior, stack_rec_cv=stack)
    return step, enc, dec


def check_step_identity(gv, dev, P, fused):
    """1. Stage4Step with 4-D inputs whose slices are equal: loss, every gradient and the weights after the step are the 3-D call's,
    bit for bit (injected masks and eps)."""
    require_feature(gv)
    masks_np = make_masks(P, "m2m/idmasks/%d" % P.hidden)
    masks = {k: [(TT(a, dev), TT(b, dev)) for a, b in v] for k, v in masks_np.items()}
    cvx3, trg3 = P.cvx[0], P.code_trg[0]
    res = []
    for c, t in ((cvx3, trg3), (repeat_cycles(cvx3, P.n_cyc), repeat_cycles(trg3, P.n_cyc))):
        step, enc, dec = step_of(gv, P, dev, fused)
        assert step.fused == fused
        loss = step(*chain_args(P, dev, c, t), TT(P.eps, dev), masks=masks)
        res.append((N(loss).copy(), N(step.grads.flat).copy(), [N(p).copy() for m in (enc, dec) for p in m.parameters()]))
    assert np.isfinite(res[0][0]) and res[0][0].tobytes() == res[1][0].tobytes(), (res[0][0], res[1][0])
    assert np.abs(res[0][1]).max() > 0 and res[0][1].tobytes() == res[1][1].tobytes(), "gradients differ"
    for a, b in zip(res[0][2], res[1][2]):
        assert a.tobytes() == b.tobytes(), "weights after the step differ"


def check_step_parity(gv, dev, P, forms, what, stack=True):
    """2. / 9. Stage4Step with distinct per-cycle inputs against the float64 reference: loss 2e-6 relative, every gradient 8e-6 of the
    tensor's largest entry (at least 1)."""
    import stage4
    require_feature(gv)
    masks_np = make_masks(P, "m2m/masks/%d" % P.hidden)
    ref_loss_, ref_g, _ = ref_step(P, masks_np)
    masks = {k: [(TT(a, dev), TT(b, dev)) for a, b in v] for k, v in masks_np.items()}
    for fused in forms:
        step, enc, dec = step_of(gv, P, dev, fused, stack=stack)
        assert step.fused == fused
        loss = float(step(*chain_args(P, dev), TT(P.eps, dev), masks=masks).item())
        rel = abs(loss - ref_loss_) / abs(ref_loss_)
        worst = 0.0
        for kind, m in (("enc", enc), ("dec", dec)):
            named = dict(m.named_parameters())
            for k in stage4.TRAINABLE:
                g, r = N(named[k].grad).astype(np.float64), ref_g[kind][k]
                worst = max(worst, float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r)))))
        print("%s step fused=%s stack=%s: loss %.7f float64 %.7f (rel %.3e, bound %.1e); gradients %.3e (bound %.1e)"
              % (what, fused, stack, loss, ref_loss_, rel, LOSS_REL, worst, GRAD_REL))
        assert rel <= LOSS_REL, (loss, ref_loss_)
        assert worst <= GRAD_REL, worst


def check_chain_forward_unfused_matches(gv, dev, P):
    """A. stage4.chain_forward / chain_loss on plain torch (float64, the stock passes) take the same shapes: the loss equals the
    reference's own composition."""
    import stage4
    require_feature(gv)
    masks = make_masks(P, "m2m/masks/%d" % P.hidden)
    leaf = {k: {n: R.t64(v) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}

    def run_pass(kind, x, y_in, clamp, mk):
        h0 = torch.zeros(1, x.shape[0], P.hidden, dtype=torch.float64)
        return ts.train_forward_t(leaf[kind], x, y_in, R.t64(mk[0]), R.t64(mk[1]), clamp, h_in=h0)

    a = [R.t64(v) for v in (P.x, P.cvx, P.code_src, P.code_trg, P.y_in_enc, P.y_in_dec, P.eps)]
    loss = stage4.chain_loss(run_pass, *a, P.lat_dim, P.n_cyc, masks)
    ref = ref_step(P, masks)[0]
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)       # (loss_terms' frame weights 1 / n are float32)


def collated_batch(B=3, T=9, n_cyc=2, cin=10, stdim=4):
    """A default-collated FeatureDatasetMultTrainVAE batch: three source and two target speakers, items built by the dataset's own
    __getitem__ from an in-memory reader, collated by torch's default_collate."""
    import loader_m2m
    from torch.utils.data import default_collate
    src, trg = ["SA", "SB", "SC"], ["TA", "TB"]
    files = ["/data/%s/u%d.h5" % (s, q) for q, s in enumerate(("SA", "TB", "SC"))][:B]
    flens = [T, T - 2, T - 4][:B]
    store = {}

    def reader(path, key):
        spk, utt = path.split("/")[-2], path.split("/")[-1]
        n = flens[int(utt[1])]
        if key == "/feat_org_lf0":
            return synth.normal("m2mbatch/%s/%s/feat" % (spk, utt), (n, cin)).astype(np.float64)
        if key == "/spcidx_range":
            return np.arange(n, dtype=np.int64)[None]
        assert key.startswith("/cvuvlogf0fil_ap_"), key
        store.setdefault((path, key), synth.normal("m2mbatch/%s%s" % (path, key), (n, stdim)).astype(np.float64))
        return store[(path, key)]

    def pad(a):
        out = np.zeros((T,) + a.shape[1:], a.dtype)
        out[:a.shape[0]] = a
        return out

    ds = loader_m2m.FeatureDatasetMultTrainVAE(files, pad, src, trg, n_cyc, reader=reader)
    state = np.random.get_state()
    np.random.seed(7)
    try:
        items = [ds[i] for i in range(B)]
    finally:
        np.random.set_state(state)
    return default_collate(items), items, (src, trg, flens, store)


def check_chain_inputs(gv, dev, run_step=True):
    """5. loader_m2m.chain_inputs on a collated batch of three utterances (two of source speakers, one of a target speaker), n_cyc 2:
    shapes, one-hot positions, stacking order, frame lengths -- and Stage4Step takes the result (run_step=False: CycleChain does; a
    train-mode step costs the emulator half a minute)."""
    import loader_m2m
    import stage4
    assert hasattr(loader_m2m, "chain_inputs"), "loader_m2m.chain_inputs is absent"
    batch, items, (src, trg, flens, store) = collated_batch()
    a = loader_m2m.chain_inputs(batch)
    B, T_, n_spk = 3, 9, 5
    assert sorted(a) == ["code_src", "code_trg", "cvx", "flen_acc", "x"]
    assert tuple(a["x"].shape) == (B, T_, 10) and tuple(a["code_src"].shape) == (B, T_, n_spk)
    assert tuple(a["code_trg"].shape) == (2, B, T_, n_spk) and tuple(a["cvx"].shape) == (2, B, T_, 4)
    assert a["flen_acc"] == flens
    own = [0, 3 + 1, 2]                                   # SA, TB (behind the three source speakers), SC
    for j, it in enumerate(items):
        n = flens[j]
        cs = N(a["code_src"][j])
        assert np.all(cs[:n].argmax(1) == own[j]) and np.all(cs[:n].sum(1) == 1) and not cs[n:].any()
        for i in range(2):
            spk = it["pair_spk_list"][i]
            col = (src + trg).index(spk)
            assert (spk in trg) == (j != 1)               # a source utterance converts to a target speaker and v.v.
            ct = N(a["code_trg"][i, j])
            assert np.all(ct[:n].argmax(1) == col) and np.all(ct[:n].sum(1) == 1) and not ct[n:].any()
            assert np.array_equal(N(a["code_trg"][i, j]), N(it["src_trg_code_list"][i]))
            assert np.array_equal(N(a["cvx"][i, j]), N(it["cv_src_list"][i]))
            assert np.array_equal(N(a["cvx"][i, j, :n]), store[(it["featfile_src"], "/cvuvlogf0fil_ap_" + spk)].astype(np.float32))
        assert np.array_equal(N(a["x"][j]), N(it["h_src"]))
    import pytest
    with pytest.raises(ValueError):
        loader_m2m.chain_inputs({k: v for k, v in batch.items() if k != "cv_src_list"})
    require_feature(gv)
    P = Problem(B, T_, 10, 6, 4, 64, n_spk, 2, "m2m/batchnets")
    if not run_step:
        enc, dec = modules(gv, P, dev)
        out = gv.CycleChain(enc, dec, 4, 2)(a["x"].to(dev), a["cvx"].to(dev), a["code_src"].to(dev), a["code_trg"].to(dev),
                                            TT(P.y_in_enc, dev), TT(P.y_in_dec, dev), eps=TT(P.eps, dev))
        assert all(np.all(np.isfinite(N(out[k]))) for k in KEYS)
        return
    enc, dec = modules(gv, P, dev, train=True)
    step = stage4.Stage4Step(enc, dec, lat_dim=4, n_cyc=2, lr=1e-4)
    args = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in a.items()}
    before = [N(p).copy() for p in dec.parameters()]
    loss = step(y_in_enc=TT(P.y_in_enc, dev), y_in_dec=TT(P.y_in_dec, dev), eps=TT(P.eps, dev), **args)
    assert np.isfinite(float(loss))
    assert any(not np.array_equal(b, N(p)) for b, p in zip(before, dec.parameters()))


# ---- stage 6: one source, many targets ---------------------------------------------------------------------------------------------
N_SMPL = 3


def targets_problem(hidden):
    """Nets of two code columns (so that convert_pairs, whose codes are the fixed (1,0) / (0,1), can be asked the same question), a
    12-frame source utterance, three draws."""
    P = Problem(1, 12, 10, 6, 4, 64, 2, 1, "m2m/s6/64") if hidden == 64 else Problem(1, 12, 54, 50, 32, 1024, 2, 1, "m2m/s6/1024", bias_scale=0.05)
    feat = synth.features("m2m/s6/%d/feat" % hidden, 1, 12, P.mu, P.sigma)[0]
    eps = synth.normal("m2m/s6/%d/eps" % hidden, (N_SMPL, 12, P.lat_dim))
    return P, feat, eps


TARGET_CODES = np.asarray([[0, 1], [1, 0], [0.25, 0.75], [0, 1], [0.5, 0.5], [1, 0]], np.float32)      # K = 1, 3, 6: the first K rows


def check_convert_targets(gv, dev, hidden, bound):
    """6. K = 1, 3, 6: a row of cv with the code (0,1) is convert_pairs' cvmcep, one with (1,0) -- and rec -- its cvmcep_src, bit for
    bit, for the same source and draws; a row's bits do not depend on K; every row against the float64 reference.
    convert_pairs is asked with TWO pairs of the same source: a one-pair call runs three decoder rows on the word-exchange kernels,
    whose sums are ordered differently; from four rows on every call runs the row-tile kernels convert_targets always runs."""
    import pytest
    import stage6
    assert hasattr(stage6, "convert_targets"), "stage6.convert_targets is absent"
    P, feat, eps = targets_problem(hidden)
    enc, dec = modules(gv, P, dev)
    L = P.lat_dim
    fd, ed = TT(feat, dev), TT(eps, dev)
    y_pp, y_dec = TT(np.zeros((1, 1, 2 * L), np.float32), dev), TT(P.y_in_dec[:1], dev)
    src = np.asarray([1, 0], np.float32)
    pairs = stage6.convert_pairs(enc, dec, [(fd, fd), (fd, fd)], y_pp, y_dec, y_dec, L, n_smpl_dec=N_SMPL, eps=[(ed, ed), (ed, ed)])
    cvmcep, cvmcep_src, _, lat_src, _ = pairs[0]
    # float64: lat, z = mu + exp(s/2) mean(eps), D([code ; z])
    e64 = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in P.enc.items()}, P.in_dim, 2 * L, P.hidden).double()
    lat64 = e64(R.t64(feat)[None], R.t64(np.zeros((1, 1, 2 * L))), clamp_lat_dim=L)[0]
    z64 = lat64[..., :L] + torch.exp(lat64[..., L:] / 2) * R.t64(eps).mean(0)[None]
    ref_row = lambda code: ref_pass(P.dec, 2 + L, P.out_dim, P.hidden, torch.cat((R.t64(code).expand(1, 12, 2), z64), 2).numpy(), P.y_in_dec[:1])[0]
    rows = {}
    for K in (1, 3, 6):
        lat, rec, cv = stage6.convert_targets(enc, dec, fd, TT(src, dev), TT(TARGET_CODES[:K], dev), y_pp, y_dec, L, n_smpl_dec=N_SMPL, eps=ed)
        assert tuple(cv.shape) == (K, 12, P.out_dim) and tuple(rec.shape) == (12, P.out_dim) and tuple(lat.shape) == (12, 2 * L)
        same(lat, lat_src, "H%d K=%d lat" % (hidden, K))
        same(rec, cvmcep_src, "H%d K=%d rec against convert_pairs' cvmcep_src" % (hidden, K))
        worst = maxdiff(N(rec), ref_row(src))
        for k in range(K):
            code = TARGET_CODES[k]
            if tuple(code) == (0, 1):
                same(cv[k], cvmcep, "H%d K=%d cv[%d] against convert_pairs' cvmcep" % (hidden, K, k))
            if tuple(code) == (1, 0):
                same(cv[k], cvmcep_src, "H%d K=%d cv[%d] against convert_pairs' cvmcep_src" % (hidden, K, k))
            if k in rows:
                same(cv[k], rows[k], "H%d cv[%d] at K=%d against a smaller K" % (hidden, k, K))
            rows[k] = N(cv[k]).copy()
            worst = max(worst, maxdiff(N(cv[k]), ref_row(code)))
        print("convert_targets H%d K=%d: max|d| vs float64 = %.3e (bound %.1e)" % (hidden, K, worst, bound))
        assert worst <= bound
    assert not np.array_equal(rows[0], rows[2])
    # Philox: the draw ids of a convert_pairs source (2 n q for list position q)
    pp = stage6.convert_pairs(enc, dec, [(fd, fd), (fd, fd)], y_pp, y_dec, y_dec, L, n_smpl_dec=N_SMPL, seed=99)
    for q in (0, 1):
        _, _, cvq = stage6.convert_targets(enc, dec, fd, TT(src, dev), TT(TARGET_CODES[:1], dev), y_pp, y_dec, L, n_smpl_dec=N_SMPL,
                                           draw_id=2 * N_SMPL * q, seed=99)
        same(cvq[0], pp[q][0], "H%d Philox draws of list position %d" % (hidden, q))
    for K in (0, 32):
        with pytest.raises(ValueError):
            stage6.convert_targets(enc, dec, fd, TT(src, dev), torch.zeros(K, 2), y_pp, y_dec, L, n_smpl_dec=N_SMPL, eps=ed)


# ---- the exact-operand recurrence at the many-to-many decoder widths ---------------------------------------------------------------
NEW_WIDTHS = ((28, 5), (44, 7), (60, 9), (68, 11))       # decoder in_dim at H = 1024 -> front-end 16-k steps per wave (KFW)


def check_plan(lib):
    """7. cvae_plan_pass at H = 1024, 64 rows: V6 at the four widths with the default flags, V2 at in_dim 20 (KFW 4: no instance) and,
    without EXACT3, at all of them."""
    import _cabi
    P_, E_, S_ = _cabi.FLAG_PERSISTENT, _cabi.FLAG_EXACT3, _cabi.FLAG_SPLIT_F16
    for in_dim, _ in NEW_WIDTHS:
        d = lib.desc(in_dim, 50, 1024, 3, 2, False, True)
        assert lib.plan_pass(d, 64, 80, P_ | E_ | S_) == _cabi.EVAL_V6, in_dim
        assert lib.plan_pass(d, 64, 80, P_ | S_) == _cabi.EVAL_V2, in_dim
        assert lib.plan_pass(d, 64, 80, P_) == _cabi.EVAL_V2, in_dim
    d = lib.desc(20, 50, 1024, 3, 2, False, True)
    assert lib.plan_pass(d, 64, 80, P_ | E_ | S_) == _cabi.EVAL_V2
    assert lib.plan_pass(d, 64, 80, P_ | S_) == _cabi.EVAL_V2


def decoder_case(in_dim, rows, T_=8):
    """A decoder-shaped pass (scale_out, no clamp) of the given input width at H = 1024: (state dict, x [rows,T,in_dim], y_in)."""
    tag = "m2m/width/%d" % in_dim
    mu, sg = synth.feature_stats(tag + "/stats", 50)
    sd = synth.gru_rnn_state(tag + "/dec", in_dim, 50, 1024, scale_out=(mu, sg), bias_scale=0.05)
    x = synth.normal(tag + "/x%d" % rows, (rows, T_, in_dim)).astype(np.float32)
    x[:, :, :in_dim - 32] = 0
    x[np.arange(rows), :, np.arange(rows) % (in_dim - 32)] = 1          # [one-hot code ; z]
    y = np.broadcast_to(((0.0 - mu) / sg).astype(np.float32)[None, None, :], (rows, 1, 50)).copy()
    return sd, x, y


def check_new_instance(mem, in_dim, kfw, rows, note=print):
    """8. one decoder-shaped pass through k_gru_steps_v6<16, KFW, 3> inside a NaN-filled arena with every buffer at its queried size
    (width_util.EvalNet): against float64 at 5e-6, against the same pass under GENERIC_STEP at 3e-6."""
    import _cabi
    import width_util as W
    from stacked_util import TIGHT_KERNELS, TIGHT_PASS
    sd, x, y = decoder_case(in_dim, rows)
    net = W.EvalNet(mem, sd, in_dim, 50, 1024)
    what = "in_dim %d (KFW %d) %d rows" % (in_dim, kfw, rows)
    got = net.forward(x, y, flags=W.DEFAULT_FLAGS, expect=_cabi.EVAL_V6, what=what)
    gen = net.forward(x, y, flags=W.DEFAULT_FLAGS | _cabi.FLAG_GENERIC_STEP, expect=_cabi.EVAL_GENERIC, what=what + " generic")
    ref = ref_pass(sd, in_dim, 50, 1024, x, y)
    d_ref, d_gen = maxdiff(got[0], ref), max(maxdiff(a, b) for a, b in zip(got, gen))
    note("%-9s m2m width %s: max|d| vs float64 %.3e (bound %.1e), vs the generic step %.3e (bound %.1e)"
         % (mem.name, what, d_ref, TIGHT_PASS, d_gen, TIGHT_KERNELS))
    assert d_ref <= TIGHT_PASS and d_gen <= TIGHT_KERNELS, (what, d_ref, d_gen)
