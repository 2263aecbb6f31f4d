"""Float64 reference of the Laplace-posterior chain, stage 6 and stage-4 step (CPU, torch): oracle/torch_stock.StockGRURNN and
train_forward_t, unchanged, fed float64 weights and inputs, with what the reference adds for the Laplace posterior written out here:

    clamp    out[..., L:] >= FLOOR                                        (GRU_RNN.forward, clamp_vae_laplace, gru_vae.py:415-417)
    draw     z = mu - exp(s) * sign(eps) * log1p(-2|eps|)                 (sampling_vae_laplace, :101-112)
    KL       mean over frames of sum_d(-s + b exp(-|mu|/b) + |mu| - 1)    (loss_vae_laplace, :130-139), b = exp(s)

composed as train_gru_cyclevae_gauss_batch.py:1326-1338 / :1363-1410 composes the Gaussian functions (the :1393 quirk included)."""
import numpy as np
import torch

from oracle import torch_stock as ts

FLOOR = -7.2543288692621097067625904247823
K_MCD_L1 = (10.0 / 2.3025850929940456840179914546844) * 1.4142135623730950488016887242097
KEYS = ("lat", "rec", "cv", "latcv", "reccyc")


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def draw(lat, eps, L):
    return lat[..., :L] - torch.exp(lat[..., L:]) * torch.sign(eps) * torch.log1p(-2 * torch.abs(eps))


def clamp(out, L):
    return torch.cat((out[..., :L], torch.clamp(out[..., L:], min=FLOOR)), -1)


def kl(par, L):
    """sum over latent dims per frame."""
    ma, s = par[..., :L].abs(), par[..., L:]
    b = torch.exp(s)
    return (-s + b * torch.exp(-ma / b) + ma - 1).sum(-1)


class Net64(object):
    def __init__(self, sd, in_dim, out_dim, hidden):
        self.m = ts.StockGRURNN({k: np.asarray(v, np.float64) for k, v in sd.items()}, in_dim, out_dim, hidden).double()

    def __call__(self, x, y, h=None, clamp_lat=-1):
        out, y, h = self.m(x, y, h)
        return (clamp(out, clamp_lat) if clamp_lat >= 0 else out), y, h


def nets(P):
    return (Net64(P.enc, P.in_dim, 2 * P.lat_dim, P.hidden), Net64(P.dec, P.lat_dim + 2, P.out_dim, P.hidden))


def chain(P, eps, windows=None, n_cyc=None):
    """The eval chain; windows [(start, stop), ...]: every pass continues from its own state of the previous window.  Returns
    {key: [n_cyc, B, T, C] float64 numpy}."""
    enc, dec = nets(P)
    L, n = P.lat_dim, P.n_cyc if n_cyc is None else n_cyc
    X, CVX, CS, CT, E = t64(P.x), t64(P.cvx), t64(P.code_src), t64(P.code_trg), t64(eps)
    ye, yd = t64(P.y_in_enc), t64(P.y_in_dec)
    out = {k: [[] for _ in range(n)] for k in KEYS}
    state = {}

    def one(net, slot, i, xin, y0, cl):
        y, h = state.get((i, slot), (y0, None))
        o = net(xin, y, h, cl)
        state[(i, slot)] = (o[1], o[2])
        out[slot][i].append(o[0])
        return o[0]

    for a, b in (windows or [(0, P.T)]):
        x, cvx, cs, ct, e = X[:, a:b], CVX[:, a:b], CS[:, a:b], CT[:, a:b], E[:, :, :, a:b]
        prev = None
        for i in range(n):
            lat = one(enc, "lat", i, x if i == 0 else torch.cat((x[:, :, :P.stdim], prev), 2), ye, L)
            one(dec, "rec", i, torch.cat((cs, draw(lat, e[i, 0], L)), 2), yd, -1)
            cv = one(dec, "cv", i, torch.cat((ct, draw(lat, e[i, 1], L)), 2), yd, -1)
            latcv = one(enc, "latcv", i, torch.cat((cvx, cv), 2), ye, L)
            prev = one(dec, "reccyc", i, torch.cat((cs, draw(latcv, e[i, 2], L)), 2), yd, -1)
    return {k: np.stack([torch.cat(v, 1).numpy() for v in out[k]]) for k in KEYS}


def stage6(P, fs, ft, y_pp, y_src, y_trg, eps_src, eps_trg):
    """decode_gru-cyclevae_gauss.py:302-319 with the Laplace draw: (cvmcep, cvmcep_src, cvmcep_trg, lat_src, lat_trg) float64 numpy."""
    enc, dec = nets(P)
    L = P.lat_dim
    lat_s = enc(t64(fs)[None], t64(y_pp), None, L)[0]
    lat_t = enc(t64(ft)[None], t64(y_pp), None, L)[0]
    z_s = torch.mean(torch.stack([draw(lat_s, e[None], L) for e in t64(eps_src)]), 0)
    z_t = torch.mean(torch.stack([draw(lat_t, e[None], L) for e in t64(eps_trg)]), 0)
    code = lambda T, c: torch.eye(2, dtype=torch.float64)[c].expand(1, T, 2)
    Ts, Tt = fs.shape[0], ft.shape[0]
    cv = dec(torch.cat((code(Ts, 1), z_s), 2), t64(y_trg))[0]
    cv_s = dec(torch.cat((code(Ts, 0), z_s), 2), t64(y_src))[0]
    cv_t = dec(torch.cat((code(Tt, 1), z_t), 2), t64(y_trg))[0]
    return tuple(v[0].numpy() for v in (cv, cv_s, cv_t, lat_s, lat_t))


def loss_terms(trajs, x, stdim, L, flen_acc=None, select=None, half=False):
    """train...:1363-1410 with loss_vae_laplace for loss_vae, on float64 tensors."""
    B, T = x.shape[0], x.shape[1]
    sel = list(range(B)) if select is None else [int(j) for j in select]
    nfr = [T] * B if flen_acc is None else [min(int(n), T) for n in flen_acc]
    tot = 0.0
    for tr in trajs:
        kls, kl_cv = [], None
        for j in sel:
            n = nfr[j]
            tgt = x[j, :n, stdim:]
            mcd = lambda v: (K_MCD_L1 * (v[j, :n] - tgt).abs().sum(1)).mean() if n > 0 else 0.0
            tot = tot + mcd(tr["rec"])
            kls.append(kl(tr["lat"][j, :n], L).mean() if n > 0 else 0.0)
            if not half:
                tot = tot + mcd(tr["reccyc"])
                kl_cv = kl(tr["latcv"][j, :n], L).mean() if n > 0 else 0.0
        tot = tot + sum(kls)
        if not half and sel:
            # :1393: for more than one utterance the lat_src_cv list is rebuilt from the lat_src list + KL(latcv) of the last one
            tot = tot + (sum(kls) if len(sel) > 1 else 0.0) + kl_cv
    return tot


def step(P, eps, masks, flen_acc=None, select=None, n_cyc=2, lr=1e-4):
    """One stage-4 step in float64: train-mode chain (the reference's ten passes, supplied dropout masks and eps), loss, backward,
    Adam.  Returns (loss, {kind: {name: gradient}}, {kind: {name: weight after the step}}, number of log-scales on the floor)."""
    L = P.lat_dim
    leaf = {k: {n: t64(v).requires_grad_(n in ts_trainable()) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}
    X, CVX, CS, CT, E = t64(P.x), t64(P.cvx), t64(P.code_src), t64(P.code_trg), t64(eps)
    ye, yd = t64(P.y_in_enc), t64(P.y_in_dec)
    cnt = {"enc": 0, "dec": 0}

    def run(kind, xin, y, cl):
        cm, gm = masks[kind][cnt[kind]]
        cnt[kind] += 1
        h0 = torch.zeros(1, xin.shape[0], P.hidden, dtype=torch.float64)
        out = ts.train_forward_t(leaf[kind], xin, y, t64(cm), t64(gm), -1, h_in=h0)
        return clamp(out, cl) if cl >= 0 else out

    trajs, prev = [], None
    for i in range(n_cyc):
        lat = run("enc", X if i == 0 else torch.cat((X[:, :, :P.stdim], prev), 2), ye, L)
        rec = run("dec", torch.cat((CS, draw(lat, E[i, 0], L)), 2), yd, -1)
        cv = run("dec", torch.cat((CT, draw(lat, E[i, 1], L)), 2), yd, -1)
        latcv = run("enc", torch.cat((CVX, cv), 2), ye, L)
        prev = run("dec", torch.cat((CS, draw(latcv, E[i, 2], L)), 2), yd, -1)
        trajs.append({"lat": lat, "rec": rec, "cv": cv, "latcv": latcv, "reccyc": prev})
    loss = loss_terms(trajs, X, P.stdim, L, flen_acc, select)
    params = [p for k in ("enc", "dec") for p in leaf[k].values() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    opt.zero_grad()
    loss.backward()
    grads = {k: {n: p.grad.numpy().copy() for n, p in leaf[k].items() if p.requires_grad} for k in leaf}
    opt.step()
    after = {k: {n: p.detach().numpy().copy() for n, p in leaf[k].items() if p.requires_grad} for k in leaf}
    n_floor = sum(int((tr[k][..., L:] == FLOOR).sum()) for tr in trajs for k in ("lat", "latcv"))
    return float(loss.item()), grads, after, n_floor


def ts_trainable():
    import stage4
    return stage4.TRAINABLE
