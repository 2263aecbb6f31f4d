"""TEST INFRASTRUCTURE: the restatements of the metric passes (validation_ref, stage5_ref, trainlog_ref, uttlog_ref) with what the
reference adds for the Laplace posterior (src/nets/gru_vae.py:101-112, :130-139, :415-417):

    clamp    out[..., L:] >= FLOOR                                        (clamp_vae_laplace)
    draw     z = mu - exp(s) * sign(eps) * log1p(-2|eps|)                 (sampling_vae_laplace), eps ~ U(-0.4999, 0.5)
    KL       mean over frames of sum_l (-s + b exp(-|mu|/b) + |mu| - 1)   (loss_vae_laplace), b = exp(s)

Everything else is the existing restatement, called unchanged.  Two networks: the fp32 oracle (oracle.gru_rnn_forward with
clamp_vae_laplace, oracle.sampling_vae_laplace, oracle.loss_vae_laplace) is the reference; its float64 twin (laplace_chain_ref.Net64)
measures the reference's own rounding, for the bound rule of frontend_util.bound_for."""
import numpy as np

from oracle import cyclevae_oracle as orc
import laplace_chain_ref as lref
import stage5_ref as sref
import trainlog_ref as tref
import uttlog_ref as uref
import validation_ref as vref

FLOOR = lref.FLOOR
_window_record, _utterance_metrics = tref.window_record, vref.utterance_metrics      # (the Gaussian ones, whatever the names hold later)
f64 = lambda a: np.array(a, dtype=np.float64)


# ---- the KL in float64, and the size of what cancels in it ---------------------------------------------------------------------

def kl_frames(p, L):
    """[..., 2L] -> [...]: sum over the latent dimensions of -s + b exp(-|mu|/b) + |mu| - 1, float64 on the values given."""
    ma, s = np.abs(f64(p[..., :L])), f64(p[..., L:])
    b = np.exp(s)
    return np.sum(-s + b * np.exp(-ma / b) + ma - 1.0, -1)


def kl_condition(p, L):
    """[..., 2L] -> [...]: sum_l (|s| + b exp(-|mu|/b) + |mu| + 1), the summand's terms without their signs.  The terms of one
    summand cancel (mu = 0, s = 0 gives 0 + 1 + 0 - 1), so a relative bound on the KL is taken against this and not against the
    result alone."""
    ma, s = np.abs(f64(p[..., :L])), f64(p[..., L:])
    b = np.exp(s)
    return np.sum(np.abs(s) + b * np.exp(-ma / b) + ma + 1.0, -1)


def kl_mean(p, L):
    """(mean over the rows of the KL, mean over the rows of its condition) of a [rows, 2L] operand."""
    return float(np.mean(kl_frames(p, L))), float(np.mean(kl_condition(p, L)))


def lat_bound(lat, L, delta):
    """|difference| allowed on a mean Laplace KL when mu and s are within delta of the reference's: |d/dmu| <= 1 and
    |d/ds| = |-1 + b exp(-m/b) (1 + m/b)| <= 1 + b + b/e (x exp(-x) <= 1/e), so per frame L delta (2 + (1 + 1/e) exp(s_max + delta))."""
    return L * delta * (2.0 + (1.0 + np.exp(-1.0)) * np.exp(float(np.max(lat[..., L:])) + delta))


# ---- cvae_trainlog_window ------------------------------------------------------------------------------------------------------

def window_record(trajs, x_win, stdim, lat_dim, spcidx, select, flen_acc, s_idx, e_idx, src_idx_s):
    """trainlog_ref.window_record with entries [3], [4] the Laplace KL of lat, latcv.  Returns (record, scale): scale is the record
    with those two entries replaced by max(|KL|, mean condition) -- what 1e-12 is relative to."""
    R = _window_record(trajs, x_win, stdim, lat_dim, spcidx, select, flen_acc, s_idx, e_idx, src_idx_s)
    S = np.abs(R)
    T = x_win.shape[1]
    for i, tr in enumerate(trajs):
        for j in select:
            n = min(int(flen_acc[j]), T)
            if n > 0:
                for q, slot in ((3, "lat"), (4, "latcv")):
                    R[i, j, q], c = kl_mean(tr[slot][j, :n], lat_dim)
                    S[i, j, q] = max(abs(R[i, j, q]), c)
    return R, S


class _LaplaceRecords(object):
    """While entered, trainlog_ref.window_record is the Laplace one: RefTrainLog.after and RefUttLog.after call it by that name."""

    def __enter__(self):
        self.saved = tref.window_record
        tref.window_record = lambda *a: window_record(*a)[0]

    def __exit__(self, *exc):
        tref.window_record = self.saved


class RefTrainLog(tref.RefTrainLog):
    def after(self, *a, **k):
        with _LaplaceRecords():
            return tref.RefTrainLog.after(self, *a, **k)


class RefUttLog(uref.RefUttLog):
    def after(self, *a, **k):
        with _LaplaceRecords():
            return uref.RefUttLog.after(self, *a, **k)


# ---- validation ----------------------------------------------------------------------------------------------------------------

def _compose(E, D, cat, src, trg, y_pp, y_src, y_trg, eps):
    """validation_ref.network_passes' statements (:837-838, :872-885) over an encoder E(x), a decoder D(code, lat, eps, y)."""
    o = {}
    o["lat_srctrg"], o["lat_trgsrc"] = E(src["feat_par"]), E(trg["feat_par"])
    o["lat_trg"], o["lat_src"] = E(trg["feat"]), E(src["feat"])
    o["trj_trg_trg"] = D(trg["code_own"], o["lat_trg"], eps["trg_trg"], y_trg)
    o["trj_trg_src"] = D(trg["code_other"], o["lat_trg"], eps["trg_src"], y_src)
    o["trj_src_src"] = D(src["code_own"], o["lat_src"], eps["src_src"], y_src)
    o["trj_src_trg"] = D(src["code_other"], o["lat_src"], eps["src_trg"], y_trg)
    o["lat_trg_src"] = E(cat(trg["cv"], o["trj_trg_src"]))
    o["lat_src_trg"] = E(cat(src["cv"], o["trj_src_trg"]))
    o["trj_trg_src_trg"] = D(trg["code_own"], o["lat_trg_src"], eps["trg_src_trg"], y_trg)
    o["trj_src_trg_src"] = D(src["code_own"], o["lat_src_trg"], eps["src_trg_src"], y_src)
    return o


def validation_passes(P, src, trg, y_pp, y_src, y_trg, eps):
    """The twelve passes on the fp32 oracle network with the Laplace clamp and draw."""
    L = P.lat_dim
    E = lambda x: orc.gru_rnn_forward(P.enc, x, y_pp, clamp_vae_laplace=True, lat_dim=L)[0]
    D = lambda code, lat, e, y: orc.gru_rnn_forward(P.dec, np.concatenate([code, orc.sampling_vae_laplace(lat, e, L)], 2), y)[0]
    return _compose(E, D, lambda a, b: np.concatenate([a, b], 2), src, trg, y_pp, y_src, y_trg, eps)


def validation_passes64(P, src, trg, y_pp, y_src, y_trg, eps):
    """The same statements on the float64 twin (numpy float64 out)."""
    import torch
    enc, dec = lref.nets(P)
    L, t = P.lat_dim, lref.t64
    E = lambda x: enc(t(x) if not torch.is_tensor(x) else x, t(y_pp), None, L)[0]
    D = lambda code, lat, e, y: dec(torch.cat((t(code), lref.draw(lat, t(e), L)), 2), t(y))[0]
    o = _compose(E, D, lambda a, b: torch.cat((t(a), b), 2), src, trg, y_pp, y_src, y_trg, eps)
    return {k: v.numpy() for k, v in o.items()}


def utterance_metrics(src, trg, o, j, lat_dim, stdim):
    """validation_ref.utterance_metrics with the four loss_lat_* figures loss_vae_laplace's (fp32, as torch computes them)."""
    r = _utterance_metrics(src, trg, o, j, lat_dim, stdim)
    fs, ft = int(src["flens"][j]), int(trg["flens"][j])
    for n, t, nfr in (("loss_lat_trg", "lat_trg", ft), ("loss_lat_src", "lat_src", fs), ("loss_lat_trg_cv", "lat_trg_src", ft),
                      ("loss_lat_src_cv", "lat_src_trg", fs)):
        r[n] = orc.loss_vae_laplace(o[t][j, :nfr], lat_dim)
    return r


class RefValidation(vref.RefValidation):
    """validation_ref.RefValidation over the Laplace passes and figures; P: the problem (its weights are the network)."""

    def __init__(self, P, gv_src_mean, gv_trg_mean, half_cyc=False):
        vref.RefValidation.__init__(self, P.enc, P.dec, P.lat_dim, P.stdim, gv_src_mean, gv_trg_mean, half_cyc)
        self.P = P

    def batch(self, src, trg, y_pp, y_src, y_trg, eps=None, trajectories=None):
        o = trajectories if trajectories is not None else validation_passes(self.P, src, trg, y_pp, y_src, y_trg, eps)
        saved = vref.utterance_metrics
        vref.utterance_metrics = utterance_metrics      # (RefValidation.batch calls it by this name)
        try:
            return vref.RefValidation.batch(self, src, trg, None, None, None, trajectories=o)
        finally:
            vref.utterance_metrics = saved


# ---- stage 5 / stage 6 ---------------------------------------------------------------------------------------------------------

def pair_passes(P, feat_src, feat_trg, y_pp, y_src, y_trg, eps_src, eps_trg):
    """stage5_ref.network_passes (:179-199) on the fp32 oracle network with the Laplace clamp and draw."""
    L = P.lat_dim
    o = {}
    for lat, feat, z, e in (("lat_src", feat_src, "lat_feat", eps_src), ("lat_trg", feat_trg, "lat_feat_trg", eps_trg)):
        o[lat] = orc.gru_rnn_forward(P.enc, feat, y_pp, clamp_vae_laplace=True, lat_dim=L)[0]
        o[z] = orc.sampling_vae_laplace(np.repeat(o[lat][None], e.shape[0], 0), e, L).mean(0)
    code = lambda T, col: np.eye(2, dtype=np.float32)[col][None].repeat(T, 0)
    Ts, Tt = feat_src.shape[0], feat_trg.shape[0]
    o["cvmcep"] = orc.gru_rnn_forward(P.dec, np.concatenate([code(Ts, 1), o["lat_feat"]], 1), y_trg)[0]
    o["cvmcep_src"] = orc.gru_rnn_forward(P.dec, np.concatenate([code(Ts, 0), o["lat_feat"]], 1), y_src)[0]
    o["cvmcep_trg"] = orc.gru_rnn_forward(P.dec, np.concatenate([code(Tt, 1), o["lat_feat_trg"]], 1), y_trg)[0]
    return o


def pair_passes64(P, feat_src, feat_trg, y_pp, y_src, y_trg, eps_src, eps_trg):
    """The five trajectories of laplace_chain_ref.stage6 (float64) under stage5_ref's names."""
    out = lref.stage6(P, feat_src, feat_trg, y_pp, y_src, y_trg, eps_src, eps_trg)
    return dict(zip(("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg"), out))


pair_metrics = sref.pair_metrics      # (the metric half reads trajectories: it has no posterior)
