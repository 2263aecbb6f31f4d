"""TEST INFRASTRUCTURE: CPU restatement of the reference's stage 5, calc_cvgv_gru-cyclevae_gauss.py:179-283 and :320-344, composed
only of oracle.gru_rnn_forward, oracle.sampling_vae_batch, oracle.mcd_aligned, oracle.dtw_org_to_trg and numpy.  Line numbers below
are that script's.

PARITY UNPINNED where it says so: dtw_c (dtw_org_to_trg, calc_mcd) is a third-party binary that is not in the reference tree, so
neither half can be recorded from the reference; the oracle's written definitions are the yardstick, as in tests/validation_ref.py.

A pair's inputs: feat_src [Ts,Cin], feat_trg [Tt,Cin] fp32, spcidx_src [Ss], spcidx_trg [St'] int64, mcepspc_src [Ss,D],
mcepspc_trg [St,D] float64, eps_src [n,Ts,L], eps_trg [n,Tt,L] (the draws torch.randn makes inside sampling_vae_batch).
"""
import numpy as np

from oracle import cyclevae_oracle as orc

PASS_NAMES = ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg", "lat_feat", "lat_feat_trg")
GV_TERMS = ("cvgv", "cvgvsrc", "cvgvtrg")
MCD_TERMS = ("mcdpow_mean", "mcdpow_std", "mcd_mean", "mcd_std", "mcdpow_src_mean", "mcdpow_src_std", "mcd_src_mean", "mcd_src_std",
             "mcdpow_trg_mean", "mcdpow_trg_std", "mcd_trg_mean", "mcd_trg_std")
DIST_TERMS = ("lat_dist_rmse_enc", "lat_dist_cosim_enc", "lat_dist_rmse_pri", "lat_dist_cosim_pri")


def network_passes(enc, dec, feat_src, feat_trg, y_pp, y_src, y_trg, eps_src, eps_trg, lat_dim):
    """:179-199 on the oracle network.  enc / dec: state dicts; y_*: [1,1,C].  Returns a dict of PASS_NAMES (fp32)."""
    L = lat_dim
    o = {}
    o["lat_src"] = orc.gru_rnn_forward(enc, feat_src, y_pp, clamp_vae=True, lat_dim=L)[0]                            # :179
    n = eps_src.shape[0]
    o["lat_feat"] = orc.sampling_vae_batch(np.repeat(o["lat_src"][None], n, 0), eps_src, L).mean(0)                  # :180-181
    o["lat_trg"] = orc.gru_rnn_forward(enc, feat_trg, y_pp, clamp_vae=True, lat_dim=L)[0]                            # :182
    o["lat_feat_trg"] = orc.sampling_vae_batch(np.repeat(o["lat_trg"][None], n, 0), eps_trg, L).mean(0)              # :183-184
    code = lambda T, col: np.eye(2, dtype=np.float32)[col][None].repeat(T, 0)                                        # :185-193
    Ts, Tt = feat_src.shape[0], feat_trg.shape[0]
    o["cvmcep"] = orc.gru_rnn_forward(dec, np.concatenate([code(Ts, 1), o["lat_feat"]], 1), y_trg)[0]                # :194
    o["cvmcep_src"] = orc.gru_rnn_forward(dec, np.concatenate([code(Ts, 0), o["lat_feat"]], 1), y_src)[0]            # :196
    o["cvmcep_trg"] = orc.gru_rnn_forward(dec, np.concatenate([code(Tt, 1), o["lat_feat_trg"]], 1), y_trg)[0]        # :198
    return o


def pair_metrics(o, spcidx_src, spcidx_trg, mcep_src, mcep_trg):
    """:203-283 for one pair from the pass outputs `o` (dict of PASS_NAMES).  Returns {name: value}."""
    f64 = lambda a: np.array(a, dtype=np.float64)
    ix_s, ix_t = np.asarray(spcidx_src), np.asarray(spcidx_trg)
    cv, cv_src, cv_trg = f64(o["cvmcep"]), f64(o["cvmcep_src"]), f64(o["cvmcep_trg"])                                # :195, :197, :199
    mcep_src, mcep_trg = f64(mcep_src), f64(mcep_trg)
    r = {"cvgv": np.var(cv[:, 1:], axis=0), "cvgvsrc": np.var(cv_src[:, 1:], axis=0), "cvgvtrg": np.var(cv_trg[:, 1:], axis=0)}   # :203-205
    # :210-215 -- PARITY UNPINNED (oracle.dtw_org_to_trg)
    pow_arr = orc.dtw_org_to_trg(cv[ix_s, :], mcep_trg[:, :])[3]
    mcd_arr = orc.dtw_org_to_trg(cv[ix_s, 1:], mcep_trg[:, 1:])[3]
    r["mcdpow_mean"], r["mcdpow_std"], r["mcd_mean"], r["mcd_std"] = np.mean(pow_arr), np.std(pow_arr), np.mean(mcd_arr), np.std(mcd_arr)
    # :224-229, :238-243 -- PARITY UNPINNED (oracle.mcd_aligned: calc_mcd's frame array)
    for tag, mc, c, ix in (("_src", mcep_src, cv_src, ix_s), ("_trg", mcep_trg, cv_trg, ix_t)):
        pow_arr = orc.mcd_aligned(mc[:, :], c[ix, :], d0=0)[0]
        mcd_arr = orc.mcd_aligned(mc[:, 1:], c[ix, 1:], d0=0)[0]
        r["mcdpow%s_mean" % tag], r["mcdpow%s_std" % tag] = np.mean(pow_arr), np.std(pow_arr)
        r["mcd%s_mean" % tag], r["mcd%s_std" % tag] = np.mean(mcd_arr), np.std(mcd_arr)
    # :255-267 (enc: the encoder output, all 2L columns), :270-282 (pri: lat_feat) -- PARITY UNPINNED
    for tag, a, b in (("enc", "lat_src", "lat_trg"), ("pri", "lat_feat", "lat_feat_trg")):
        s, t = f64(o[a][ix_s]), f64(o[b][ix_t])
        d_st = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(s, t)[0] - t) ** 2, axis=0)))                            # :257-258
        c_st = orc.dtw_org_to_trg(t, s, mcd=0)[2]                                                                    # :259
        d_ts = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(t, s)[0] - s) ** 2, axis=0)))                            # :260-261
        c_ts = orc.dtw_org_to_trg(s, t, mcd=0)[2]                                                                    # :262
        r["lat_dist_rmse_" + tag], r["lat_dist_cosim_" + tag] = (d_st + d_ts) / 2, (c_st + c_ts) / 2                 # :264-265
    return {k: (v if k in GV_TERMS else float(v)) for k, v in r.items()}


class RefCvgv(object):
    """The script's lists and their reduction, :289-307 and :320-344."""

    def __init__(self, gv_mean_src, gv_mean_trg):
        self.gv_mean_src, self.gv_mean_trg = np.asarray(gv_mean_src, np.float64), np.asarray(gv_mean_trg, np.float64)
        self.acc = {k: [] for k in GV_TERMS + MCD_TERMS + DIST_TERMS}

    def add(self, r):
        for k in self.acc:
            self.acc[k].append(r[k])

    def summary(self):
        s = {}
        for g in GV_TERMS:                                                                                           # :320-325
            s[g + "_mean"], s[g + "_var"] = np.mean(np.array(self.acc[g]), axis=0), np.var(np.array(self.acc[g]), axis=0)
        for n in MCD_TERMS + DIST_TERMS:                                                                             # :329-344
            s[n], s[n + "_std"] = float(np.mean(np.array(self.acc[n]))), float(np.std(np.array(self.acc[n])))
        for tag, g, ref in (("", "cvgv", self.gv_mean_trg), ("_src", "cvgvsrc", self.gv_mean_src), ("_trg", "cvgvtrg", self.gv_mean_trg)):
            d = np.sqrt(np.square(np.log(s[g + "_mean"]) - np.log(ref)))                                             # :332, :336, :340
            s["gv_dist" + tag], s["gv_dist" + tag + "_std"] = float(np.mean(d)), float(np.std(d))
        return s
