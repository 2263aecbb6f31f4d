"""TEST INFRASTRUCTURE: CPU restatement of the reference's per-epoch validation pass, train_gru_cyclevae_gauss_batch.py:837-1139
(and the comparison of :1153), composed only of oracle.gru_rnn_forward, oracle.sampling_vae_batch, oracle.loss_vae,
oracle.twfse_loss, oracle.mcd_aligned, oracle.dtw_org_to_trg and numpy.  Line numbers below are that script's.

PARITY UNPINNED where it says so: dtw_c (dtw_org_to_trg, calc_mcd) is a third-party binary that is not in the reference tree, so
neither half can be recorded from the reference; the oracle's written definitions are the yardstick, as for the existing DTW
tests.  One deliberate difference: np.var of :888-893 runs in float32 on the fp32 trajectory; here, as in the library, the same
values are taken to float64 first.

A side (`src` / `trg`) is a dict of numpy arrays: feat [B,T,Cin], code_own, code_other [B,T,2], feat_par [B,Tp,Cin] (the parallel
utterance), cv [B,T,stdim], spcidx [B,S], spcidx_par [B,Sp] int64, flens, flens_par, flens_spc, flens_spc_par [B].
"""
import numpy as np

from oracle import cyclevae_oracle as orc

PASS_NAMES = ("lat_srctrg", "lat_trgsrc", "lat_trg", "lat_src", "trj_trg_trg", "trj_trg_src", "trj_src_src", "trj_src_trg",
              "lat_trg_src", "lat_src_trg", "trj_trg_src_trg", "trj_src_trg_src")
LOSS_TERMS = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_mcd_src_src", "loss_mcd_src_trg_src",
              "loss_mcd_src_trg", "loss_lat_trg", "loss_lat_trg_cv", "loss_lat_src", "loss_lat_src_cv")
DB_TERMS = ("mcdpow_trg_trg", "mcd_trg_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg", "mcdpow_trg_src", "mcd_trg_src",
            "mcdpow_src_src", "mcd_src_src", "mcdpow_src_trg_src", "mcd_src_trg_src", "mcdpow_src_trg", "mcd_src_trg")
DIST_TERMS = ("lat_dist_trgsrc1", "lat_dist_trgsrc2", "lat_dist_srctrg1", "lat_dist_srctrg2")
GV_TERMS = ("gv_trg_trg", "gv_trg_src_trg", "gv_trg_src", "gv_src_src", "gv_src_trg_src", "gv_src_trg")


def network_passes(enc, dec, src, trg, y_pp, y_src, y_trg, eps, lat_dim):
    """:837-838, :872-885 on the oracle network.  enc / dec: state dicts; y_*: [B,1,C]; eps: {draw name: [B,T,L]}."""
    L = lat_dim
    E = lambda x: orc.gru_rnn_forward(enc, x, y_pp, clamp_vae=True, lat_dim=L)[0]
    D = lambda code, lat, e, y: orc.gru_rnn_forward(dec, np.concatenate([code, orc.sampling_vae_batch(lat, e, L)], 2), y)[0]
    o = {}
    o["lat_srctrg"], o["lat_trgsrc"] = E(src["feat_par"]), E(trg["feat_par"])                       # :837-838
    o["lat_trg"], o["lat_src"] = E(trg["feat"]), E(src["feat"])                                     # :872-873
    o["trj_trg_trg"] = D(trg["code_own"], o["lat_trg"], eps["trg_trg"], y_trg)                      # :875
    o["trj_trg_src"] = D(trg["code_other"], o["lat_trg"], eps["trg_src"], y_src)                    # :876
    o["trj_src_src"] = D(src["code_own"], o["lat_src"], eps["src_src"], y_src)                      # :878
    o["trj_src_trg"] = D(src["code_other"], o["lat_src"], eps["src_trg"], y_trg)                    # :879
    o["lat_trg_src"] = E(np.concatenate([trg["cv"], o["trj_trg_src"]], 2))                          # :881
    o["lat_src_trg"] = E(np.concatenate([src["cv"], o["trj_src_trg"]], 2))                          # :882
    o["trj_trg_src_trg"] = D(trg["code_own"], o["lat_trg_src"], eps["trg_src_trg"], y_trg)          # :884
    o["trj_src_trg_src"] = D(src["code_own"], o["lat_src_trg"], eps["src_trg_src"], y_src)          # :885
    return o


def _calc_mcd(a, b):
    """dtw_c.calc_mcd(a, b)[0]: the mean mel-cd of two aligned f64 sequences.  PARITY UNPINNED (oracle.mcd_aligned)."""
    return orc.mcd_aligned(a, b, d0=0, L2=True)[1]


def utterance_metrics(src, trg, o, j, lat_dim, stdim):
    """:888-951 and :1006-1019 for utterance j of the batch from the pass outputs `o`.  Returns {name: value}."""
    L, sd = lat_dim, stdim
    f64 = lambda a: np.array(a, dtype=np.float64)
    fs, ft = int(src["flens"][j]), int(trg["flens"][j])
    ix_s, ix_t = src["spcidx"][j, :int(src["flens_spc"][j])], trg["spcidx"][j, :int(trg["flens_spc"][j])]
    ix_sp, ix_tp = src["spcidx_par"][j, :int(src["flens_spc_par"][j])], trg["spcidx_par"][j, :int(trg["flens_spc_par"][j])]
    r = {}
    # :888-893 (float64 here, float32 there)
    for g, t, n in (("gv_src_src", "trj_src_src", fs), ("gv_src_trg", "trj_src_trg", fs), ("gv_src_trg_src", "trj_src_trg_src", fs),
                    ("gv_trg_trg", "trj_trg_trg", ft), ("gv_trg_src", "trj_trg_src", ft), ("gv_trg_src_trg", "trj_trg_src_trg", ft)):
        r[g] = np.var(f64(o[t][j, :n, 1:]), axis=0)
    # :895-907 -- PARITY UNPINNED (oracle.dtw_org_to_trg)
    for side, lat_par, lat_own, ip, io in (("srctrg", "lat_srctrg", "lat_src", ix_sp, ix_s), ("trgsrc", "lat_trgsrc", "lat_trg", ix_tp, ix_t)):
        par, own = f64(o[lat_par][j][ip]), f64(o[lat_own][j][io])
        al1 = orc.dtw_org_to_trg(own, par)[0]                                                       # :897 / :914
        d1 = np.mean(np.sqrt(np.mean((al1 - par) ** 2, axis=0)))                                    # :898
        c1 = orc.dtw_org_to_trg(par, own, mcd=0)[2]                                                 # :899
        al2 = orc.dtw_org_to_trg(par, own)[0]                                                       # :900
        d2 = np.mean(np.sqrt(np.mean((al2 - own) ** 2, axis=0)))                                    # :901
        c2 = orc.dtw_org_to_trg(own, par, mcd=0)[2]                                                 # :902
        r["lat_dist_%s1" % side] = (d1 + d2) / 2                                                    # :904
        r["lat_dist_%s2" % side] = (c1 + c2) / 2                                                    # :906
    # :929-951 -- PARITY UNPINNED (oracle.mcd_aligned / oracle.dtw_org_to_trg)
    for a, b, ia, ib in (("trg", "src", ix_t, ix_tp), ("src", "trg", ix_s, ix_sp)):
        S = trg if a == "trg" else src
        spc_, spc__ = f64(S["feat"][j][:, sd:][ia]), f64(S["feat"][j][:, sd + 1:][ia])              # :929-930
        for n in ("%s_%s" % (a, a), "%s_%s_%s" % (a, b, a)):
            r["mcdpow_" + n] = _calc_mcd(spc_, f64(o["trj_" + n][j][ia]))                           # :932, :935
            r["mcd_" + n] = _calc_mcd(spc__, f64(o["trj_" + n][j][:, 1:][ia]))                      # :933, :936
        n = "%s_%s" % (a, b)
        r["mcdpow_" + n] = orc.dtw_org_to_trg(f64(o["trj_" + n][j][ia]), f64(S["feat_par"][j][:, sd:][ib]))[2]             # :938
        r["mcd_" + n] = orc.dtw_org_to_trg(f64(o["trj_" + n][j][:, 1:][ia]), f64(S["feat_par"][j][:, sd + 1:][ib]))[2]     # :939
    # :1006-1019 (fp32, as torch computes them)
    for n, S, nfr in (("trg_trg", trg, ft), ("trg_src", trg, ft), ("src_src", src, fs), ("src_trg", src, fs), ("trg_src_trg", trg, ft),
                      ("src_trg_src", src, fs)):
        r["loss_mcd_" + n] = orc.twfse_loss(o["trj_" + n][j, :nfr], S["feat"][j, :nfr, sd:], L2=False)[1]
    r["loss_lat_trg"], r["loss_lat_src"] = orc.loss_vae(o["lat_trg"][j, :ft], L), orc.loss_vae(o["lat_src"][j, :fs], L)
    r["loss_lat_trg_cv"], r["loss_lat_src_cv"] = orc.loss_vae(o["lat_trg_src"][j, :ft], L), orc.loss_vae(o["lat_src_trg"][j, :fs], L)
    return r


class RefValidation(object):
    """The epoch's lists and their reduction, :748-813 and :1102-1139."""

    def __init__(self, enc, dec, lat_dim, stdim, gv_src_mean, gv_trg_mean, half_cyc=False):
        self.enc, self.dec, self.lat_dim, self.stdim, self.half_cyc = enc, dec, lat_dim, stdim, half_cyc
        self.gv_src_mean, self.gv_trg_mean = np.asarray(gv_src_mean, np.float64), np.asarray(gv_trg_mean, np.float64)
        self.acc = {k: [] for k in ("loss",) + LOSS_TERMS + DB_TERMS + DIST_TERMS + GV_TERMS}

    def batch(self, src, trg, y_pp, y_src, y_trg, eps=None, trajectories=None):
        """trajectories: {PASS_NAMES: array}: the metric half runs on these arrays and no network pass is made."""
        o = trajectories if trajectories is not None else network_passes(self.enc, self.dec, src, trg, y_pp, y_src, y_trg, eps, self.lat_dim)
        B = src["feat"].shape[0]
        utts = [utterance_metrics(src, trg, o, j, self.lat_dim, self.stdim) for j in range(B)]
        out = {}
        for n in LOSS_TERMS:                                                                        # :1052-1077
            out[n] = float(np.mean(np.array([u[n] for u in utts], np.float32), dtype=np.float32))
            self.acc[n].append(out[n])
        for n in DB_TERMS + DIST_TERMS:                                                             # :988-1003, :905-979
            out[n] = float(np.mean([u[n] for u in utts]))
            self.acc[n] += [float(u[n]) for u in utts]
        for g in GV_TERMS:
            self.acc[g] += [u[g] for u in utts]
        terms = ("loss_mcd_trg_trg", "loss_mcd_src_src", "loss_lat_trg", "loss_lat_src")            # :1088
        if not self.half_cyc:                                                                       # :1086
            terms = ("loss_mcd_trg_trg", "loss_mcd_src_src", "loss_mcd_trg_src_trg", "loss_mcd_src_trg_src", "loss_lat_trg", "loss_lat_src",
                     "loss_lat_trg_cv", "loss_lat_src_cv")
        out["loss"] = float(sum(out[n] for n in terms))
        self.acc["loss"].append(out["loss"])                                                        # :1090
        return out, o

    def summary(self):
        s = {"eval_loss": float(np.mean(self.acc["loss"]))}                                         # :1102
        for n in LOSS_TERMS + DB_TERMS + DIST_TERMS:                                                # :1104-1139
            s["eval_" + n] = float(np.mean(self.acc[n]))
        for n in ("trg_src", "src_trg"):                                                            # :1122, :1124, :1135, :1137
            s["eval_mcdpowstd_" + n] = float(np.std(self.acc["mcdpow_" + n]))
            s["eval_mcdstd_" + n] = float(np.std(self.acc["mcd_" + n]))
        for g in GV_TERMS:                                                                          # :1114-1133
            ref = self.gv_trg_mean if g in ("gv_trg_trg", "gv_trg_src_trg", "gv_src_trg") else self.gv_src_mean
            s["eval_" + g] = float(np.mean(np.sqrt(np.square(np.log(np.mean(self.acc[g], axis=0)) - np.log(ref)))))
        return s


def better(summary, best):
    """:1153."""
    f = lambda s: s["eval_mcdpow_src_trg"] + s["eval_mcdpowstd_src_trg"] + s["eval_mcd_src_trg"] + s["eval_mcdstd_src_trg"]
    return best is None or f(summary) <= f(best)
