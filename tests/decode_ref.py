"""TEST INFRASTRUCTURE: CPU restatement of the reference's stage 6 between the network and the vocoder,
decode_gru-cyclevae_gauss.py:328-475 and :606-644, composed only of oracle.mc2e, oracle.mod_pow_dpow, oracle.gv_postfilter,
oracle.mcd_aligned, oracle.dtw_org_to_trg and numpy.  Line numbers below are that script's.  The network statements (:302-323) are
those of calc_cvgv...:179-199: tests/stage5_ref.py::network_passes.

PARITY UNPINNED where it says so: dtw_c (dtw_org_to_trg, calc_mcd) and pysptk (mc2e, inside mod_pow) are third-party binaries that
are not in the reference tree; the oracle's written definitions are the yardstick, as in tests/stage5_ref.py.

A pair's inputs: the pass outputs `o` (dict of PASS_NAMES, fp32), spcidx_src [Ss], spcidx_trg [St] int64, mcep [Ts,D], mcep_trg
[Tt,D] (the analysis' mel-cepstra, :259 and :272; mcepspc_trg of :278 is mcep_trg at spcidx_trg).
"""
import numpy as np

from oracle import cyclevae_oracle as orc
from stage5_ref import PASS_NAMES, DIST_TERMS, network_passes      # noqa: F401  (re-exported)

MCD_NAMES = ("mcdpow_cv", "mcd_cv", "mcdpow_src_cv", "mcd_src_cv", "mcdpow_trg_cv", "mcd_trg_cv", "mcd_cvgv", "mcd_src_cvgv", "mcd_trg_cvgv")
MCD_TERMS = tuple("%s_%s" % (n, k) for n in MCD_NAMES for k in ("mean", "std"))
GV_LISTS = (("cvlist", "trg"), ("cvgvlist", "trg"), ("cvlist_src", "src"), ("cvgvlist_src", "src"), ("cvlist_trg", "trg"), ("cvgvlist_trg", "trg"))
GV_TERMS = tuple(n for n, _ in GV_LISTS)
TRAJ_NAMES = ("cvmcep", "cvmcep_src", "cvmcep_trg", "cvmcep_gv", "cvmcep_src_gv", "cvmcep_trg_gv", "mc_cv_diff_nogv", "mc_cv_diff")


def mod_pow(cvmcep, mcep, alpha, irlen):
    """feature_extract_vc.py:131-138: only coefficient 0 moves.  PARITY UNPINNED (oracle.mc2e)."""
    out = np.array(cvmcep, dtype=np.float64)
    out[:, 0] += orc.mod_pow_dpow(cvmcep, mcep, alpha, irlen)
    return out


def pair_results(o, spcidx_src, spcidx_trg, mcep, mcep_trg, gv_mean_src, gv_mean_trg, cvgv_mean, cvgvsrc_mean, cvgvtrg_mean,
                 alpha=0.455, irlen=1024):
    """:328-475 for one pair.  Returns {name: value}: TRAJ_NAMES [T,D] f64, GV_TERMS [D-1], MCD_TERMS and DIST_TERMS floats."""
    f64 = lambda a: np.array(a, dtype=np.float64)
    ix_s, ix_t = np.asarray(spcidx_src), np.asarray(spcidx_trg)
    cvmcep, cvmcep_src, cvmcep_trg = f64(o["cvmcep"]), f64(o["cvmcep_src"]), f64(o["cvmcep_trg"])                    # :319-323
    mcep, mcep_trg = f64(mcep), f64(mcep_trg)
    mcepspc_trg = mcep_trg[ix_t]                                                                                     # :278
    r = {}
    # :332-360 -- PARITY UNPINNED (oracle.dtw_org_to_trg)
    for tag, a, b in (("enc", "lat_src", "lat_trg"), ("pri", "lat_feat", "lat_feat_trg")):
        s, t = f64(o[a][ix_s]), f64(o[b][ix_t])
        d_st = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(s, t)[0] - t) ** 2, axis=0)))                            # :334-335
        c_st = orc.dtw_org_to_trg(t, s, mcd=0)[2]                                                                    # :336
        d_ts = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(t, s)[0] - s) ** 2, axis=0)))                            # :337-338
        c_ts = orc.dtw_org_to_trg(s, t, mcd=0)[2]                                                                    # :339
        r["lat_dist_rmse_" + tag], r["lat_dist_cosim_" + tag] = (d_st + d_ts) / 2, (c_st + c_ts) / 2                 # :341-342

    def ms(name, arr):
        r[name + "_mean"], r[name + "_std"] = np.mean(arr), np.std(arr)
    ms("mcdpow_cv", orc.dtw_org_to_trg(cvmcep[ix_s, :], mcepspc_trg[:, :])[3])                                       # :363
    ms("mcd_cv", orc.dtw_org_to_trg(cvmcep[ix_s, 1:], mcepspc_trg[:, 1:])[3])                                        # :364
    r["cvlist"] = np.var(cvmcep[:, 1:], axis=0)                                                                      # :375
    ms("mcdpow_src_cv", orc.mcd_aligned(mcep[ix_s, :], cvmcep_src[ix_s, :], d0=0)[0])                                # :377
    ms("mcd_src_cv", orc.mcd_aligned(mcep[ix_s, 1:], cvmcep_src[ix_s, 1:], d0=0)[0])                                 # :378
    r["cvlist_src"] = np.var(cvmcep_src[:, 1:], axis=0)                                                              # :389
    ms("mcdpow_trg_cv", orc.mcd_aligned(mcepspc_trg[:, :], cvmcep_trg[ix_t, :], d0=0)[0])                            # :392
    ms("mcd_trg_cv", orc.mcd_aligned(mcepspc_trg[:, 1:], cvmcep_trg[ix_t, 1:], d0=0)[0])                             # :393
    r["cvlist_trg"] = np.var(cvmcep_trg[:, 1:], axis=0)                                                              # :404
    cvmcep = mod_pow(cvmcep, mcep, alpha, irlen)                                                                     # :407
    cvmcep_src = mod_pow(cvmcep_src, mcep, alpha, irlen)                                                             # :411
    cvmcep_trg = mod_pow(cvmcep_trg, mcep_trg, alpha, irlen)                                                         # :415
    cvmcep_gv, r["cvgvlist"] = orc.gv_postfilter(cvmcep, gv_mean_trg, cvgv_mean)                                     # :419-422
    ms("mcd_cvgv", orc.dtw_org_to_trg(cvmcep_gv[ix_s, 1:], mcepspc_trg[:, 1:])[3])                                   # :424
    cvmcep_gv = mod_pow(cvmcep_gv, mcep, alpha, irlen)                                                               # :432
    cvmcep_src_gv, r["cvgvlist_src"] = orc.gv_postfilter(cvmcep_src, gv_mean_src, cvgvsrc_mean)                      # :436-439
    ms("mcd_src_cvgv", orc.mcd_aligned(mcep[ix_s, 1:], cvmcep_src_gv[ix_s, 1:], d0=0)[0])                            # :441
    cvmcep_src_gv = mod_pow(cvmcep_src_gv, mcep, alpha, irlen)                                                       # :449
    cvmcep_trg_gv, r["cvgvlist_trg"] = orc.gv_postfilter(cvmcep_trg, gv_mean_trg, cvgvtrg_mean)                      # :453-456
    ms("mcd_trg_cvgv", orc.mcd_aligned(mcepspc_trg[:, 1:], cvmcep_trg_gv[ix_t, 1:], d0=0)[0])                        # :458
    cvmcep_trg_gv = mod_pow(cvmcep_trg_gv, mcep_trg, alpha, irlen)                                                   # :466
    r.update(cvmcep=cvmcep, cvmcep_src=cvmcep_src, cvmcep_trg=cvmcep_trg, cvmcep_gv=cvmcep_gv, cvmcep_src_gv=cvmcep_src_gv,
             cvmcep_trg_gv=cvmcep_trg_gv, mc_cv_diff_nogv=cvmcep - mcep, mc_cv_diff=cvmcep_gv - mcep)               # :470, :474
    return {k: (v if k in GV_TERMS + TRAJ_NAMES else float(v)) for k, v in r.items()}


class RefDecode(object):
    """The script's lists and what :606-644 log of them."""

    def __init__(self, gv_mean_src, gv_mean_trg):
        self.gv = {"src": np.asarray(gv_mean_src, np.float64), "trg": np.asarray(gv_mean_trg, np.float64)}
        self.acc = {k: [] for k in GV_TERMS + MCD_TERMS + DIST_TERMS}

    def add(self, r):
        for k in self.acc:
            self.acc[k].append(r[k])

    def summary(self):
        s = {}
        for n in MCD_TERMS + DIST_TERMS:
            s[n], s[n + "_std"] = float(np.mean(np.array(self.acc[n]))), float(np.std(np.array(self.acc[n])))
        for g, spk in GV_LISTS:
            s[g + "_mean"], s[g + "_var"] = np.mean(np.array(self.acc[g]), axis=0), np.var(np.array(self.acc[g]), axis=0)    # :608-609
            d = np.sqrt(np.square(np.log(s[g + "_mean"]) - np.log(self.gv[spk])))                                           # :611
            s["gv_dist_" + g], s["gv_dist_" + g + "_std"] = float(np.mean(d)), float(np.std(d))
        return s

    def log_lines(self):
        """:606-644, the arguments of the script's logging calls in its order."""
        a = lambda n: np.array(self.acc[n])
        four = lambda n: (np.mean(a(n + "_mean")), np.std(a(n + "_mean")), np.mean(a(n + "_std")), np.std(a(n + "_std")))

        def gvline(g, spk):
            cvgv_ev_mean = np.mean(a(g), axis=0)
            d = np.sqrt(np.square(np.log(cvgv_ev_mean) - np.log(self.gv[spk])))
            return "%lf +- %lf" % (np.mean(d), np.std(d))
        out = [
            "mcdpow_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcdpow_cv"),                    # :606
            "mcd_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_cv"),                          # :607
            gvline("cvlist", "trg"),                                                                  # :611
            "mcd_cvGV: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_cvgv"),                      # :612
            gvline("cvgvlist", "trg"),                                                                # :616
            "mcdpow_src_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcdpow_src_cv"),            # :618
            "mcd_src_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_src_cv"),                  # :619
            gvline("cvlist_src", "src"),                                                              # :623
            "mcd_src_cvGV: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_src_cvgv"),              # :624
            gvline("cvgvlist_src", "src"),                                                            # :628
            "mcdpow_trg_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcdpow_trg_cv"),            # :630
            "mcd_trg_cv: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_trg_cv"),                  # :631
            gvline("cvlist_trg", "trg"),                                                              # :635
            "mcd_trg_cvGV: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % four("mcd_trg_cvgv"),              # :636
            gvline("cvgvlist_trg", "trg"),                                                            # :640
        ]
        for n in DIST_TERMS:                                                                          # :641-644
            out.append("%s: %.6f (+- %.6f)" % (n, np.mean(a(n)), np.std(a(n))))
        return out
