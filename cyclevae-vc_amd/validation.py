"""The per-epoch validation pass of stage-4 training on the device (reference train_gru_cyclevae_gauss_batch.py:741-1139, and
the comparison of :1153 that decides which checkpoint is kept).

The reference runs twelve network passes per evaluation batch and then, per utterance, copies about thirty slices to the host
and calls the host library dtw_c twelve times.  Here the passes are the eval passes of gru_vae.GRU_RNN, and everything behind
them is three launches and one copy: cvae_eval_stats (GV variances, speech-frame MCDs, the ten loss terms' per-utterance values
and the packed f64 DTW operands), cvae_dtw_batch (twelve alignments per utterance pair, one block each), cvae_eval_stats again
(the latent distances of the aligned sequences), and ONE D2H copy of the result vector.

PARITY UNPINNED for the DTW and calc_mcd halves: dtw_c is a third-party binary that is not in the reference tree; the yardstick
is the written definition at oracle/cyclevae_oracle.py::dtw_org_to_trg / mcd_aligned, as for stage6.dtw_org_to_trg.  The GV
variances are taken in float64 from the fp32 trajectories (the reference's np.var runs in float32 on the same values).
"""
import numpy as np
import torch

import _cabi
import gru_vae
import stage4
from metricplan import MetricPlan, batch_rows, ints, row

N_EV_CYC = 1      # train...:604

# the per-batch / per-epoch quantities under the reference's names (:988-1090, :1102-1139)
LOSS_TERMS = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_mcd_src_src", "loss_mcd_src_trg_src",
              "loss_mcd_src_trg", "loss_lat_trg", "loss_lat_trg_cv", "loss_lat_src", "loss_lat_src_cv")
DB_TERMS = ("mcdpow_trg_trg", "mcd_trg_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg", "mcdpow_trg_src", "mcd_trg_src",
            "mcdpow_src_src", "mcd_src_src", "mcdpow_src_trg_src", "mcd_src_trg_src", "mcdpow_src_trg", "mcd_src_trg")
DIST_TERMS = ("lat_dist_trgsrc1", "lat_dist_trgsrc2", "lat_dist_srctrg1", "lat_dist_srctrg2")
GV_TERMS = ("gv_trg_trg", "gv_trg_src_trg", "gv_trg_src", "gv_src_src", "gv_src_trg_src", "gv_src_trg")
# eps (tests): the six draws of :875-885 in the order they are made
DRAWS = ("trg_trg", "trg_src", "src_src", "src_trg", "trg_src_trg", "src_trg_src")
# what network_passes returns, [B, T, C] fp32 each
PASS_NAMES = ("lat_srctrg", "lat_trgsrc", "lat_trg", "lat_src", "trj_trg_trg", "trj_trg_src", "trj_src_src", "trj_src_trg",
              "lat_trg_src", "lat_src_trg", "trj_trg_src_trg", "trj_src_trg_src")


def _side(items):
    """One evaluation generator's yield (loader.train_generator(batch_size=0): 16 fields) as a dict."""
    if isinstance(items, dict):
        return items
    (feat, code_own, code_other, feat_par, cv, _c, _i, spc, spc_par, _f, _fp, flens, flens_par, flens_spc, flens_spc_par, n_utt) = items
    return {"feat": feat, "code_own": code_own, "code_other": code_other, "feat_par": feat_par, "cv": cv, "spcidx": spc,
            "spcidx_par": spc_par, "flens": flens, "flens_par": flens_par, "flens_spc": flens_spc, "flens_spc_par": flens_spc_par,
            "n_utt": n_utt}


class ValidationPass(object):
    """ValidationPass(model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, half_cyc=False, posterior="gauss"):
    call batch() on every pair of yields of the two evaluation generators, then summary(); better() is the checkpoint decision.
    posterior="laplace": the Laplace posterior of the sibling recipes (reference gru_vae.py:101-112, :130-139, :415-417) -- the six
    encoder passes clamp as clamp_vae_laplace does, the draws are sampling_vae_laplace's (injected eps are then its uniforms in
    (-0.4999, 0.5)) and the four loss_lat_* figures are loss_vae_laplace's KL (CVAE_STAT_KL_LAPLACE).  It has to be the posterior the
    model was trained with (stage4.Stage4Step(posterior=)): a disagreement cannot be detected here and is the caller's mistake."""

    def __init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, half_cyc=False, posterior="gauss"):
        self._laplace = stage4._check_posterior(posterior)      # (ValueError for anything but "gauss" / "laplace")
        self.posterior = posterior
        self.enc, self.dec, self.lat_dim, self.stdim, self.half_cyc = model_encoder, model_decoder, int(lat_dim), int(stdim), bool(half_cyc)
        self.gv_src_mean = np.asarray(gv_src_mean, np.float64)
        self.gv_trg_mean = np.asarray(gv_trg_mean, np.float64)
        self.reset()

    def reset(self):
        """Forget the batches seen so far (the reference empties its lists after every epoch, :1202-)."""
        self.last_passes = None
        self.acc = {k: [] for k in ("loss",) + LOSS_TERMS + DB_TERMS + DIST_TERMS + GV_TERMS}

    # ---- the twelve passes of :837-885 ------------------------------------------------------------------------------------------
    def network_passes(self, src, trg, y_in_pp, y_in_src, y_in_trg, eps=None):
        """The passes in eval mode through the module calls; same-length inputs of the two sides go as rows of one call.  Returns a
        dict of PASS_NAMES.  Model modes and requires_grad flags are restored on exit."""
        enc, dec, L = self.enc, self.dec, self.lat_dim
        mods = (enc, dec)
        was = [(m.training, [p.requires_grad for p in m.parameters()]) for m in mods]
        try:
            for m in mods:                                   # :741-746
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False
            with torch.no_grad():
                return self._passes(src, trg, y_in_pp, y_in_src, y_in_trg, eps)
        finally:
            for m, (tr, rg) in zip(mods, was):
                m.train(tr)
                for p, r in zip(m.parameters(), rg):
                    p.requires_grad = r

    def _passes(self, src, trg, y_pp, y_src, y_trg, eps):
        enc, dec, L, sd = self.enc, self.dec, self.lat_dim, self.stdim
        f = lambda t: t.to(torch.float32)
        laplace = self._laplace

        def run(mod, xs, ys, clamp):
            """mod over a list of [B, T, C] inputs: inputs of one length go as rows of one call (rows are independent recurrences)."""
            outs = [None] * len(xs)
            kw = {"clamp_vae_laplace": clamp} if laplace else {"clamp_vae": clamp}
            for T in sorted({x.shape[1] for x in xs}):
                ids = [i for i, x in enumerate(xs) if x.shape[1] == T]
                if len(ids) == 1:
                    outs[ids[0]] = mod(xs[ids[0]], ys[ids[0]], lat_dim=L, **kw)[0]
                    continue
                out = mod(torch.cat([xs[i] for i in ids], 0), torch.cat([ys[i] for i in ids], 0), lat_dim=L, **kw)[0]
                for i, part in zip(ids, torch.split(out, [xs[i].shape[0] for i in ids], 0)):
                    outs[i] = part
            return outs

        def draw(lat, name):
            if laplace:      # rows flattened to [B T, 2L]; eps: the reference's uniforms, through its eps= argument
                e = None if eps is None else f(eps[name]).reshape(-1, L)
                return gru_vae.sampling_vae_laplace(lat.reshape(-1, 2 * L), lat_dim=L, eps=e).reshape(lat.shape[0], lat.shape[1], L)
            if eps is None:
                return gru_vae.sampling_vae_batch(lat, lat_dim=L)
            return gru_vae.sampling_with_eps(lat, f(eps[name]), lat_dim=L)

        B = src["feat"].shape[0]
        ypp, ys, yt = batch_rows(y_pp, B), batch_rows(y_src, B), batch_rows(y_trg, B)
        o = {}
        o["lat_srctrg"], o["lat_trgsrc"], o["lat_trg"], o["lat_src"] = run(
            enc, [f(src["feat_par"]), f(trg["feat_par"]), f(trg["feat"]), f(src["feat"])], [ypp] * 4, True)      # :837-838, :872-873
        cat = lambda a, b: torch.cat((f(a), b), 2)
        o["trj_trg_trg"], o["trj_trg_src"], o["trj_src_src"], o["trj_src_trg"] = run(                                # :875-879
            dec, [cat(trg["code_own"], draw(o["lat_trg"], "trg_trg")), cat(trg["code_other"], draw(o["lat_trg"], "trg_src")),
                  cat(src["code_own"], draw(o["lat_src"], "src_src")), cat(src["code_other"], draw(o["lat_src"], "src_trg"))],
            [yt, ys, ys, yt], False)
        o["lat_trg_src"], o["lat_src_trg"] = run(enc, [cat(trg["cv"], o["trj_trg_src"]), cat(src["cv"], o["trj_src_trg"])],   # :881-882
                                                 [ypp] * 2, True)
        o["trj_trg_src_trg"], o["trj_src_trg_src"] = run(                                                            # :884-885
            dec, [cat(trg["code_own"], draw(o["lat_trg_src"], "trg_src_trg")), cat(src["code_own"], draw(o["lat_src_trg"], "src_trg_src"))],
            [yt, ys], False)
        return {k: v.contiguous() for k, v in o.items()}

    # ---- the metric half of :887-1019 -------------------------------------------------------------------------------------------
    def metrics(self, src, trg, passes, profile=None):
        """Per-utterance figures of one batch from the pass outputs (dict of PASS_NAMES, fp32 device tensors): three launches and one
        D2H copy.  Returns {name: [B] float64 numpy} for LOSS_TERMS, DB_TERMS, DIST_TERMS and {gv name: [B, D-1]}.
        profile: a dict that receives the device milliseconds of "stats", "dtw" and "latdist" (events around the three calls;
        tools/validation_timing.py) and the counts "jobs", "problems", "work_bytes"."""
        L, sd = self.lat_dim, self.stdim
        dev = passes["lat_src"].device
        plan = MetricPlan(dev, profile is not None)
        f32 = lambda t: plan.hold(t.to(torch.float32).contiguous())
        P = {k: f32(v) for k, v in passes.items()}
        feat = {"src": f32(src["feat"]), "trg": f32(trg["feat"]), "src_par": f32(src["feat_par"]), "trg_par": f32(trg["feat_par"])}
        spc = {"src": src["spcidx"], "trg": trg["spcidx"], "src_par": src["spcidx_par"], "trg_par": trg["spcidx_par"]}
        spc = {k: plan.hold(v.to(device=dev, dtype=torch.int64).contiguous()) for k, v in spc.items()}
        flen = {"src": ints(src["flens"]), "trg": ints(trg["flens"])}
        nspc = {"src": ints(src["flens_spc"]), "trg": ints(trg["flens_spc"]), "src_par": ints(src["flens_spc_par"]),
                "trg_par": ints(trg["flens_spc_par"])}
        B, Cin = feat["src"].shape[0], feat["src"].shape[2]
        Co = Cin - sd
        for s in ("src", "trg"):
            if len(flen[s]) != B or feat[s].shape[0] != B or feat[s + "_par"].shape[0] != B or feat[s].shape[2] != Cin or feat[s + "_par"].shape[2] != Cin:
                raise ValueError("the %s side does not hold %d utterances of %d features" % (s, B, Cin))
            if max(flen[s]) > feat[s].shape[1] or min(flen[s]) < 1:
                raise ValueError("flens of the %s side %s do not fit %d frames" % (s, flen[s], feat[s].shape[1]))
        for k in PASS_NAMES:      # the kernels address these by the sides' shapes: a pass output of another shape must not reach them
            side = {"lat_srctrg": "src_par", "lat_trgsrc": "trg_par"}.get(k) or k.split("_")[1]
            want = (B, feat[side].shape[1], 2 * L if k.startswith("lat") else Co)
            if tuple(P[k].shape) != want:
                raise ValueError("pass output %s has shape %s, expected %s" % (k, tuple(P[k].shape), want))
        for s in spc:
            if spc[s].shape[0] != B or len(nspc[s]) != B:
                raise ValueError("speech-frame indices of %s: %d rows for %d utterances" % (s, spc[s].shape[0], B))
            if max(nspc[s]) > spc[s].shape[1] or min(nspc[s]) < 1:
                raise ValueError("flens_spc of %s %s do not fit %d speech-frame indices" % (s, nspc[s], spc[s].shape[1]))

        # per utterance: result regions, jobs and alignments, declared together
        idx_of = lambda side, j: spc[side].data_ptr() + 8 * j * spc[side].shape[1]
        stat, out = plan.stat, []
        for j in range(B):
            fs, ft, o, g = flen["src"][j], flen["trg"][j], {}, {}
            # :888-893
            for n, t, nfr in (("gv_src_src", "trj_src_src", fs), ("gv_src_trg", "trj_src_trg", fs), ("gv_src_trg_src", "trj_src_trg_src", fs),
                              ("gv_trg_trg", "trj_trg_trg", ft), ("gv_trg_src", "trj_trg_src", ft), ("gv_trg_src_trg", "trj_trg_src_trg", ft)):
                a, lda = row(P[t], j)
                o[n] = plan.vec(Co - 1)
                stat(1, _cabi.STAT_GV, nfr, 1, Co, a, lda, out=o[n])
            # :929-948 calc_mcd on the speech frames, with and without the power coefficient
            for side, names in (("trg", ("trg_trg", "trg_src_trg")), ("src", ("src_src", "src_trg_src"))):
                fa, lfa = row(feat[side], j, sd)
                for n in names:
                    b, ldb = row(P["trj_" + n], j)
                    for pre, c0 in (("mcdpow_", 0), ("mcd_", 1)):
                        o[pre + n] = plan.vec()
                        stat(1, _cabi.STAT_MCD_SPC, nspc[side][j], c0, Co, fa, lfa, b, ldb, idx_of(side, j), out=o[pre + n],
                             src_rows=feat[side].shape[1])
            # :1006-1013 (the trg_src / src_trg conversions are held against the utterance's OWN features, as the script does)
            for n, side, nfr in (("trg_trg", "trg", ft), ("trg_src", "trg", ft), ("src_src", "src", fs), ("src_trg", "src", fs),
                                 ("trg_src_trg", "trg", ft), ("src_trg_src", "src", fs)):
                a, lda = row(P["trj_" + n], j)
                b, ldb = row(feat[side], j, sd)
                o["loss_mcd_" + n] = plan.vec()
                stat(1, _cabi.STAT_MCD_L1, nfr, 0, Co, a, lda, b, ldb, out=o["loss_mcd_" + n])
            # :1015-1019
            for n, t, nfr in (("loss_lat_trg", "lat_trg", ft), ("loss_lat_src", "lat_src", fs), ("loss_lat_trg_cv", "lat_trg_src", ft),
                              ("loss_lat_src_cv", "lat_src_trg", fs)):
                a, lda = row(P[t], j)
                o[n] = plan.vec()
                stat(1, _cabi.STAT_KL_LAPLACE if self._laplace else _cabi.STAT_KL, nfr, 0, L, a, lda, out=o[n])
            # :895-896, :912-913, :938-939, :950-951: the f64 DTW operands
            for key, t, side, col, c1 in (("lat_srctrg", P["lat_srctrg"], "src_par", 0, 2 * L), ("lat_src", P["lat_src"], "src", 0, 2 * L),
                                          ("lat_trgsrc", P["lat_trgsrc"], "trg_par", 0, 2 * L), ("lat_trg", P["lat_trg"], "trg", 0, 2 * L),
                                          ("trj_trg_src", P["trj_trg_src"], "trg", 0, Co), ("feat_trg_par", feat["trg_par"], "trg_par", sd, Co),
                                          ("trj_src_trg", P["trj_src_trg"], "src", 0, Co), ("feat_src_par", feat["src_par"], "src_par", sd, Co)):
                a, lda = row(t, j, col)
                g[key] = plan.mat(nspc[side][j], c1)
                stat(1, _cabi.STAT_GATHER64, g[key].rows, 0, c1, a, lda, idx=idx_of(side, j), dst=g[key], src_rows=t.shape[1])
            # :897-906, :914-923
            o["srctrg"] = plan.latent_distance(g["lat_src"], g["lat_srctrg"])
            o["trgsrc"] = plan.latent_distance(g["lat_trg"], g["lat_trgsrc"])
            # :938-939, :950-951 -- the converted trajectory against the parallel utterance, with and without coefficient 0
            for n, org, par in (("trg_src", "trj_trg_src", "feat_trg_par"), ("src_trg", "trj_src_trg", "feat_src_par")):
                for pre, c0 in (("mcdpow_", 0), ("mcd_", 1)):
                    o[pre + n] = plan.vec()
                    plan.align(g[org], g[par], -1, None, o[pre + n], c0=c0)
            out.append(o)
        plan.finalise()
        plan.begin()
        plan.stats(1)
        plan.dtw()
        plan.stats(2)
        host = plan.results().cpu().numpy()          # the ONE D2H copy (waits for the stream)
        if profile is not None:
            ms = plan.times()
            profile.update(stats=ms["stats1"], dtw=ms["dtw"], latdist=ms["stats2"], jobs=len(plan.table), problems=len(plan.probs),
                           work_bytes=int(plan.work_bytes))
        gru_vae.check_status()
        res = {}
        for n in LOSS_TERMS + DB_TERMS:
            res[n] = np.array([host[o[n].off] for o in out])
        for n in GV_TERMS:
            res[n] = np.stack([o[n].of(host) for o in out])
        for n in ("srctrg", "trgsrc"):               # :904-906, :921-923
            rmse_a, rmse_b, cos_a, cos_b = (np.array([host[o[n][k].off] for o in out]) for k in range(4))
            res["lat_dist_%s1" % n], res["lat_dist_%s2" % n] = (rmse_a + rmse_b) / 2, (cos_a + cos_b) / 2
        return res

    def batch(self, src_items, trg_items, y_in_pp, y_in_src, y_in_trg, eps=None):
        """One evaluation batch: src_items / trg_items are what the two evaluation generators yield (the 16 fields of
        loader.train_generator(batch_size=0), or a dict of feat, code_own, code_other, feat_par, cv, spcidx, spcidx_par, flens,
        flens_par, flens_spc, flens_spc_par).  eps: None (on-device draws) or {name of DRAWS: [B, T, lat_dim]}.
        Returns the per-batch dictionary of :988-1090: "loss", the ten batch_loss_* terms, the twelve dB figures and the four latent
        distances, as floats under the names of LOSS_TERMS / DB_TERMS / DIST_TERMS."""
        src, trg = _side(src_items), _side(trg_items)
        gru_vae._need_cuda(src["feat"], "ValidationPass.batch(features)")
        gru_vae.check_status()
        self.last_passes = self.network_passes(src, trg, y_in_pp, y_in_src, y_in_trg, eps)      # (kept: the trajectories of the latest batch)
        return self.accumulate(self.metrics(src, trg, self.last_passes))

    def accumulate(self, per_utt):
        """Per-utterance figures of one batch -> its dictionary, and into the epoch's lists."""
        out = {}
        for n in LOSS_TERMS:                                 # :1052-1077 (torch.mean over the batch's utterances)
            out[n] = float(np.mean(per_utt[n]))
            self.acc[n].append(out[n])
        for n in DB_TERMS + DIST_TERMS:                      # :988-1003; the epoch keeps the per-utterance values (:967-979, :905-924)
            out[n] = float(np.mean(per_utt[n]))
            self.acc[n] += [float(v) for v in per_utt[n]]
        for g in GV_TERMS:
            self.acc[g] += [v for v in per_utt[g]]
        terms = ("loss_mcd_trg_trg", "loss_mcd_src_src", "loss_lat_trg", "loss_lat_src")          # :1085-1088
        if not self.half_cyc:
            terms = ("loss_mcd_trg_trg", "loss_mcd_src_src", "loss_mcd_trg_src_trg", "loss_mcd_src_trg_src", "loss_lat_trg", "loss_lat_src",
                     "loss_lat_trg_cv", "loss_lat_src_cv")
        out["loss"] = float(sum(out[n] for n in terms))
        self.acc["loss"].append(out["loss"])
        return out

    def summary(self):
        """The eval_* quantities of :1102-1139 under the reference's names (n_ev_cyc = 1: scalars, not lists)."""
        if not self.acc["loss"]:
            raise RuntimeError("ValidationPass.summary(): no batch seen")
        s = {"eval_loss": float(np.mean(self.acc["loss"]))}
        for n in LOSS_TERMS + DB_TERMS + DIST_TERMS:
            s["eval_" + n] = float(np.mean(self.acc[n]))
        for n in ("trg_src", "src_trg"):
            s["eval_mcdpowstd_" + n] = float(np.std(self.acc["mcdpow_" + n]))
            s["eval_mcdstd_" + n] = float(np.std(self.acc["mcd_" + n]))
        for g in GV_TERMS:               # a conversion INTO a speaker is held against that speaker's GV statistics
            ref = self.gv_trg_mean if g in ("gv_trg_trg", "gv_trg_src_trg", "gv_src_trg") else self.gv_src_mean
            s["eval_" + g] = float(np.mean(np.sqrt(np.square(np.log(np.mean(self.acc[g], axis=0)) - np.log(ref)))))
        return s

    @staticmethod
    def score(summary):
        """:1153's figure of merit."""
        return summary["eval_mcdpow_src_trg"] + summary["eval_mcdpowstd_src_trg"] + summary["eval_mcd_src_trg"] + summary["eval_mcdstd_src_trg"]

    @classmethod
    def better(cls, summary, best):
        """True when `summary` replaces `best` as the kept checkpoint (:1153: "<=" on the sum of the src->trg mcdpow, mcd and
        their standard deviations); best None: the first epoch."""
        return best is None or cls.score(summary) <= cls.score(best)

    @staticmethod
    def log_line(s):
        """The "average evaluation loss" text of :1140-1151."""
        return ("%.3f ;; [1] %.3f %.3f %.3f %.3f %.3f %.3f ; %.3f %.3f %.3f %.3f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
                "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
                "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ;; " % tuple(
                    [s["eval_loss"]] + [s["eval_" + n] for n in LOSS_TERMS] + [s["eval_" + n] for n in (
                        "gv_trg_trg", "mcdpow_trg_trg", "mcd_trg_trg", "gv_trg_src_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg", "gv_trg_src",
                        "mcdpow_trg_src", "mcdpowstd_trg_src", "mcd_trg_src", "mcdstd_trg_src", "lat_dist_trgsrc1", "lat_dist_trgsrc2",
                        "gv_src_src", "mcdpow_src_src", "mcd_src_src", "gv_src_trg_src", "mcdpow_src_trg_src", "mcd_src_trg_src", "gv_src_trg",
                        "mcdpow_src_trg", "mcdpowstd_src_trg", "mcd_src_trg", "mcdstd_src_trg", "lat_dist_srctrg1", "lat_dist_srctrg2")]))
