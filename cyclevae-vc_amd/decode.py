"""Stage 6 of the recipe on the device: what decode_gru-cyclevae_gauss.py (line numbers below are that script's) does between the
network and the vocoder.  Per utterance pair the script copies three trajectories to the host and then, in float64 numpy and two
host libraries (dtw_c, pysptk): 8 latent alignments (:334-354), 3 mel-cepstrum alignments (:363-364, :424), 6 calc_mcd, 3 + 3 GV
variances, 6 mod_pow (8 distinct mc2e matrices), 3 GV post-filters and 2 differential cepstra (:470, :474); after the file loop it
logs the lists' means (:606-644).

Here a call takes up to ten pairs.  Network half (:302-323): stage5.CvgvPass.network_passes, unchanged -- the statements are those
of calc_cvgv...:179-199.  Metric half (:328-475), a metricplan.MetricPlan: one f64 arena and, whatever the number of pairs,
    cvae_eval_stats     GV variances of the raw trajectories, the packed f64 speech frames of the fp32 pass outputs
    cvae_mc2e_batch     round 1: mcep, mcep_trg and the three raw trajectories (5 matrices per pair)
    cvae_decode_jobs    mod_pow + GV post-filter + its variance (3 per pair), with cvmcep - mcep
    cvae_decode_jobs    the f64 speech-frame gathers: mcep, mcep_trg, the three post-filtered trajectories
    cvae_dtw_batch      11 alignments per pair
    cvae_mc2e_batch     round 2: the three post-filtered trajectories
    cvae_decode_jobs    their mod_pow in place (coefficient 0 only), with cvmcep_gv - mcep
    cvae_eval_stats     mean / std of the alignments' frame costs, calc_mcd's mean / std, the latent distances
and ONE D2H copy of the scalars.  Every figure of a pair is one block's fixed-order reduction (one wave's, for mc2e): it does not
depend on the call the pair lands in.  The arithmetic is the script's, not a shortened one: every mod_pow runs mc2e on the array it
is given (the energies of mcep / mcep_trg are computed once per pair -- the same bits), the post-filter reads the array AFTER
mod_pow, the alignment of :424 reads the post-filtered array BEFORE its own mod_pow.

PARITY UNPINNED for the DTW, calc_mcd and mc2e parts: dtw_c and pysptk are third-party binaries that are not in the reference tree;
the yardsticks are the written definitions in oracle/cyclevae_oracle.py (dtw_org_to_trg, mcd_aligned, mc2e), as for stage6.* and
stage5.CvgvPass.  Out of scope: the waveform analysis of :240-299 and the vocoder of :477-, the multi-device fan-out, file I/O.
"""
import ctypes as C

import numpy as np
import torch

import _cabi
import gru_vae
import stage5
from metricplan import MetricPlan

# the script's per-utterance figures: "<name>_mean" / "<name>_std" are what it appends to its two lists per name
MCD_NAMES = ("mcdpow_cv", "mcd_cv", "mcdpow_src_cv", "mcd_src_cv", "mcdpow_trg_cv", "mcd_trg_cv", "mcd_cvgv", "mcd_src_cvgv", "mcd_trg_cvgv")
MCD_TERMS = tuple("%s_%s" % (n, k) for n in MCD_NAMES for k in ("mean", "std"))
DIST_TERMS = stage5.DIST_TERMS
# the script's six GV lists (:375, :389, :404, :422, :439, :456) with the speaker whose GV statistic :611-640 compares them to
GV_LISTS = (("cvlist", "trg"), ("cvgvlist", "trg"), ("cvlist_src", "src"), ("cvgvlist_src", "src"), ("cvlist_trg", "trg"), ("cvgvlist_trg", "trg"))
GV_TERMS = tuple(n for n, _ in GV_LISTS)
TRAJ_NAMES = ("cvmcep", "cvmcep_src", "cvmcep_trg", "cvmcep_gv", "cvmcep_src_gv", "cvmcep_trg_gv", "mc_cv_diff_nogv", "mc_cv_diff")
PASS_NAMES = stage5.PASS_NAMES
MAX_PAIRS = stage5.MAX_PAIRS
PROFILE_PARTS = ("stats", "dtw", "mc2e_1", "mc2e_2", "modpow")


class DecodePass(object):
    """DecodePass(model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, cvgv_mean, cvgvsrc_mean, cvgvtrg_mean,
    n_smpl_dec=300, mcep_alpha=0.455, irlen=1024, posterior="gauss"): call pairs() on the evaluation pairs, ten at a time at most,
    then summary() / log_lines().  gv_mean_*: "/gv_range_mean"[1:] of the two speakers (:186-187); cvgv*_mean: the three vectors of
    :205-210, which stage5.CvgvPass.write produces.  posterior: handed to the stage5.CvgvPass that runs the network half ("laplace":
    the Laplace clamp and draws); it has to be the posterior the model was trained with, which cannot be detected here."""

    def __init__(self, model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, cvgv_mean, cvgvsrc_mean, cvgvtrg_mean,
                 n_smpl_dec=300, mcep_alpha=0.455, irlen=1024, posterior="gauss"):
        self.net = stage5.CvgvPass(model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, n_smpl_dec=n_smpl_dec,
                                   posterior=posterior)
        self.posterior = posterior
        self.enc, self.dec, self.lat_dim, self.n_smpl_dec = model_encoder, model_decoder, int(lat_dim), int(n_smpl_dec)
        self.D = int(model_decoder.out_dim)
        self.mcep_alpha, self.irlen = float(mcep_alpha), int(irlen)
        if not 2 <= self.irlen <= 4000:
            raise ValueError("irlen must be 2 .. 4000 (cvae_mc2e_batch), got %d" % self.irlen)
        if self.D < 2:
            raise ValueError("the decoder must give at least 2 coefficients, got %d" % self.D)
        self.stat = {}
        for name, v in (("gv_mean_src", gv_mean_src), ("gv_mean_trg", gv_mean_trg), ("cvgv_mean", cvgv_mean), ("cvgvsrc_mean", cvgvsrc_mean),
                        ("cvgvtrg_mean", cvgvtrg_mean)):
            a = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
            if a.shape[0] != self.D - 1:
                raise ValueError("%s has %d entries, expected D - 1 = %d" % (name, a.shape[0], self.D - 1))
            self.stat[name] = a
        self.gv_mean_src, self.gv_mean_trg = self.stat["gv_mean_src"], self.stat["gv_mean_trg"]
        self._dev_stat = {}
        self.reset()

    def reset(self):
        self.last_passes = None
        self.acc = {k: [] for k in GV_TERMS + MCD_TERMS + DIST_TERMS}

    def _stat_on(self, dev):
        """the five statistics vectors as one f64 device tensor [5, D-1], uploaded once per device"""
        key = str(dev)
        if key not in self._dev_stat:
            names = ("gv_mean_src", "gv_mean_trg", "cvgv_mean", "cvgvsrc_mean", "cvgvtrg_mean")
            t = torch.from_numpy(np.stack([self.stat[n] for n in names])).to(dev)
            self._dev_stat[key] = {n: t[k] for k, n in enumerate(names)}
        return self._dev_stat[key]

    def _check_items(self, items):
        """Everything about a call's items that can be refused from their shapes, before anything is launched.  Returns per pair
        (mcep_src, mcep_trg): [T, D] float32 / float64 tensors with unit column stride (views of feat when the item has none)."""
        if not 1 <= len(items) <= MAX_PAIRS:
            raise ValueError("1..%d utterance pairs per call, got %d" % (MAX_PAIRS, len(items)))
        D, out = self.D, []
        for q, it in enumerate(items):
            if len(it) not in (4, 6):
                raise ValueError("pair %d: an item is (feat_src, feat_trg, spcidx_src, spcidx_trg[, mcep_src, mcep_trg])" % q)
            mc = []
            for side, feat, m in (("src", it[0], it[4] if len(it) == 6 else None), ("trg", it[1], it[5] if len(it) == 6 else None)):
                if feat.dim() != 2 or feat.shape[0] < 1 or feat.shape[1] < D:
                    raise ValueError("pair %d: feat_%s has shape %s" % (q, side, tuple(feat.shape)))
                if m is None:
                    m = feat[:, feat.shape[1] - D:]
                if tuple(m.shape) != (feat.shape[0], D):
                    raise ValueError("pair %d: mcep_%s has shape %s, expected %s" % (q, side, tuple(m.shape), (feat.shape[0], D)))
                if m.dtype not in (torch.float32, torch.float64):
                    m = m.to(torch.float64)
                if m.stride(1) != 1 or m.stride(0) < D:
                    m = m.contiguous()
                mc.append(m.to(feat.device))
            for side, ix in (("src", it[2]), ("trg", it[3])):
                if ix.numel() < 1:
                    raise ValueError("pair %d: empty speech-frame index list (%s)" % (q, side))
            out.append(tuple(mc))
        return out

    # ---- :328-475 ---------------------------------------------------------------------------------------------------------------
    def metrics(self, items, passes, profile=None):
        """Per-pair results from the pass outputs (list of dicts of PASS_NAMES).  Returns a list of dicts: TRAJ_NAMES -> [T, D]
        float64 device tensors (views of the call's arena), GV_TERMS -> [D-1] float64 numpy, MCD_TERMS and DIST_TERMS -> float.
        A speech-frame index outside its utterance makes the MCD_TERMS and DIST_TERMS of THAT pair NaN (the library gathers NaN rows
        instead of reading there); the trajectories and GV vectors do not read the index lists and stay.
        profile: a dict that receives the device milliseconds of PROFILE_PARTS and the counts "frames_1", "frames_2" (frames of the
        two mc2e rounds), "problems", "jobs"."""
        lib, st = gru_vae._lib(), gru_vae._stream()
        L, D = self.lat_dim, self.D
        if len(items) != len(passes):
            raise ValueError("%d items and %d pass outputs" % (len(items), len(passes)))
        mceps = self._check_items(items)
        gru_vae._need_cuda(passes[0]["cvmcep"], "DecodePass.metrics(cvmcep)")
        dev = passes[0]["cvmcep"].device
        plan = MetricPlan(dev, profile is not None)
        S = self._stat_on(dev)
        is64 = lambda t: int(t.dtype == torch.float64)

        # DecodeJob / Mc2eJob fields; the arena regions among them (Refs) become addresses behind plan.finalise()
        def modpow(c, c_f64, T, e_ref, e_c, x, ref=None, diff=None, gv=None, cvgv=None, g=None, var=None):
            rp, rf, rl = (ref.data_ptr(), is64(ref), ref.stride(0)) if ref is not None else (None, 0, 0)
            return (_cabi.DEC_MODPOW, T, D, c_f64, rf, 0, 0, 0, c, D, e_ref, e_c, gv, cvgv, x, g, var, None, rp, rl, diff, None)

        def gather(src, src_f64, ld, src_rows, ix, dst):
            return (_cabi.DEC_GATHER, dst.rows, D, src_f64, 0, src_rows, 0, D, src, ld, None, None, None, None, dst, None, None, None, None, 0,
                    None, ix.data_ptr())
        mcjob = lambda t, e: (t.data_ptr(), is64(t), t.shape[0], D, 0, t.stride(0), e)
        mc1, mc2, dA, dG, dB, out = [], [], [], [], [], []
        for q, (it, p, (mc_s, mc_t)) in enumerate(zip(items, passes, mceps)):
            p, ix_s, ix_t, ta, tb = stage5.pair_inputs(plan, q, it, p, L, D)
            if mc_s.shape[0] != ta or mc_t.shape[0] != tb:
                raise ValueError("pair %d: mcep of %d / %d frames beside trajectories of %d / %d" % (q, mc_s.shape[0], mc_t.shape[0], ta, tb))
            plan.hold((mc_s, mc_t))
            # :375, :389, :404; :332-354, :363, :377, :392 -- the speech frames of the pass outputs as packed f64 matrices
            o = stage5.pair_operands(plan, p, ix_s, ix_t, ("cvlist", "cvlist_src", "cvlist_trg"), MCD_NAMES)
            g, ns, nt = o["g"], ix_s.numel(), ix_t.numel()
            gv, ms = o["gv"], o["ms"]
            gv.update((n, plan.vec(D - 1)) for n in ("cvgvlist", "cvgvlist_src", "cvgvlist_trg"))
            E = {n: plan.mat(1, tb if "trg" in n else ta) for n in ("mcep", "mcep_trg") + TRAJ_NAMES[:6]}      # mc2e's energies
            X = o["trj"] = {n: plan.mat(tb if "trg" in n else ta, D) for n in TRAJ_NAMES}
            # :407-415 -- mod_pow of the three trajectories; :419-422, :436-439, :453-456 -- the post-filter of its result
            mc1 += [mcjob(mc_s, E["mcep"]), mcjob(mc_t, E["mcep_trg"])]
            for k, ref, er, T, gm, cg in (("cvmcep", mc_s, "mcep", ta, "gv_mean_trg", "cvgv_mean"),
                                          ("cvmcep_src", mc_s, "mcep", ta, "gv_mean_src", "cvgvsrc_mean"),
                                          ("cvmcep_trg", mc_t, "mcep_trg", tb, "gv_mean_trg", "cvgvtrg_mean")):
                kg, first = k + "_gv", k == "cvmcep"
                mc1.append(mcjob(p[k], E[k]))
                dA.append(modpow(p[k].data_ptr(), 0, T, E[er], E[k], X[k], ref=ref if first else None,
                                 diff=X["mc_cv_diff_nogv"] if first else None,                                   # :470
                                 gv=S[gm].data_ptr(), cvgv=S[cg].data_ptr(), g=X[kg], var=gv[k.replace("cvmcep", "cvgvlist")]))
                # :432, :449, :466 -- mod_pow of the post-filtered array, in place
                mc2.append((X[kg], 1, T, D, 0, D, E[kg]))
                dB.append(modpow(X[kg], 1, T, E[er], E[kg], X[kg], ref=ref if first else None,
                                 diff=X["mc_cv_diff"] if first else None))                                       # :474
            # :377 mcep[spcidx_src], :278 mcepspc_trg, :424 / :441 / :458 the post-filtered arrays at the speech frames
            mcspc_s, mcspc_t = plan.mat(ns, D), plan.mat(nt, D)
            gg = {k: plan.mat(nt if "trg" in k else ns, D) for k in ("cvmcep", "cvmcep_src", "cvmcep_trg")}
            dG += [gather(mc_s.data_ptr(), is64(mc_s), mc_s.stride(0), ta, ix_s, mcspc_s),
                   gather(mc_t.data_ptr(), is64(mc_t), mc_t.stride(0), tb, ix_t, mcspc_t)]
            dG += [gather(X[k + "_gv"], 1, D, tb if "trg" in k else ta, ix_t if "trg" in k else ix_s, gg[k]) for k in gg]
            # :363-368, :424-426 -- the three mel-cepstrum alignments; mean and np.std of their frame costs
            for n, org, c0 in (("mcdpow_cv", g["cvmcep"], 0), ("mcd_cv", g["cvmcep"], 1), ("mcd_cvgv", gg["cvmcep"], 1)):
                frames = plan.align(org, mcspc_t, -1, c0=c0)
                plan.stat(2, _cabi.STAT_MEANSTD64, nt, 0, 1, frames, 1, out=ms[n], src_rows=nt)
            # :377-378, :392-393, :441, :458 -- calc_mcd(mcep at the speech frames, reconstruction at the speech frames)
            for n, mc, r, c0 in (("mcdpow_src_cv", mcspc_s, g["cvmcep_src"], 0), ("mcd_src_cv", mcspc_s, g["cvmcep_src"], 1),
                                 ("mcdpow_trg_cv", mcspc_t, g["cvmcep_trg"], 0), ("mcd_trg_cv", mcspc_t, g["cvmcep_trg"], 1),
                                 ("mcd_src_cvgv", mcspc_s, gg["cvmcep_src"], 1), ("mcd_trg_cvgv", mcspc_t, gg["cvmcep_trg"], 1)):
                plan.stat(2, _cabi.STAT_MCD64, r.rows, c0, D, mc, D, r, D, out=ms[n], src_rows=r.rows)
            out.append(o)
        dtw_bytes = plan.dtw_work_bytes()
        mc_bytes = lib.mc2e_batch_work_bytes(len(mc1), D, self.irlen)
        if mc_bytes == 0:
            raise _cabi.CvaeError("cvae_mc2e_batch_work_bytes: bad arguments (D=%d, irlen=%d)" % (D, self.irlen))
        dj = C.sizeof(_cabi.DecodeJob)
        up = lambda v: (v + 255) // 256 * 256
        parts = [dtw_bytes, mc_bytes, len(dA) * dj, len(dG) * dj, len(dB) * dj]
        offs = np.concatenate([[0], np.cumsum([up(v) for v in parts])])
        work = plan.hold(torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev))
        W = lambda k: work.data_ptr() + int(offs[k])
        plan.finalise(work=W(0))
        mc1, mc2 = ([_cabi.Mc2eJob(*plan.resolve(f)) for f in jobs] for jobs in (mc1, mc2))
        dA, dG, dB = ([_cabi.DecodeJob(*plan.resolve(f)) for f in jobs] for jobs in (dA, dG, dB))
        plan.begin()
        plan.stats(1)
        lib.mc2e_batch(mc1, self.mcep_alpha, self.irlen, W(1), mc_bytes, st)
        plan.mark("mc2e_1")
        lib.decode_jobs(dA, W(2), parts[2], st)
        lib.decode_jobs(dG, W(3), parts[3], st)
        plan.mark("modpow")
        plan.dtw()
        lib.mc2e_batch(mc2, self.mcep_alpha, self.irlen, W(1), mc_bytes, st)
        plan.mark("mc2e_2")
        lib.decode_jobs(dB, W(4), parts[4], st)
        plan.mark("modpow")
        plan.stats(2)
        host = plan.results().cpu().numpy()          # the ONE D2H copy (waits for the stream)
        if profile is not None:
            t = plan.times()
            profile.update(stats=t["stats1"] + t["stats2"], mc2e_1=t["mc2e_1"], modpow=t["modpow"], dtw=t["dtw"], mc2e_2=t["mc2e_2"],
                           frames_1=sum(j.T for j in mc1), frames_2=sum(j.T for j in mc2), problems=len(plan.probs),
                           jobs=len(plan.table) + len(dA) + len(dG) + len(dB))
        gru_vae.check_status()
        res = []
        for o in out:
            r = {n: plan.view(x) for n, x in o["trj"].items()}
            r.update(stage5.pair_figures(host, o, MCD_TERMS, ("mcdpow_src_cv", "mcdpow_trg_cv")))
            res.append(r)
        return res

    def pairs(self, items, y_in_pp, y_in_src, y_in_trg, eps=None, seed=None, first_pair_id=0):
        """One call of at most ten pairs.  items: tuples (feat_src [Ts,Cin], feat_trg [Tt,Cin], spcidx_src, spcidx_trg[, mcep_src
        [Ts,D], mcep_trg [Tt,D]]) of device tensors; mcep_*: float64 or float32, the analysis' mel-cepstrum (:259, :272) -- without
        them the last D columns of feat_* are used (the same numbers in float32).  eps, seed, first_pair_id: as in
        stage5.CvgvPass.pairs.  Returns the per-pair dicts (metrics()) and appends their figures to the pass's lists; last_passes
        holds the five fp32 trajectories and two latent means per pair."""
        items = list(items)
        self._check_items(items)
        self.last_passes = self.net.network_passes(items, y_in_pp, y_in_src, y_in_trg, eps, seed, first_pair_id)
        res = self.metrics(items, self.last_passes)
        for r in res:
            for k in GV_TERMS + MCD_TERMS + DIST_TERMS:
                self.acc[k].append(r[k])
        return res

    # ---- :606-644 ---------------------------------------------------------------------------------------------------------------
    def summary(self):
        """Every figure of :606-644.  "<name>_mean", "<name>_mean_std", "<name>_std", "<name>_std_std" for the nine MCD_NAMES: np.mean
        and np.std over the pairs of the per-pair means and of the per-pair standard deviations; "<list>_mean" / "<list>_var": the
        cvgv_ev_mean / cvgv_ev_var of the six GV lists, "gv_dist_<list>" / "gv_dist_<list>_std" their log-GV distances; DIST_TERMS
        with "_std"."""
        if not self.acc["cvlist"]:
            raise RuntimeError("DecodePass.summary(): no pair seen")
        s = {}
        for n in MCD_TERMS + DIST_TERMS:
            v = np.array(self.acc[n])
            s[n], s[n + "_std"] = float(np.mean(v)), float(np.std(v))
        for g, spk in GV_LISTS:
            v = np.array(self.acc[g])
            s[g + "_mean"], s[g + "_var"] = np.mean(v, axis=0), np.var(v, axis=0)
            d = np.sqrt(np.square(np.log(s[g + "_mean"]) - np.log(self.stat["gv_mean_" + spk])))
            s["gv_dist_" + g], s["gv_dist_" + g + "_std"] = float(np.mean(d)), float(np.std(d))
        return s

    def log_lines(self):
        """The text of :606-644, one string per logging call, in the script's order."""
        s = self.summary()
        mcd = lambda n, label: "%s: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % (label, s[n + "_mean"], s[n + "_mean_std"], s[n + "_std"],
                                                                           s[n + "_std_std"])
        gv = lambda g: "%f +- %f" % (s["gv_dist_" + g], s["gv_dist_" + g + "_std"])
        out = []
        for tag in ("", "_src", "_trg"):
            out += [mcd("mcdpow%s_cv" % tag, "mcdpow%s_cv" % tag), mcd("mcd%s_cv" % tag, "mcd%s_cv" % tag), gv("cvlist" + tag),
                    mcd("mcd%s_cvgv" % tag, "mcd%s_cvGV" % tag), gv("cvgvlist" + tag)]
        for n in DIST_TERMS:
            out.append("%s: %.6f (+- %.6f)" % (n, s[n], s[n + "_std"]))
        return out
