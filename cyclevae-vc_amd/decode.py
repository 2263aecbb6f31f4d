"""Stage 6 of the recipe on the device: what decode_gru-cyclevae_gauss.py (line numbers below are that script's) does between the
network and the vocoder.  Per utterance pair the script copies three trajectories to the host and then, in float64 numpy and two
host libraries (dtw_c, pysptk): 8 latent alignments (:334-354), 3 mel-cepstrum alignments (:363-364, :424), 6 calc_mcd, 3 + 3 GV
variances, 6 mod_pow (8 distinct mc2e matrices), 3 GV post-filters and 2 differential cepstra (:470, :474); after the file loop it
logs the lists' means (:606-644).

Here a call takes up to ten pairs.  Network half (:302-323): stage5.CvgvPass.network_passes, unchanged -- the statements are those
of calc_cvgv...:179-199.  Metric half (:328-475), as in stage5.CvgvPass.metrics: one f64 arena and, whatever the number of pairs,
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
    n_smpl_dec=300, mcep_alpha=0.455, irlen=1024): call pairs() on the evaluation pairs, ten at a time at most, then summary() /
    log_lines().  gv_mean_*: "/gv_range_mean"[1:] of the two speakers (:186-187); cvgv*_mean: the three vectors of :205-210, which
    stage5.CvgvPass.write produces."""

    def __init__(self, model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, cvgv_mean, cvgvsrc_mean, cvgvtrg_mean,
                 n_smpl_dec=300, mcep_alpha=0.455, irlen=1024):
        self.net = stage5.CvgvPass(model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, n_smpl_dec=n_smpl_dec)
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
        f32 = lambda t: t.to(torch.float32).contiguous()
        i64 = lambda t: t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        P = [{k: f32(p[k]) for k in PASS_NAMES} for p in passes]
        S = self._stat_on(dev)
        cursor = [0]

        def take(k):
            at = cursor[0]
            cursor[0] += int(k)
            return at
        lay = []
        for q, (it, p, (mc_s, mc_t)) in enumerate(zip(items, P, mceps)):
            ix_s, ix_t = i64(it[2]), i64(it[3])
            ta, tb, ns, nt = p["cvmcep"].shape[0], p["cvmcep_trg"].shape[0], ix_s.numel(), ix_t.numel()
            want = {"cvmcep": (ta, D), "cvmcep_src": (ta, D), "cvmcep_trg": (tb, D), "lat_src": (ta, 2 * L), "lat_trg": (tb, 2 * L),
                    "lat_feat": (ta, L), "lat_feat_trg": (tb, L)}
            for k, shape in want.items():      # the kernels address these by the shapes: another shape must not reach them
                if tuple(p[k].shape) != shape:
                    raise ValueError("pair %d: pass output %s has shape %s, expected %s" % (q, k, tuple(p[k].shape), shape))
            if mc_s.shape[0] != ta or mc_t.shape[0] != tb:
                raise ValueError("pair %d: mcep of %d / %d frames beside trajectories of %d / %d" % (q, mc_s.shape[0], mc_t.shape[0], ta, tb))
            e = {"ix_s": ix_s, "ix_t": ix_t, "mc_s": mc_s, "mc_t": mc_t, "ta": ta, "tb": tb, "ns": ns, "nt": nt}
            e["gv"] = {n: take(D - 1) for n in GV_TERMS}
            e["ms"] = {n: take(2) for n in MCD_NAMES}
            e["ld"] = {n: take(1) for n in ("enc_rmse_a", "enc_cos_a", "enc_rmse_b", "enc_cos_b", "pri_rmse_a", "pri_cos_a", "pri_rmse_b",
                                            "pri_cos_b")}
            e["junk"] = [take(1) for _ in range(7)]      # (mean costs of the mel-cd alignments: MEANSTD64 gives the means that are read)
            lay.append(e)
        n_out = cursor[0]
        twf_len = 0
        for e in lay:
            ta, tb, ns, nt = e["ta"], e["tb"], e["ns"], e["nt"]
            mat = lambda rows, cols: (take(rows * cols), rows, cols)
            e["g_cv"], e["g_cvsrc"], e["g_cvtrg"] = mat(ns, D), mat(ns, D), mat(nt, D)
            e["g_enc_s"], e["g_enc_t"], e["g_pri_s"], e["g_pri_t"] = mat(ns, 2 * L), mat(nt, 2 * L), mat(ns, L), mat(nt, L)
            e["al_enc_st"], e["al_enc_ts"], e["al_pri_st"], e["al_pri_ts"] = mat(nt, 2 * L), mat(ns, 2 * L), mat(nt, L), mat(ns, L)
            e["mcspc_s"], e["mcspc_t"] = mat(ns, D), mat(nt, D)                      # mcep[spcidx_src], mcepspc_trg (:278)
            e["gg_cv"], e["gg_cvsrc"], e["gg_cvtrg"] = mat(ns, D), mat(ns, D), mat(nt, D)      # the post-filtered arrays' speech frames
            t2s = [nt, nt, nt, ns, ns, nt, nt, ns, ns, nt, nt]      # T2 of the eleven alignments
            e["frames"] = [take(t) for t in t2s]
            e["twf"] = []
            for t in t2s:
                e["twf"].append(twf_len)
                twf_len += t
            e["e"] = {"mcep": take(ta), "mcep_trg": take(tb), "cvmcep": take(ta), "cvmcep_src": take(ta), "cvmcep_trg": take(tb),
                      "cvmcep_gv": take(ta), "cvmcep_src_gv": take(ta), "cvmcep_trg_gv": take(tb)}
            e["trj"] = {n: take((tb if "trg" in n else ta) * D) for n in TRAJ_NAMES}
        arena = torch.empty(cursor[0], dtype=torch.float64, device=dev)
        twf = torch.empty(twf_len, dtype=torch.int64, device=dev)
        a0, w0 = arena.data_ptr(), twf.data_ptr()
        A = lambda off: a0 + 8 * off

        def job(kind, rows, c0, c1, a, lda, b=None, ldb=0, idx=None, dst=None, out_off=0, src_rows=0):
            return _cabi.StatJob(kind, rows, c0, c1, src_rows, 0, a, b, lda, ldb, idx, dst, out_off)

        def modpow(c, c_f64, ldc, T, e_ref, e_c, x, ref=None, diff=None, gv=None, cvgv=None, g=None, var=None):
            rp, rf, rl = (ref.data_ptr(), int(ref.dtype == torch.float64), ref.stride(0)) if ref is not None else (None, 0, 0)
            return _cabi.DecodeJob(_cabi.DEC_MODPOW, T, D, c_f64, rf, 0, 0, 0, c, ldc, A(e_ref), A(e_c), gv, cvgv, A(x),
                                   None if g is None else A(g), None if var is None else A(var), None, rp, rl,
                                   None if diff is None else A(diff), None)

        def gather(src, src_f64, ld, src_rows, ix, dst):
            return _cabi.DecodeJob(_cabi.DEC_GATHER, dst[1], D, src_f64, 0, src_rows, 0, D, src, ld, None, None, None, None, A(dst[0]), None,
                                   None, None, None, 0, None, ix.data_ptr())
        mcjob = lambda t, e_off: _cabi.Mc2eJob(t.data_ptr(), int(t.dtype == torch.float64), t.shape[0], D, 0, t.stride(0), A(e_off))
        mcjob64 = lambda off, T, e_off: _cabi.Mc2eJob(A(off), 1, T, D, 0, D, A(e_off))
        jobs1, jobs2, probs, mc1, mc2, dA, dG, dB = [], [], [], [], [], [], [], []
        for e, p in zip(lay, P):
            ns, nt, ta, tb, E, X = e["ns"], e["nt"], e["ta"], e["tb"], e["e"], e["trj"]
            # :375, :389, :404
            for n, k in (("cvlist", "cvmcep"), ("cvlist_src", "cvmcep_src"), ("cvlist_trg", "cvmcep_trg")):
                jobs1.append(job(_cabi.STAT_GV, p[k].shape[0], 1, D, p[k].data_ptr(), D, out_off=e["gv"][n]))
            # :332-333, :347-348, :363, :377, :392 -- the speech frames of the pass outputs as packed f64 matrices
            for key, k, ix in (("g_cv", "cvmcep", "ix_s"), ("g_cvsrc", "cvmcep_src", "ix_s"), ("g_cvtrg", "cvmcep_trg", "ix_t"),
                               ("g_enc_s", "lat_src", "ix_s"), ("g_enc_t", "lat_trg", "ix_t"), ("g_pri_s", "lat_feat", "ix_s"),
                               ("g_pri_t", "lat_feat_trg", "ix_t")):
                off, r, c = e[key]
                jobs1.append(job(_cabi.STAT_GATHER64, r, 0, c, p[k].data_ptr(), c, idx=e[ix].data_ptr(), dst=A(off), src_rows=p[k].shape[0]))
            # :407-415 -- mod_pow of the three trajectories; :419-422, :436-439, :453-456 -- the post-filter of its result
            mc1 += [mcjob(e["mc_s"], E["mcep"]), mcjob(e["mc_t"], E["mcep_trg"])]
            for k, ref, er, T, gv, cg in (("cvmcep", e["mc_s"], "mcep", ta, "gv_mean_trg", "cvgv_mean"),
                                          ("cvmcep_src", e["mc_s"], "mcep", ta, "gv_mean_src", "cvgvsrc_mean"),
                                          ("cvmcep_trg", e["mc_t"], "mcep_trg", tb, "gv_mean_trg", "cvgvtrg_mean")):
                kg, first = k + "_gv", k == "cvmcep"
                mc1.append(mcjob(p[k], E[k]))
                dA.append(modpow(p[k].data_ptr(), 0, D, T, E[er], E[k], X[k], ref=ref if first else None,
                                 diff=X["mc_cv_diff_nogv"] if first else None,                                   # :470
                                 gv=S[gv].data_ptr(), cvgv=S[cg].data_ptr(), g=X[kg], var=e["gv"][k.replace("cvmcep", "cvgvlist")]))
                # :432, :449, :466 -- mod_pow of the post-filtered array, in place
                mc2.append(mcjob64(X[kg], T, E[kg]))
                dB.append(modpow(A(X[kg]), 1, D, T, E[er], E[kg], X[kg], ref=ref if first else None,
                                 diff=X["mc_cv_diff"] if first else None))                                       # :474
            # :377 mcep[spcidx_src], :278 mcepspc_trg, :424 / :441 / :458 the post-filtered arrays at the speech frames
            f64 = lambda t: int(t.dtype == torch.float64)
            dG += [gather(e["mc_s"].data_ptr(), f64(e["mc_s"]), e["mc_s"].stride(0), ta, e["ix_s"], e["mcspc_s"]),
                   gather(e["mc_t"].data_ptr(), f64(e["mc_t"]), e["mc_t"].stride(0), tb, e["ix_t"], e["mcspc_t"]),
                   gather(A(X["cvmcep_gv"]), 1, D, ta, e["ix_s"], e["gg_cv"]),
                   gather(A(X["cvmcep_src_gv"]), 1, D, ta, e["ix_s"], e["gg_cvsrc"]),
                   gather(A(X["cvmcep_trg_gv"]), 1, D, tb, e["ix_t"], e["gg_cvtrg"])]

            def prob(org, trg_, k, mcd, aligned=None, mean=None, c0=0):
                """org / trg_: (address, rows, columns) of packed f64 matrices; c0: the first compared column"""
                (oa, r1, c), (ta_, r2, _) = org, trg_
                return _cabi.DtwProblem(oa + 8 * c0, ta_ + 8 * c0, c, c, r1, r2, c - c0, mcd, None if aligned is None else A(aligned[0]),
                                        w0 + 8 * e["twf"][k], A(e["frames"][k]), A(mean))
            at = lambda m: (A(m[0]), m[1], m[2])
            mct, g_cv = at(e["mcspc_t"]), at(e["g_cv"])
            J, ld = e["junk"], e["ld"]
            probs += [prob(g_cv, mct, 0, -1, None, J[0]), prob(g_cv, mct, 1, -1, None, J[1], c0=1)]          # :363-364
            for tag, gs, gt, al_st, al_ts, j0, k0 in (("enc", e["g_enc_s"], e["g_enc_t"], e["al_enc_st"], e["al_enc_ts"], 2, 2),      # :334-339
                                                      ("pri", e["g_pri_s"], e["g_pri_t"], e["al_pri_st"], e["al_pri_ts"], 4, 6)):    # :349-354
                probs += [prob(at(gs), at(gt), k0, -1, al_st, J[j0]), prob(at(gt), at(gs), k0 + 1, 0, None, ld[tag + "_cos_a"]),
                          prob(at(gt), at(gs), k0 + 2, -1, al_ts, J[j0 + 1]), prob(at(gs), at(gt), k0 + 3, 0, None, ld[tag + "_cos_b"])]
                # :335, :338, :350, :353
                jobs2.append(job(_cabi.STAT_LATDIST, gt[1], 0, gt[2], A(al_st[0]), gt[2], A(gt[0]), gt[2], out_off=ld[tag + "_rmse_a"]))
                jobs2.append(job(_cabi.STAT_LATDIST, gs[1], 0, gs[2], A(al_ts[0]), gs[2], A(gs[0]), gs[2], out_off=ld[tag + "_rmse_b"]))
            probs.append(prob(at(e["gg_cv"]), mct, 10, -1, None, J[6], c0=1))                                   # :424
            # :365-368, :425-426 -- mean and np.std of the three mel-cepstrum alignments' frame costs
            for n, k in (("mcdpow_cv", 0), ("mcd_cv", 1), ("mcd_cvgv", 10)):
                jobs2.append(job(_cabi.STAT_MEANSTD64, nt, 0, 1, A(e["frames"][k]), 1, out_off=e["ms"][n], src_rows=nt))
            # :377-378, :392-393, :441, :458 -- calc_mcd(mcep at the speech frames, reconstruction at the speech frames)
            for n, mc, g, c0 in (("mcdpow_src_cv", e["mcspc_s"], e["g_cvsrc"], 0), ("mcd_src_cv", e["mcspc_s"], e["g_cvsrc"], 1),
                                 ("mcdpow_trg_cv", e["mcspc_t"], e["g_cvtrg"], 0), ("mcd_trg_cv", e["mcspc_t"], e["g_cvtrg"], 1),
                                 ("mcd_src_cvgv", e["mcspc_s"], e["gg_cvsrc"], 1), ("mcd_trg_cvgv", e["mcspc_t"], e["gg_cvtrg"], 1)):
                jobs2.append(job(_cabi.STAT_MCD64, g[1], c0, D, A(mc[0]), D, A(g[0]), D, out_off=e["ms"][n], src_rows=g[1]))
        n1, n2 = len(jobs1), len(jobs2)
        raw = bytes((_cabi.StatJob * (n1 + n2))(*(jobs1 + jobs2)))
        jdev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        dtw_bytes = lib.dtw_batch_work_bytes(len(probs), max(p.T1 for p in probs), max(p.T2 for p in probs))
        mc_bytes = lib.mc2e_batch_work_bytes(len(mc1), D, self.irlen)
        if mc_bytes == 0:
            raise _cabi.CvaeError("cvae_mc2e_batch_work_bytes: bad arguments (D=%d, irlen=%d)" % (D, self.irlen))
        dj = C.sizeof(_cabi.DecodeJob)
        up = lambda v: (v + 255) // 256 * 256
        parts = [dtw_bytes, mc_bytes, len(dA) * dj, len(dG) * dj, len(dB) * dj]
        offs = np.concatenate([[0], np.cumsum([up(v) for v in parts])])
        work = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        W = lambda k: work.data_ptr() + int(offs[k])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(9)] if profile is not None else None
        mark = (lambda k: ev[k].record()) if ev else (lambda k: None)
        mark(0)
        lib.eval_stats(jdev.data_ptr(), n1, a0, st)
        mark(1)
        lib.mc2e_batch(mc1, self.mcep_alpha, self.irlen, W(1), mc_bytes, st)
        mark(2)
        lib.decode_jobs(dA, W(2), parts[2], st)
        lib.decode_jobs(dG, W(3), parts[3], st)
        mark(3)
        lib.dtw_batch(probs, W(0), dtw_bytes, st)
        mark(4)
        lib.mc2e_batch(mc2, self.mcep_alpha, self.irlen, W(1), mc_bytes, st)
        mark(5)
        lib.decode_jobs(dB, W(4), parts[4], st)
        mark(6)
        lib.eval_stats(jdev.data_ptr() + n1 * C.sizeof(_cabi.StatJob), n2, a0, st)
        mark(7)
        host = arena[:n_out].cpu().numpy()          # the ONE D2H copy (waits for the stream)
        if ev:
            ms = lambda a, b: ev[a].elapsed_time(ev[b])
            profile.update(stats=ms(0, 1) + ms(6, 7), mc2e_1=ms(1, 2), modpow=ms(2, 3) + ms(5, 6), dtw=ms(3, 4), mc2e_2=ms(4, 5),
                           frames_1=sum(j.T for j in mc1), frames_2=sum(j.T for j in mc2), problems=len(probs),
                           jobs=n1 + n2 + len(dA) + len(dG) + len(dB))
        gru_vae.check_status()
        res = []
        for e in lay:
            r = {n: arena[off:off + (e["tb"] if "trg" in n else e["ta"]) * D].view(-1, D) for n, off in e["trj"].items()}
            for n, off in e["gv"].items():
                r[n] = host[off:off + D - 1].copy()
            for n, off in e["ms"].items():
                r[n + "_mean"], r[n + "_std"] = float(host[off]), float(host[off + 1])
            v = {n: float(host[off]) for n, off in e["ld"].items()}
            for tag in ("enc", "pri"):                                                           # :341-342, :356-357
                r["lat_dist_rmse_" + tag] = (v[tag + "_rmse_a"] + v[tag + "_rmse_b"]) / 2
                r["lat_dist_cosim_" + tag] = (v[tag + "_cos_a"] + v[tag + "_cos_b"]) / 2
            # calc_mcd's means are NaN exactly when a gathered row is (an index outside the utterance, or a NaN trajectory): an
            # alignment may step around such a row, so its figures are withdrawn here rather than trusted
            if not (np.isfinite(r["mcdpow_src_cv_mean"]) and np.isfinite(r["mcdpow_trg_cv_mean"])):
                for n in MCD_TERMS + DIST_TERMS:
                    r[n] = float("nan")
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
