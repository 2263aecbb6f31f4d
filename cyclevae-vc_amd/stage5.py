"""Stage 5 of the recipe on the device: the converted-GV statistics of calc_cvgv_gru-cyclevae_gauss.py (line numbers below are
that script's).  The script converts every training utterance pair, keeps np.var of the converted trajectory and of the two
reconstructions (:203-205) and reduces them to cvgv_mean / cvgv_var (:320-325) -- the statistic stage6.gv_postfilter consumes --
and logs MCD and latent-distance figures on the way (:208-283, :329-344).  Per utterance it copies three trajectories to the host
and calls the host library dtw_c ten times.

Here a call takes up to ten pairs.  Network half (:179-199): the 2N encoder rows as one stacked pass (stage6._encode_pairs), ONE
cvae_latent_mean launch for all 2N n_smpl_dec-draw means lat_feat, the 3N decoder rows as one stacked pass whose cells read
lat_feat as a plain input segment -- the mean is formed once and read by both the decoder and the statistics, as in the script.
Metric half (:203-283), a metricplan.MetricPlan: one f64 arena, cvae_eval_stats (GV variances, packed f64 DTW
operands), one cvae_dtw_batch (ten alignments per pair), cvae_eval_stats again (mean / std of the DTW frame costs, calc_mcd's
mean / std, the latent distances of the aligned sequences) and ONE D2H copy.  The number of library calls does not depend on N,
and every figure of a pair is one block's fixed-order reduction: it does not depend on which call the pair lands in.

PARITY UNPINNED for the DTW and calc_mcd halves: dtw_c is a third-party binary that is not in the reference tree; the yardstick
is the written definition at oracle/cyclevae_oracle.py::dtw_org_to_trg / mcd_aligned, as for stage6.dtw_org_to_trg and
validation.ValidationPass.  The GV variances are exact counterparts: the script casts the trajectory to float64 before np.var
(:195).  Out of scope: the multi-device fan-out of :120-123 (stage6.split_file_list gives the chunks), mod_pow.
"""
import numpy as np
import torch

import _cabi
import gru_vae
import stage6
from metricplan import MetricPlan

# per-pair scalars, under the script's names (:212-282)
MCD_TERMS = ("mcdpow_mean", "mcdpow_std", "mcd_mean", "mcd_std", "mcdpow_src_mean", "mcdpow_src_std", "mcd_src_mean", "mcd_src_std",
             "mcdpow_trg_mean", "mcdpow_trg_std", "mcd_trg_mean", "mcd_trg_std")
MS_NAMES = ("mcdpow", "mcd", "mcdpow_src", "mcd_src", "mcdpow_trg", "mcd_trg")      # MCD_TERMS are these with _mean / _std
DIST_TERMS = ("lat_dist_rmse_enc", "lat_dist_cosim_enc", "lat_dist_rmse_pri", "lat_dist_cosim_pri")
GV_TERMS = ("cvgv", "cvgvsrc", "cvgvtrg")                      # np.var(traj[:, 1:], 0) of cvmcep, cvmcep_src, cvmcep_trg (:203-205)
# what last_passes holds: the five trajectories of stage6.convert_pairs and the two latent means, per pair
PASS_NAMES = ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg", "lat_feat", "lat_feat_trg")
MAX_PAIRS = 10                                                   # 3N decoder rows: one 32-row tile


def dataset_suffix(mdl_name, n_cyc, lat_dim, iterations, spk_trg, n_smpl_dec):
    """:349's string: the six datasets are "/cvgv_mean_" + this, and so on."""
    return "%s-%s-%s-%s-%s-%s" % (mdl_name, n_cyc, lat_dim, iterations, spk_trg, n_smpl_dec)


def pair_inputs(plan, q, item, p, L, D):
    """Pair q's pass outputs as contiguous fp32 and its two speech-frame index lists as int64 device vectors, held by the plan;
    refused unless every pass output has the shape the kernels address it by.  Returns (outputs, ix_src, ix_trg, Ts, Tt)."""
    dev = p["cvmcep"].device
    p = {k: plan.hold(p[k].to(torch.float32).contiguous()) for k in PASS_NAMES}
    ix_s, ix_t = (plan.hold(t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()) for t in (item[2], item[3]))
    ta, tb = p["cvmcep"].shape[0], p["cvmcep_trg"].shape[0]
    want = {"cvmcep": (ta, D), "cvmcep_src": (ta, D), "cvmcep_trg": (tb, D), "lat_src": (ta, 2 * L), "lat_trg": (tb, 2 * L),
            "lat_feat": (ta, L), "lat_feat_trg": (tb, L)}
    for k, shape in want.items():      # the kernels address these by the shapes: another shape must not reach them
        if tuple(p[k].shape) != shape:
            raise ValueError("pair %d: pass output %s has shape %s, expected %s" % (q, k, tuple(p[k].shape), shape))
    if ix_s.numel() < 1 or ix_t.numel() < 1:      # (stage 5's refusal: decode.DecodePass._check_items has refused this before, in its words)
        raise ValueError("pair %d: empty speech-frame index list" % q)
    return p, ix_s, ix_t, ta, tb


def pair_operands(plan, p, ix_s, ix_t, gv_names, ms_names):
    """What stages 5 and 6 both declare for a pair.  Returns the pair's regions, which pair_figures() reads:
      "gv"  {name: result vector}: the GV variances of cvmcep, cvmcep_src, cvmcep_trg under the three gv_names (a caller with
            further GV vectors adds them here)
      "ms"  {name: result vector of (mean, std)} for ms_names; the caller declares the jobs that write them
      "g"   {pass name: packed f64 matrix}: the speech frames of all seven pass outputs
      "ld"  {"enc" / "pri": latent_distance() slots} of the encoder's and of the decoder-input latents"""
    o = {"gv": {}, "ms": {n: plan.vec(2) for n in ms_names}, "g": {}}
    for n, k in zip(gv_names, ("cvmcep", "cvmcep_src", "cvmcep_trg")):
        o["gv"][n] = plan.vec(p[k].shape[1] - 1)
        plan.stat(1, _cabi.STAT_GV, p[k].shape[0], 1, p[k].shape[1], p[k].data_ptr(), p[k].shape[1], out=o["gv"][n])
    for k in PASS_NAMES:
        ix, c = ix_t if k.endswith("trg") else ix_s, p[k].shape[1]
        o["g"][k] = plan.mat(ix.numel(), c)
        plan.stat(1, _cabi.STAT_GATHER64, ix.numel(), 0, c, p[k].data_ptr(), c, idx=ix.data_ptr(), dst=o["g"][k], src_rows=p[k].shape[0])
    o["ld"] = {"enc": plan.latent_distance(o["g"]["lat_src"], o["g"]["lat_trg"]),
               "pri": plan.latent_distance(o["g"]["lat_feat"], o["g"]["lat_feat_trg"])}
    return o


def pair_figures(host, o, mcd_terms, calc_mcd):
    """A pair's result dict from the host copy of the results and pair_operands()'s regions: the GV vectors, "<n>_mean" / "<n>_std"
    of o["ms"], DIST_TERMS.  calc_mcd: the o["ms"] names of one calc_mcd figure per side; mcd_terms: what is withdrawn with them."""
    r = {n: ref.of(host) for n, ref in o["gv"].items()}
    for n, ref in o["ms"].items():
        r[n + "_mean"], r[n + "_std"] = float(host[ref.off]), float(host[ref.off + 1])
    for tag, refs in o["ld"].items():                                                        # :264-265, :279-280
        rmse_a, rmse_b, cos_a, cos_b = (float(host[x.off]) for x in refs)
        r["lat_dist_rmse_" + tag], r["lat_dist_cosim_" + tag] = (rmse_a + rmse_b) / 2, (cos_a + cos_b) / 2
    # calc_mcd's means are NaN exactly when a gathered row is (an index outside the utterance, or a NaN trajectory): an
    # alignment may step around such a row, so its figures are withdrawn here rather than trusted
    if not all(np.isfinite(r[n + "_mean"]) for n in calc_mcd):
        for n in mcd_terms + DIST_TERMS:
            r[n] = float("nan")
    return r


class CvgvPass(object):
    """CvgvPass(model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, n_smpl_dec=300, posterior="gauss"): call pairs() on
    the training pairs, ten at a time at most, then summary() / log_lines() / write().
    posterior="laplace": the Laplace posterior of the sibling recipes, as stage6.convert_pairs(posterior="laplace") runs it -- the
    encoder passes clamp as clamp_vae_laplace does and lat_feat is the mean over n_smpl_dec draws of sampling_vae_laplace(lat)
    (cvae_latent_mean with lat_dim | CVAE_DRAW_LAPLACE; supplied eps are its uniforms in (-0.4999, 0.5)).  It has to be the posterior
    the model was trained with: a disagreement cannot be detected here and is the caller's mistake."""

    def __init__(self, model_encoder, model_decoder, lat_dim, gv_mean_src, gv_mean_trg, n_smpl_dec=300, posterior="gauss"):
        _cabi.posterior_flags(posterior, 0)      # (ValueError for anything but "gauss" / "laplace")
        self.posterior = posterior
        self.enc, self.dec, self.lat_dim, self.n_smpl_dec = model_encoder, model_decoder, int(lat_dim), int(n_smpl_dec)
        if self.lat_dim < 1 or self.n_smpl_dec < 1:
            raise ValueError("lat_dim and n_smpl_dec must be >= 1, got %d and %d" % (self.lat_dim, self.n_smpl_dec))
        self.gv_mean_src = np.asarray(gv_mean_src, np.float64)       # :127-128 ("/gv_range_mean"[1:])
        self.gv_mean_trg = np.asarray(gv_mean_trg, np.float64)
        self.reset()

    def reset(self):
        self.last_passes = None
        self.acc = {k: [] for k in GV_TERMS + MCD_TERMS + DIST_TERMS}

    # ---- :179-199 ---------------------------------------------------------------------------------------------------------------
    def network_passes(self, items, y_in_pp, y_in_src, y_in_trg, eps=None, seed=None, first_pair_id=0, profile=None):
        """The five trajectories and two latent means per pair, a list of dicts of PASS_NAMES (fp32 device tensors).  Draw ids are
        2n p and 2n p + n for list position p = first_pair_id + position in the call, as stage6.convert_many keys them.
        profile: a dict that receives the device milliseconds of "encoder", "latent_mean" and "decoder" (tools/stage5_timing.py)."""
        gru_vae.check_status()
        if not 1 <= len(items) <= MAX_PAIRS:
            raise ValueError("1..%d utterance pairs per call, got %d" % (MAX_PAIRS, len(items)))
        gru_vae._need_cuda(items[0][0], "CvgvPass.pairs(feat_src)")
        if seed is None and eps is None:
            seed = gru_vae._draw_seed()      # (a call repeated on the fp32-operand kernels draws what the first try drew)
        return gru_vae._with_range_retry(lambda: self._passes(items, y_in_pp, y_in_src, y_in_trg, eps, seed, int(first_pair_id), profile))

    def _passes(self, items, y_in_pp, y_in_src, y_in_trg, eps, seed, first, profile=None):
        lib, st = gru_vae._lib(), gru_vae._stream()
        L, n, dec = self.lat_dim, self.n_smpl_dec, self.dec
        f = lambda t: t.to(torch.float32).contiguous()
        N = len(items)
        feats = [(it[0], it[1]) for it in items]
        # A pass of at most three rows would take another recurrence kernel (the word-exchange one) than the passes of longer calls,
        # and a pair's figures would depend on the call it lands in by that kernel's rounding.  A one-pair call of a one-layer
        # network therefore repeats cells up to four rows: every call runs the row-tile kernels, whose rows are independent.
        pad_enc, pad_dec = (1, 1) if N == 1 and self.enc.hidden_layers == 1 and dec.hidden_layers == 1 else (0, 0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if profile is not None else None
        mark = (lambda k: ev[k].record()) if ev else (lambda k: None)
        mark(0)
        with torch.no_grad():
            enc = stage6._encode_pairs(self.enc, feats + feats[:pad_enc], y_in_pp, L, self.posterior)
        lens, T, lat, dev = enc["lens"][:N], enc["T"], enc["lat"], enc["dev"]
        mark(1)
        # :180-184 -- all 2N means in one launch; rows behind a cell's frames stay zero and are never read
        latfeat = torch.zeros(2 * N, T, L, dtype=torch.float32, device=dev)
        keep, jobs = [], []
        for q, (ta, tb) in enumerate(lens):
            for side, frames in ((0, ta), (1, tb)):
                e = None
                if eps is not None:
                    e = f(eps[q][side])
                    if tuple(e.shape) != (n, frames, L):
                        raise ValueError("eps of pair %d: shape %s, expected %s" % (q, tuple(e.shape), (n, frames, L)))
                    keep.append(e)
                r = 2 * q + side
                jobs.append(_cabi.LatMeanJob(lat[r].data_ptr(), None if e is None else e.data_ptr(), 2 * n * (first + q) + side * n, frames, 0,
                                             latfeat[r].data_ptr()))
        lib.latent_mean(jobs, _cabi.posterior_flags(self.posterior, L)[0], n, 0 if seed is None else int(seed), st)
        mark(2)
        # :185-199 -- [code ; lat_feat] through the decoder: cvmcep and cvmcep_src share lat_feat, cvmcep_trg reads lat_feat_trg
        Co = dec.out_dim
        dd, idd = dec.prepared(dev)
        ws = torch.empty(gru_vae.cells_workspace_bytes(dec, dd, 3 * N + pad_dec, T), dtype=torch.uint8, device=dev)
        codes = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float32, device=dev)     # src_code, trg_code (:185-193)
        out = torch.empty(3 * N + pad_dec, T, Co, dtype=torch.float32, device=dev)
        ys, yt = f(y_in_src.reshape(1, -1)), f(y_in_trg.reshape(1, -1))
        pins, yins = [], []
        for q, (ta, tb) in enumerate(lens):
            cell = lambda code_row, r, frames: lib.pass_input((codes[code_row].data_ptr(), 2, 0), seg1=(latfeat[r].data_ptr(), L, L),
                                                              frames=frames)
            pins += [cell(1, 2 * q, ta), cell(0, 2 * q, ta), cell(1, 2 * q + 1, tb)]
            yins += [yt.data_ptr(), ys.data_ptr(), yt.data_ptr()]
        pins, yins = pins + pins[:pad_dec], yins + yins[:pad_dec]
        gru_vae.run_cells(dec, dd, idd, pins, yins, T, -1, [out[r].data_ptr() for r in range(3 * N + pad_dec)], ws,
                          gru_vae._flags(dec.hidden_layers), st)
        mark(3)
        if ev:
            ev[3].synchronize()
            profile.update(encoder=ev[0].elapsed_time(ev[1]), latent_mean=ev[1].elapsed_time(ev[2]), decoder=ev[2].elapsed_time(ev[3]))
        return [{"cvmcep": out[3 * q, :ta], "cvmcep_src": out[3 * q + 1, :ta], "cvmcep_trg": out[3 * q + 2, :tb],
                 "lat_src": lat[2 * q, :ta], "lat_trg": lat[2 * q + 1, :tb], "lat_feat": latfeat[2 * q, :ta],
                 "lat_feat_trg": latfeat[2 * q + 1, :tb]} for q, (ta, tb) in enumerate(lens)]

    # ---- :203-283 ---------------------------------------------------------------------------------------------------------------
    def metrics(self, items, passes, profile=None):
        """Per-pair figures from the pass outputs (list of dicts of PASS_NAMES): cvae_eval_stats, cvae_dtw_batch, cvae_eval_stats and
        one D2H copy.  Returns a list of dicts: GV_TERMS -> [D-1] float64 numpy, MCD_TERMS and DIST_TERMS -> float.
        A speech-frame index outside its utterance makes every figure of THAT pair that reads through the index lists (MCD_TERMS,
        DIST_TERMS) NaN -- the library gathers NaN rows instead of reading there; the GV vectors do not read them and stay.
        profile: a dict that receives the device milliseconds of "stats" (both statistics launches) and "dtw", and the counts "jobs",
        "problems", "work_bytes"."""
        L = self.lat_dim
        if len(items) != len(passes) or not 1 <= len(items) <= MAX_PAIRS:
            raise ValueError("1..%d utterance pairs per call, got %d items and %d pass outputs" % (MAX_PAIRS, len(items), len(passes)))
        gru_vae._need_cuda(passes[0]["cvmcep"], "CvgvPass.metrics(cvmcep)")
        dev = passes[0]["cvmcep"].device
        plan = MetricPlan(dev, profile is not None)
        f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
        D = passes[0]["cvmcep"].shape[1]
        out = []
        for q, (it, p) in enumerate(zip(items, passes)):
            p, ix_s, ix_t, ta, tb = pair_inputs(plan, q, it, p, L, D)
            mc_s, mc_t = plan.hold(f64(it[4])), f64(it[5])
            if tuple(mc_s.shape) != (ix_s.numel(), D) or mc_t.dim() != 2 or mc_t.shape[1] != D or mc_t.shape[0] < 1:
                # (:224: calc_mcd compares mcepspc_src with the ns gathered frames row by row)
                raise ValueError("pair %d: mcepspc_src %s / mcepspc_trg %s do not fit %d speech frames of %d coefficients"
                                 % (q, tuple(mc_s.shape), tuple(mc_t.shape), ix_s.numel(), D))
            o = pair_operands(plan, p, ix_s, ix_t, GV_TERMS, MS_NAMES)                                       # :203-205, :257-262, :272-277
            g, ms, St = o["g"], o["ms"], mc_t.shape[0]
            mct = plan.f64(mc_t)
            # :210-215 -- the two alignments with mcepspc_trg; mean and np.std of their frame costs
            for n, c0 in (("mcdpow", 0), ("mcd", 1)):
                frames = plan.align(g["cvmcep"], mct, -1, c0=c0)
                plan.stat(2, _cabi.STAT_MEANSTD64, St, 0, 1, frames, 1, out=ms[n], src_rows=St)
            # :224-229, :238-243 -- calc_mcd(mcepspc, reconstruction at the speech frames), with and without coefficient 0
            for n, mc, r in (("_src", mc_s, g["cvmcep_src"]), ("_trg", mc_t, g["cvmcep_trg"])):
                for pre, c0 in (("mcdpow", 0), ("mcd", 1)):
                    plan.stat(2, _cabi.STAT_MCD64, r.rows, c0, D, mc.data_ptr(), D, r, D, out=ms[pre + n], src_rows=min(r.rows, mc.shape[0]))
            out.append(o)
        plan.finalise()
        plan.begin()
        plan.stats(1)
        plan.dtw()
        plan.stats(2)
        host = plan.results().cpu().numpy()          # the ONE D2H copy (waits for the stream)
        if profile is not None:
            t = plan.times()
            profile.update(stats=t["stats1"] + t["stats2"], dtw=t["dtw"], jobs=len(plan.table), problems=len(plan.probs),
                           work_bytes=int(plan.work_bytes))
        gru_vae.check_status()
        return [pair_figures(host, o, MCD_TERMS, ("mcdpow_src", "mcdpow_trg")) for o in out]

    def pairs(self, items, y_in_pp, y_in_src, y_in_trg, eps=None, seed=None, first_pair_id=0):
        """One call of at most ten pairs.  items: tuples (feat_src [Ts,Cin], feat_trg [Tt,Cin], spcidx_src, spcidx_trg, mcepspc_src
        [Ss,D] f64, mcepspc_trg [St,D] f64) of device tensors -- what :174-175, :208-209, :223 and :237 read; Ss = len(spcidx_src).
        eps: None (Philox draws from `seed`, keyed by first_pair_id + position so that grouping does not change them) or a list of
        (eps_src [n_smpl_dec,Ts,L], eps_trg [n_smpl_dec,Tt,L]).  Returns the per-pair dicts and appends them to the pass's lists."""
        items = list(items)
        self.last_passes = self.network_passes(items, y_in_pp, y_in_src, y_in_trg, eps, seed, first_pair_id)
        res = self.metrics(items, self.last_passes)
        for r in res:
            for k in GV_TERMS + MCD_TERMS + DIST_TERMS:
                self.acc[k].append(r[k])
        return res

    # ---- :320-344 ---------------------------------------------------------------------------------------------------------------
    def summary(self):
        """cvgv_mean / cvgv_var, cvgvsrc_*, cvgvtrg_* (:320-325) and every figure the script logs (:329-344): "<term>" and
        "<term>_std" are np.mean / np.std over the pairs of the per-pair MCD_TERMS and DIST_TERMS; gv_dist*, gv_dist*_std the log-GV
        distances of :332, :336, :340."""
        if not self.acc["cvgv"]:
            raise RuntimeError("CvgvPass.summary(): no pair seen")
        s = {}
        for g in GV_TERMS:
            v = np.array(self.acc[g])
            s[g + "_mean"], s[g + "_var"] = np.mean(v, axis=0), np.var(v, axis=0)
        for n in MCD_TERMS + DIST_TERMS:
            v = np.array(self.acc[n])
            s[n], s[n + "_std"] = float(np.mean(v)), float(np.std(v))
        for tag, g, ref in (("", "cvgv", self.gv_mean_trg), ("_src", "cvgvsrc", self.gv_mean_src), ("_trg", "cvgvtrg", self.gv_mean_trg)):
            d = np.sqrt(np.square(np.log(s[g + "_mean"]) - np.log(ref)))
            s["gv_dist" + tag], s["gv_dist" + tag + "_std"] = float(np.mean(d)), float(np.std(d))
        return s

    def log_lines(self):
        """The text of :329-344, one string per logging call."""
        s = self.summary()
        out = []
        for tag in ("", "_src", "_trg"):
            for pre in ("mcdpow", "mcd"):
                m, d = "%s%s_mean" % (pre, tag), "%s%s_std" % (pre, tag)
                out.append("%s%s: %.6f dB (+- %.6f) +- %.6f (+- %.6f)" % (pre, tag, s[m], s[m + "_std"], s[d], s[d + "_std"]))
            out.append("%f +- %f" % (s["gv_dist" + tag], s["gv_dist" + tag + "_std"]))
        for n in DIST_TERMS:
            out.append("%s: %.6f (+- %.6f)" % (n, s[n], s[n + "_std"]))
        return out

    def write(self, stats_path, suffix):
        """The six datasets of :351-362 into the source speaker's statistics file; suffix: dataset_suffix(...)."""
        import hdf5io
        s = self.summary()
        for g in GV_TERMS:
            hdf5io.write_hdf5(stats_path, "/%s_mean_%s" % (g, suffix), s[g + "_mean"])
            hdf5io.write_hdf5(stats_path, "/%s_var_%s" % (g, suffix), s[g + "_var"])


def run_files(cvgv_pass, file_pairs, y_in_pp, y_in_src, y_in_trg, per_call=10, seed=None):
    """The file loop of :170-283 on the current device: file_pairs is a list of (source feature file, target feature file), each
    with "/feat_org_lf0" [T,Cin], "/spcidx_range" [1,S] and "/mcepspc_range" [S,D]; calls of `per_call` pairs in list order.  Pair i
    draws with (seed, i).  Returns the per-pair dicts in list order."""
    import hdf5io
    if not 1 <= int(per_call) <= MAX_PAIRS:
        raise ValueError("per_call must be 1..%d, got %r" % (MAX_PAIRS, per_call))
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if seed is None:
        seed = gru_vae._draw_seed()

    def load(path):
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        return (t(hdf5io.read_hdf5(path, "/feat_org_lf0"), np.float32), t(np.asarray(hdf5io.read_hdf5(path, "/spcidx_range")).reshape(-1), np.int64),
                t(hdf5io.read_hdf5(path, "/mcepspc_range"), np.float64))
    out = []
    for k in range(0, len(file_pairs), int(per_call)):
        items = []
        for fa, fb in file_pairs[k:k + int(per_call)]:
            (xa, ia, ma), (xb, ib, mb) = load(fa), load(fb)
            items.append((xa, xb, ia, ib, ma, mb))
        out += cvgv_pass.pairs(items, y_in_pp, y_in_src, y_in_trg, seed=seed, first_pair_id=k)
    return out
