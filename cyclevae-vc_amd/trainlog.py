"""What the stage-4 training loop does AROUND every step, on the device and without a host stall (reference
train_gru_cyclevae_gauss_batch.py:660-739, :1312-1316, :1339-1353, :1364-1472: TrainLog, frame windows, batch_size > 0; :705-706,
:1476-1665: UttLog, utterance-length mini-batches, batch_size == 0).

The script reads five scalars back per utterance and cycle (`.item()`), runs four dtw_c.calc_mcd per utterance and cycle on host
copies, copies three trajectories per window to the host for its GV buffers, and at the end of an utterance batch runs one more
encoder pass and six dtw_c.dtw_org_to_trg per utterance on host copies: a device synchronisation each.  Here:

  per window       ONE launch (cvae_trainlog_window: nine f64 figures per cycle and utterance, and the window's rows appended to
                   four utterance-long device buffers), one asynchronous copy of the record and of the step's loss to a pinned slot
                   behind an event; the host formats the script's text when the slot has arrived (lines / poll)
  per batch        a metricplan.MetricPlan on the accumulated buffers: one eval-form encoder pass, GATHER64 jobs, six
                   problems of cvae_dtw_batch per utterance, LATDIST jobs, the GV variances (CVAE_STAT_GV) -- again behind an event
  per epoch        epoch_end(): the figures and the line of :719-739

PARITY UNPINNED for the DTW / calc_mcd halves (dtw_c is not in the reference tree; oracle.dtw_org_to_trg / mcd_aligned are the
written definitions).  The five loss figures and the GV variances are formed in float64 from the fp32 trajectories, where the
script's are fp32 reductions.

The GV rule of :1339-1348 appends the variances of the PREVIOUS utterance batch when a new one starts with iter_count > 0.  The
reference's generator yields one dataloader batch per pass and the loop resets iter_count at the sentinel, so with it the rule never
fires and the epoch line prints nan for the six GV figures -- exactly as the script does.  The rule is implemented as written: it
fires when two utterance batches follow each other without a sentinel between them.

Utterance-length mini-batches (UttLog): the script's branch runs the extra encoder pass BEFORE the step (:1489-1490), appends the GV
variances of the three cycle-0 trajectories per utterance at every step (:1516-1524: no "previous batch" rule, the epoch line shows
real GV figures), aligns per utterance on cycle 0 (:1526-1545) and logs the five loss figures and four calc_mcd means per utterance
and cycle (:1567-1582, without the list quirk of :1393).  Here:

  per step         before(): the no-grad encoder pass over batch_src_trg on the current stream, ahead of the step (pre-update weights);
                   after(): ONE cvae_trainlog_window launch over the whole padded utterances (no accumulators) and ONE MetricPlan
                   (3 B STAT_GV, 4 B STAT_GATHER64, 2 B alignments, B latent distances) reading the step's cycle-0 trajectories
                   directly, one copy of [record | plan results | loss] to a pinned slot behind one event
  per epoch        epoch_end(): shared with TrainLog

TrainLog and UttLog share the lists, the resets, the pinned slots, poll / lines and epoch_end through _LogBase.
"""
import os

import numpy as np
import torch

import _cabi
import gru_vae
import stage4
from metricplan import MetricPlan, batch_rows, ints, row

WIN_SRC = ("loss_mcd_src_src", "loss_mcd_src_trg_src", "loss_mcd_src_trg", "loss_lat_src", "loss_lat_src_cv")      # record [0..4]
WIN_TRG = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_lat_trg", "loss_lat_trg_cv")
DB_SRC = ("mcdpow_src_src", "mcd_src_src", "mcdpow_src_trg_src", "mcd_src_trg_src")                                # record [5..8]
DB_TRG = ("mcdpow_trg_trg", "mcd_trg_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg")
CLOSE_SRC = ("mcdpow_src_trg", "mcd_src_trg", "lat_dist_srctrg1", "lat_dist_srctrg2")                              # :679-695
CLOSE_TRG = ("mcdpow_trg_src", "mcd_trg_src", "lat_dist_trgsrc1", "lat_dist_trgsrc2")
GV_SRC = ("gv_src_src", "gv_src_trg", "gv_src_trg_src")                                                            # :1342-1344
GV_TRG = ("gv_trg_trg", "gv_trg_src", "gv_trg_src_trg")
EPOCH_ORDER = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_mcd_src_src", "loss_mcd_src_trg_src", "loss_mcd_src_trg",
               "loss_lat_trg", "loss_lat_trg_cv", "loss_lat_src", "loss_lat_src_cv",
               "eval_gv_trg_trg", "mcdpow_trg_trg", "mcd_trg_trg", "eval_gv_trg_src_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg",
               "eval_gv_trg_src", "mcdpow_trg_src", "mcdpowstd_trg_src", "mcd_trg_src", "mcdstd_trg_src", "lat_dist_trgsrc1", "lat_dist_trgsrc2",
               "eval_gv_src_src", "mcdpow_src_src", "mcd_src_src", "eval_gv_src_trg_src", "mcdpow_src_trg_src", "mcd_src_trg_src",
               "eval_gv_src_trg", "mcdpow_src_trg", "mcdpowstd_src_trg", "mcd_src_trg", "mcdstd_src_trg", "lat_dist_srctrg1", "lat_dist_srctrg2")
EPOCH_FMT = ("[%d] %.3f %.3f %.3f %.3f %.3f %.3f ; %.3f %.3f %.3f %.3f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
             "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
             "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ;; ")           # :728


class _Done(object):
    """The event of a build without a device queue (the host-fiber emulation: a call has finished when it returns)."""

    def query(self):
        return True

    def synchronize(self):
        pass


def _mean(v):
    return float(np.mean(v)) if len(v) else float("nan")


def _std(v):
    return float(np.std(v)) if len(v) else float("nan")


class _LogBase(object):
    """What TrainLog and UttLog share: the script's lists and their resets (:1202-1269), pinned slots behind events, the host half's
    queue (poll / lines) and the epoch report (:719-739).  A subclass queues (kind, event, slot, meta) in _pending and names the
    method that takes a finished slot of each kind in _TAKE."""

    MAX_IN_FLIGHT = stage4.Stage4Step.MAX_IN_FLIGHT
    _TAKE = {}

    def __init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False,
                 posterior="gauss"):
        self._laplace = stage4._check_posterior(posterior)      # (ValueError for anything but "gauss" / "laplace")
        self.posterior = posterior
        # the window launch's L (the flag makes record entries [3], [4] loss_vae_laplace's KL) and the log's own encoder passes' clamp
        self._win_L = _cabi.posterior_flags(posterior, int(lat_dim))[0]
        self._clamp_kw = {"clamp_vae_laplace": True} if self._laplace else {"clamp_vae": True}
        if not 1 <= int(n_cyc) <= _cabi.TRAINLOG_MAX_CYC:
            raise ValueError("n_cyc = %d: %s takes 1 .. %d cycles" % (n_cyc, type(self).__name__, _cabi.TRAINLOG_MAX_CYC))
        self.enc, self.dec, self.lat_dim, self.stdim, self.n_cyc = model_encoder, model_decoder, int(lat_dim), int(stdim), int(n_cyc)
        self.spk_src, self.half_cyc = spk_src, bool(half_cyc)
        self.gv_src_mean, self.gv_trg_mean = np.asarray(gv_src_mean, np.float64), np.asarray(gv_trg_mean, np.float64)
        self.epoch_idx = self.iter_idx = 0
        self._pending, self._lines, self._free = [], [], {}
        self.last_lat_srctrg = None            # (kept: the latest no-grad encoder pass over batch_src_trg)
        self.last_record = None                # (kept: the device record [n_cyc, B, 9] of the latest launch)
        self.last_args = None
        self._reset()

    def _reset(self):
        """:1202-1269."""
        names = WIN_SRC + WIN_TRG + DB_SRC + DB_TRG + CLOSE_SRC + CLOSE_TRG + GV_SRC + GV_TRG
        self.lists = {k: [[] for _ in range(self.n_cyc)] for k in names}
        self.loss, self.total = [], []
        self.iter_count = 0

    # ---- plumbing ----------------------------------------------------------------------------------------------------------------
    def _is_src(self, featfile):
        return os.path.basename(os.path.dirname(featfile)) == self.spk_src

    def _pinned(self, n):
        """A pinned float64 slot of n values from the free list (pageable where there is no device)."""
        free = self._free.setdefault(n, [])
        if free:
            return free.pop()
        return torch.empty(n, dtype=torch.float64, pin_memory=torch.cuda.is_available())

    def _behind(self, dev_tensor, slot):
        """Queue the copy of dev_tensor to the pinned slot and return the event behind it."""
        slot.copy_(dev_tensor, non_blocking=True)
        if not dev_tensor.is_cuda:
            return _Done()
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def _throttle(self, kind):
        """Wait for the oldest slot while MAX_IN_FLIGHT of `kind` are queued (as the step does)."""
        while sum(1 for q in self._pending if q[0] == kind) >= self.MAX_IN_FLIGHT:
            self._pending[0][1].synchronize()
            self.poll()

    def _traj_ptrs(self, a, trajs, B, T, D, who):
        """The trajectories of a chain (Stage4Step.last_trajs) into an argument block's traj table; returns what it points to."""
        if len(trajs) != self.n_cyc:
            raise ValueError("%s: %d cycles of trajectories, n_cyc = %d" % (who, len(trajs), self.n_cyc))
        keep = []
        for i, tr in enumerate(trajs):
            for k, name in enumerate(_cabi.TRAINLOG_SLOTS):
                t = tr[name].detach()
                want = (B, T, 2 * self.lat_dim if name in ("lat", "latcv") else D)
                if tuple(t.shape) != want or t.dtype != torch.float32:
                    raise ValueError("trajectory %s of cycle %d has shape %s, expected %s" % (name, i, tuple(t.shape), want))
                t = t.contiguous()
                keep.append(t)
                a.traj[i][k] = t.data_ptr()
        return keep

    def _align_jobs(self, plan, where, j, cv, lat, feat_trg, lat_par, spc, spc_trg, n, n_trg):
        """The jobs of one utterance's alignments (:679-688 / :1526-1542): its converted trajectory and own latents gathered at its
        n speech frames, the parallel utterance's features and latents at their n_trg, two alignments of the conversion (all
        coefficients; without the power coefficient) and the latent distance."""
        L, sd, D = self.lat_dim, self.stdim, cv.shape[2]
        ix = spc.data_ptr() + 8 * j * spc.shape[1]
        ixp = spc_trg.data_ptr() + 8 * j * spc_trg.shape[1]
        g = {}
        for key, t, idx, col, c1, rows in (("trj", cv, ix, 0, D, n), ("feat", feat_trg, ixp, sd, D, n_trg),
                                           ("par", lat_par, ixp, 0, 2 * L, n_trg), ("own", lat, ix, 0, 2 * L, n)):
            a, lda = row(t, j, col)
            g[key] = plan.mat(rows, c1)
            plan.stat(1, _cabi.STAT_GATHER64, rows, 0, c1, a, lda, idx=idx, dst=g[key], src_rows=t.shape[1])
        for name, c0 in (("mcdpow", 0), ("mcd", 1)):                                              # :679-680
            where[(name, j)] = plan.vec()
            plan.align(g["trj"], g["feat"], -1, None, where[(name, j)], c0=c0)
        where[("ld", j)] = plan.latent_distance(g["own"], g["par"])                               # :683-688

    # ---- the host half: whatever has arrived, oldest first -----------------------------------------------------------------------
    def poll(self):
        """Take the finished slots, oldest first, into the lists and the text lines; stops at the first one still in flight.
        Returns the number of slots taken."""
        n = 0
        while self._pending and self._pending[0][1].query():
            kind, _, slot, meta = self._pending.pop(0)
            getattr(self, self._TAKE[kind])(slot.numpy().copy(), meta)
            self._free.setdefault(slot.numel(), []).append(slot)
            n += 1
        return n

    def lines(self):
        """The text lines that have become available since the last call, in the script's order."""
        self.poll()
        out, self._lines = self._lines, []
        return out

    def _take_close_figures(self, host, W, j, featfile, featfile_trg):
        """:689-704 / :1535-1560 -- the four figures of one utterance's alignments into the epoch lists, and their line."""
        ld_a, ld_b, cd_a, cd_b = (float(host[r.off]) for r in W[("ld", j)])
        vals = (float(host[W[("mcdpow", j)].off]), float(host[W[("mcd", j)].off]), (ld_a + ld_b) / 2, (cd_a + cd_b) / 2)
        src = self._is_src(featfile)
        for n, x in zip(CLOSE_SRC if src else CLOSE_TRG, vals):
            self.lists[n][0].append(x)
        return ("srctrg" if src else "trgsrc", featfile, featfile_trg) + vals

    # ---- :719-739 ----------------------------------------------------------------------------------------------------------------
    def epoch_end(self):
        """Wait for everything in flight; the epoch's figures under the reference's names (n_ev_cyc = 1: the lists of cycle 1) --
        "loss", the means of the ten loss lists, of the twelve dB lists and of the four latent distances, mcdpowstd_* / mcdstd_* of
        the two conversions, eval_gv_* -- and "line", the "(EPOCH:%d) average optimization loss" text.  Then the resets of :1202-1269.
        Lines not yet fetched stay available through lines()."""
        while self._pending:
            self._pending[0][1].synchronize()
            self.poll()
        l0 = lambda n: self.lists[n][0]
        s = {"loss": _mean(self.loss)}
        for n in WIN_SRC + WIN_TRG + DB_SRC + DB_TRG + CLOSE_SRC + CLOSE_TRG:
            s[n] = _mean(l0(n))
        for n in ("mcdpow_trg_src", "mcd_trg_src", "mcdpow_src_trg", "mcd_src_trg"):
            s[n.replace("_", "std_", 1)] = _std(l0(n))
        for g in GV_SRC + GV_TRG:                                   # a conversion INTO a speaker is held against that speaker's statistics
            ref = self.gv_trg_mean if g in ("gv_trg_trg", "gv_src_trg", "gv_trg_src_trg") else self.gv_src_mean
            s["eval_" + g] = float(np.mean(np.sqrt(np.square(np.log(np.mean(l0(g), axis=0)) - np.log(ref))))) if l0(g) else float("nan")
        text = "%.3f ;; " % s["loss"] + EPOCH_FMT % ((1,) + tuple(s[n] for n in EPOCH_ORDER))
        line = "(EPOCH:%d) average optimization loss = %s" % (self.epoch_idx + 1, text)
        if self.total:
            line += "  (%.3f min., %.3f sec / batch)" % (np.sum(self.total) / 60.0, np.mean(self.total))
        s["line"] = line
        self._reset()
        self.epoch_idx += 1
        return s


class TrainLog(_LogBase):
    """TrainLog(model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False,
    posterior="gauss"), used around an unchanged stage4.Stage4Step:

        tl.before(items, y_in_pp)      # items: one 22-field yield of loader.train_generator (batch_size > 0), or the sentinel
        loss, state = step(...)
        tl.after(items, step.last_trajs, loss)
        for line in tl.lines(): logging.info(line)
        ...
        s = tl.epoch_end()             # after before(sentinel): the figures of :722-738 and s["line"], then the resets of :1202-1269

    Neither before() on a window nor after() waits for the device.  Timing fields: after(..., sec=) takes the caller's seconds for
    the "(%.3f sec)" of :1472 and the "(%.3f min., %.3f sec / batch)" of :739; without it both parentheses are omitted.
    epoch_idx (0 on construction) numbers the epoch line; set it when resuming.
    posterior="laplace", around a Stage4Step(posterior="laplace"): the window launch carries _cabi.DRAW_LAPLACE, so the two KL
    figures of a record are loss_vae_laplace's and the logged terms sum to that step's loss, and the log's own encoder pass
    (_close) clamps as clamp_vae_laplace does; the texts are unchanged.  A posterior that disagrees with the step's cannot be
    detected here and is the caller's mistake."""

    _TAKE = {"win": "_take_window", "close": "_take_close"}

    def __init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False,
                 posterior="gauss"):
        self._prev = self._prev_featfile = self._acc = None
        self._fresh = True
        _LogBase.__init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc, spk_src, half_cyc, posterior)

    # ---- before: :660-704 and the GV rule of :1339-1348 --------------------------------------------------------------------------
    def before(self, items, y_in_pp):
        if len(items) == 16:
            raise NotImplementedError("utterance-length mini-batches (batch_size == 0, train...:1476-1665) are UttLog's: TrainLog takes the "
                                      "22-field yields of loader.train_generator(batch_size > 0)")
        if len(items) != 22:
            raise ValueError("TrainLog.before: a yield of %d fields, expected 22" % len(items))
        sentinel = items[9] < 0
        if not sentinel:
            gru_vae._need_cuda(items[0], "TrainLog.before(batch_src)")
        closing = self.iter_count > 0 and (sentinel or items[5] == 0)                                 # :672
        fresh = sentinel or not (items[5] > 0 and self._prev_featfile == list(items[13]) and self.iter_count > 0)      # :1298
        gv_rows = 0
        if fresh and not sentinel and self.iter_count > 0:                                            # :1339-1340
            gv_rows = min(int(items[21]), int(self._prev[21]))
        if closing or gv_rows:
            self._close(y_in_pp, closing, gv_rows)
        self._fresh = fresh

    def _close(self, y_in_pp, closing, gv_rows):
        """The figures of the utterance batch that has just ended, from its accumulators: one encoder pass, two statistics launches
        around one cvae_dtw_batch, one copy behind an event."""
        p, L, sd = self._prev, self.lat_dim, self.stdim
        acc = self._acc
        dev = acc["cv"].device
        B, rows, D = acc["cv"].shape
        plan = MetricPlan(dev)
        plan.hold(acc)
        where = {}
        n_close = int(p[21]) if closing else 0
        flens = ints(p[15])
        for j in range(gv_rows):                                                                      # :1342-1348 (float64 here)
            if not 1 <= flens[j] <= rows:
                raise ValueError("flens_src[%d] = %d does not fit the %d accumulated frames" % (j, flens[j], rows))
            for k in ("rec", "cv", "reccyc"):
                a, lda = row(acc[k], j)
                where[("gv", k, j)] = plan.vec(D - 1)
                plan.stat(1, _cabi.STAT_GV, flens[j], 1, D, a, lda, out=where[("gv", k, j)])
        if closing:
            feat_trg = plan.hold(p[3].to(torch.float32).contiguous())
            spc = plan.hold(p[11].to(device=dev, dtype=torch.int64).contiguous())
            spc_trg = plan.hold(p[12].to(device=dev, dtype=torch.int64).contiguous())
            ns, nsp = ints(p[17]), ints(p[18])
            if feat_trg.shape[0] != B or spc.shape[0] != B or spc_trg.shape[0] != B or feat_trg.shape[2] != sd + D:
                raise ValueError("the previous yield does not hold %d utterances of %d features" % (B, sd + D))
            for j in range(n_close):
                if not (1 <= ns[j] <= spc.shape[1] and 1 <= nsp[j] <= spc_trg.shape[1]):
                    raise ValueError("flens_spc of utterance %d (%d, %d) do not fit the speech-frame index rows" % (j, ns[j], nsp[j]))
            with torch.no_grad():                                                                     # :673-677
                lat_par = self.enc(feat_trg, batch_rows(y_in_pp, B), lat_dim=L, **self._clamp_kw)[0].contiguous()
            self.last_lat_srctrg = lat_par
        for j in range(n_close):
            self._align_jobs(plan, where, j, acc["cv"], acc["lat"], feat_trg, lat_par, spc, spc_trg, ns[j], nsp[j])
        plan.finalise()
        plan.begin(pinned=True)
        plan.stats(1)
        plan.dtw()
        plan.stats(2)
        slot = self._pinned(max(1, plan.n_out))
        ev = self._behind(plan.results(), slot)
        meta = dict(where=where, gv_rows=gv_rows, n_close=n_close, files=list(p[13]), files_trg=list(p[14]),
                    gv_files=list(self._prev_featfile or []), keep=plan)
        self._pending.append(("close", ev, slot, meta))

    # ---- after: the window's launch ----------------------------------------------------------------------------------------------
    def after(self, items, trajs, loss, sec=None):
        """Launch cvae_trainlog_window on the trajectories of the window's chain (Stage4Step.last_trajs), queue the copy of its record
        and of `loss` (the step's 0-dim loss tensor) behind an event, and return.  sec: the caller's seconds for this window."""
        if len(items) != 22 or items[9] < 0:
            raise ValueError("TrainLog.after: not a window's yield")
        x, s, e = items[0], int(items[5]), int(items[6])
        gru_vae._need_cuda(x, "TrainLog.after(batch_src)")
        if len(trajs) != self.n_cyc:
            raise ValueError("TrainLog.after: %d cycles of trajectories, n_cyc = %d" % (len(trajs), self.n_cyc))
        self._throttle("win")
        B, F, Cin = x.shape
        T, L, sd = e - s + 1, self.lat_dim, self.stdim
        D = Cin - sd
        dev = x.device
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("TrainLog.after: batch_src must be a contiguous float32 tensor")
        if not 0 <= s <= e < F:
            raise ValueError("TrainLog.after: window %d .. %d outside the %d frames of batch_src" % (s, e, F))
        a = _cabi.TrainlogWindowArgs()
        keep = self._traj_ptrs(a, trajs, B, T, D, "TrainLog.after")
        if self._fresh or self._acc is None or self._acc["cv"].shape[:2] != (B, F):                   # :1349-1353
            self._acc = {"rec": torch.zeros(B, F, D, dtype=torch.float32, device=dev), "cv": torch.zeros(B, F, D, dtype=torch.float32, device=dev),
                         "reccyc": torch.zeros(B, F, D, dtype=torch.float32, device=dev), "lat": torch.zeros(B, F, 2 * L, dtype=torch.float32, device=dev)}
        spc = items[11]
        if spc.dtype != torch.int64 or not spc.is_contiguous() or spc.shape[0] != B:
            raise ValueError("TrainLog.after: spcidx_src must be a contiguous int64 tensor of %d rows" % B)
        sel = np.zeros(B, np.uint8)
        sel_list = [int(j) for j in items[19]]
        sel[sel_list] = 1
        host = [np.ascontiguousarray(np.asarray(items[20]), np.int32), np.ascontiguousarray(np.asarray(items[7]), np.int32),
                np.ascontiguousarray(np.asarray(items[8]), np.int32), sel]
        if any(h.shape != (B,) for h in host):
            raise ValueError("TrainLog.after: the generator's bookkeeping does not hold %d utterances" % B)
        n = self.n_cyc * B * _cabi.TRAINLOG_REC
        rec = torch.empty(n + 1, dtype=torch.float64, device=dev)
        a.x_win, a.x_row_stride, a.x_utt_stride = x.data_ptr() + 4 * s * Cin, Cin, F * Cin
        a.spcidx, a.spc_ld = spc.data_ptr(), spc.shape[1]
        a.flen_acc, a.s_idx, a.e_idx, a.selected = (h.ctypes.data for h in host)
        a.n_cyc, a.B, a.T, a.D, a.L, a.stdim, a.src_idx_s, a.acc_rows = self.n_cyc, B, T, D, self._win_L, sd, s, F
        for q, k in enumerate(("rec", "cv", "reccyc", "lat")):
            a.acc[q] = self._acc[k].data_ptr()
        a.rec_out = rec.data_ptr()
        gru_vae._lib().trainlog_window(a, gru_vae._stream())
        self.last_args = (a, keep, host)       # (kept: the argument block of the latest launch and what it points to, for tools/trainlog_timing.py)
        self.last_record = rec[:n].view(self.n_cyc, B, _cabi.TRAINLOG_REC)
        self._prev, self._prev_featfile = items, list(items[13])                                      # :1354
        if not sel_list:                                                                              # :1356: no loss, no step, no line
            return
        rec[n:].copy_(loss.detach().reshape(1))
        slot = self._pinned(n + 1)
        ev = self._behind(rec, slot)
        meta = dict(B=B, sel=sel_list, spoken=[j for j in sel_list if int(host[1][j]) >= 0], files=list(items[13]), c_idx=int(items[9]),
                    sec=sec, keep=keep)
        self._pending.append(("win", ev, slot, meta))
        self.iter_idx += 1
        self.iter_count += 1

    # ---- the host half -----------------------------------------------------------------------------------------------------------
    def _take_close(self, host, meta):
        W = meta["where"]
        for j in range(meta["gv_rows"]):                                                              # :1341-1348
            names = GV_SRC if self._is_src(meta["gv_files"][j]) else GV_TRG
            for n, k in zip(names, ("rec", "cv", "reccyc")):
                self.lists[n][0].append(W[("gv", k, j)].of(host))
        for j in range(meta["n_close"]):                                                              # :689-704
            self._lines.append("batch %s loss %s %s = %.3f dB %.3f dB , %.3f %.3f" % self._take_close_figures(
                host, W, j, meta["files"][j], meta["files_trg"][j]))

    def _take_window(self, host, meta):
        B, sel, spoken = meta["B"], meta["sel"], meta["spoken"]
        R = host[:-1].reshape(self.n_cyc, B, _cabi.TRAINLOG_REC)
        loss = float(host[-1])
        means = []
        for i in range(self.n_cyc):
            for j in sel:                                                                             # :1373-1386
                for n, q in zip(WIN_SRC if self._is_src(meta["files"][j]) else WIN_TRG, range(5)):
                    self.lists[n][i].append(float(R[i, j, q]))
            kl, klcv = [R[i, j, 3] for j in sel], [R[i, j, 4] for j in sel]
            # :1393: with more than one selected utterance the script rebuilds the lat_src_cv list from the lat_src list
            # (stage4.script_loss_loop): KL(lat) of every utterance and KL(latcv) of the LAST one
            cvlist = klcv if len(sel) == 1 else kl + [klcv[-1]]
            means.append((_mean([R[i, j, 0] for j in sel]), _mean([R[i, j, 1] for j in sel]), _mean([R[i, j, 2] for j in sel]),
                          _mean(kl), _mean(cvlist)))                                                  # :1412-1416
        self.loss.append(loss)                                                                        # :1422
        for j in spoken:                                                                              # :1431-1458
            for i in range(self.n_cyc):
                for n, q in zip(DB_SRC if self._is_src(meta["files"][j]) else DB_TRG, (5, 6, 7, 8)):
                    self.lists[n][i].append(float(R[i, j, q]))
        text = "%.3f ;; " % loss                                                                      # :1460-1471 (print_mcd_flag = bool(spoken))
        for i in range(self.n_cyc):
            text += "[%d] %.3f %.3f %.3f ; %.3f %.3f " % ((i + 1,) + means[i])
            if spoken:
                text += "; %.3f dB %.3f dB , %.3f dB %.3f dB " % tuple(_mean([R[i, j, q] for j in spoken]) for q in (5, 6, 7, 8))
            text += ";; "
        line = "batch loss [%d] = %s" % (meta["c_idx"] + 1, text)                                     # :1472
        if meta["sec"] is not None:
            line += "  (%.3f sec)" % meta["sec"]
            self.total.append(float(meta["sec"]))
        self._lines.append(line)



class UttLog(_LogBase):
    """UttLog(model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False,
    posterior="gauss"): TrainLog's sibling for utterance-length mini-batches (train...:705-706, :1476-1665), around an unchanged
    stage4.Stage4Step:

        ul.before(items, y_in_pp)      # items: one 16-field yield of loader.train_generator(batch_size=0), or the sentinel
        loss = step(**stage4.utterance_step_args(items), y_in_enc=..., y_in_dec=..., eps=None)
        ul.after(items, step.last_trajs, loss)
        for line in ul.lines(): logging.info(line)
        ...
        s = ul.epoch_end()             # after before(sentinel)

    before() runs the no-grad encoder pass of :1489-1490 over batch_src_trg on the current stream, AHEAD of the step, so it reads
    the weights the script reads; after() launches the step's figures.  Neither waits for the device; after() stalls only with
    MAX_IN_FLIGHT slots queued.  sec= and epoch_idx as in TrainLog.  posterior as in TrainLog: "laplace" puts the flag on the
    window launch and the Laplace clamp on before()'s encoder pass; it must be the step's posterior, which cannot be detected here."""

    _TAKE = {"utt": "_take_utt"}

    def __init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False,
                 posterior="gauss"):
        self._lat_of = None                    # the yield the kept encoder pass belongs to
        _LogBase.__init__(self, model_encoder, model_decoder, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc, spk_src, half_cyc, posterior)

    @staticmethod
    def _fields(items, who):
        if len(items) == 22:
            raise NotImplementedError("%s: a 22-field yield is a frame window (batch_size > 0, train...:1298-1472): that is TrainLog's; "
                                      "UttLog takes the 16-field yields of loader.train_generator(batch_size=0)" % who)
        if len(items) != 16:
            raise ValueError("%s: a yield of %d fields, expected 16" % (who, len(items)))

    # ---- before: :1489-1490 ------------------------------------------------------------------------------------------------------
    def before(self, items, y_in_pp):
        self._fields(items, "UttLog.before")
        if items[5] < 0:                       # the sentinel: nothing but the epoch's end (epoch_end() is the caller's next call)
            self._lat_of = None
            return
        feat_trg = items[3]
        gru_vae._need_cuda(items[0], "UttLog.before(batch_src)")
        gru_vae._need_cuda(feat_trg, "UttLog.before(batch_src_trg)")
        B = feat_trg.shape[0]
        with torch.no_grad():                  # (on the current stream, ahead of the step: the pre-update weights)
            self.last_lat_srctrg = self.enc(feat_trg.to(torch.float32).contiguous(), batch_rows(y_in_pp, B), lat_dim=self.lat_dim,
                                            **self._clamp_kw)[0].contiguous()
        self._lat_of = items

    # ---- after: one window launch, one plan, one copy ----------------------------------------------------------------------------
    def after(self, items, trajs, loss, sec=None):
        """The figures of the step on `items` from the trajectories of its chain (Stage4Step.last_trajs) and its 0-dim loss tensor:
        cvae_trainlog_window over the whole padded utterances, a MetricPlan on the cycle-0 trajectories and before()'s encoder
        pass, and the copy of [record | plan results | loss] behind an event.  sec: the caller's seconds for this step."""
        self._fields(items, "UttLog.after")
        if items[5] < 0:
            raise ValueError("UttLog.after: not an utterance batch's yield")
        x, feat_trg, spc, spc_trg = items[0], items[3], items[7], items[8]
        gru_vae._need_cuda(x, "UttLog.after(batch_src)")
        if self._lat_of is not items:
            raise ValueError("UttLog.after: before() has not been given this yield")
        self._throttle("utt")
        B, T, Cin = x.shape
        L, sd = self.lat_dim, self.stdim
        D = Cin - sd
        dev = x.device
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("UttLog.after: batch_src must be a contiguous float32 tensor")
        if int(items[15]) != B:
            raise ValueError("UttLog.after: n_batch_utt = %d, batch_src holds %d utterances" % (int(items[15]), B))
        a = _cabi.TrainlogWindowArgs()
        keep = self._traj_ptrs(a, trajs, B, T, D, "UttLog.after")
        if spc.dtype != torch.int64 or not spc.is_contiguous() or spc.shape[0] != B:
            raise ValueError("UttLog.after: spcidx_src must be a contiguous int64 tensor of %d rows" % B)
        flens, ns, nsp = ints(items[11]), ints(items[13]), ints(items[14])
        if not (len(flens) == len(ns) == len(nsp) == len(items[9]) == len(items[10]) == B):
            raise ValueError("UttLog.after: the generator's bookkeeping does not hold %d utterances" % B)
        lat_par = self.last_lat_srctrg
        feat_trg = feat_trg.to(torch.float32).contiguous()
        spc_trg = spc_trg.to(device=dev, dtype=torch.int64).contiguous()
        if feat_trg.shape[0] != B or spc_trg.shape[0] != B or feat_trg.shape[2] != Cin or tuple(lat_par.shape[:2]) != tuple(feat_trg.shape[:2]):
            raise ValueError("UttLog.after: batch_src_trg / spcidx_src_trg do not hold %d utterances of %d features" % (B, Cin))
        for j in range(B):
            if not 1 <= flens[j] <= T:
                raise ValueError("flens_src[%d] = %d does not fit the %d padded frames" % (j, flens[j], T))
            if not (1 <= ns[j] <= spc.shape[1] and 1 <= nsp[j] <= spc_trg.shape[1]):
                raise ValueError("flens_spc of utterance %d (%d, %d) do not fit the speech-frame index rows" % (j, ns[j], nsp[j]))
        # the window launch: the whole utterance is the window (:1567-1582)
        host = [np.ascontiguousarray(flens, np.int32), np.zeros(B, np.int32), np.ascontiguousarray(ns, np.int32) - 1, np.ones(B, np.uint8)]
        # the plan on cycle 0: :1516-1524 (GV), :1526-1545 (alignments)
        plan = MetricPlan(dev)
        plan.hold((keep, feat_trg, spc, spc_trg, lat_par))
        tr0 = {name: keep[k] for k, name in enumerate(_cabi.TRAINLOG_SLOTS)}
        where = {}
        for j in range(B):
            for k in ("rec", "cv", "reccyc"):
                at, lda = row(tr0[k], j)
                where[("gv", k, j)] = plan.vec(D - 1)
                plan.stat(1, _cabi.STAT_GV, flens[j], 1, D, at, lda, out=where[("gv", k, j)])
        for j in range(B):
            self._align_jobs(plan, where, j, tr0["cv"], tr0["lat"], feat_trg, lat_par, spc, spc_trg, ns[j], nsp[j])
        plan.finalise()
        n, n_out = self.n_cyc * B * _cabi.TRAINLOG_REC, max(1, plan.n_out)
        out = torch.empty(n + n_out + 1, dtype=torch.float64, device=dev)        # [record | plan results | loss]: ONE copy to the host
        a.x_win, a.x_row_stride, a.x_utt_stride = x.data_ptr(), Cin, T * Cin
        a.spcidx, a.spc_ld = spc.data_ptr(), spc.shape[1]
        a.flen_acc, a.s_idx, a.e_idx, a.selected = (h.ctypes.data for h in host)
        a.n_cyc, a.B, a.T, a.D, a.L, a.stdim, a.src_idx_s, a.acc_rows = self.n_cyc, B, T, D, self._win_L, sd, 0, 0
        a.rec_out = out.data_ptr()
        gru_vae._lib().trainlog_window(a, gru_vae._stream())
        self.last_args = (a, keep, host)
        self.last_record = out[:n].view(self.n_cyc, B, _cabi.TRAINLOG_REC)
        plan.begin(pinned=True)
        plan.stats(1)
        plan.dtw()
        plan.stats(2)
        out[n:n + n_out].copy_(plan.results())
        out[n + n_out:].copy_(loss.detach().reshape(1))
        slot = self._pinned(out.numel())
        ev = self._behind(out, slot)
        meta = dict(B=B, n=n, where=where, files=list(items[9]), files_trg=list(items[10]), flens=flens, flens_trg=ints(items[12]), ns=ns, nsp=nsp,
                    c_idx=int(items[5]), sec=sec, keep=(plan, out))
        self._pending.append(("utt", ev, slot, meta))
        self._lat_of = None
        self.iter_idx += 1
        self.iter_count += 1

    # ---- the host half -----------------------------------------------------------------------------------------------------------
    def _take_utt(self, host, meta):
        B, n, W, files, files_trg = meta["B"], meta["n"], meta["where"], meta["files"], meta["files_trg"]
        R = host[:n].reshape(self.n_cyc, B, _cabi.TRAINLOG_REC)
        res, loss = host[n:-1], float(host[-1])
        for j in range(B):                                                                            # :1478
            self._lines.append("%s %s %d %d %d %d" % (files[j], files_trg[j], meta["flens"][j], meta["flens_trg"][j], meta["ns"][j], meta["nsp"][j]))
        for j in range(B):
            for name, k in zip(GV_SRC if self._is_src(files[j]) else GV_TRG, ("rec", "cv", "reccyc")):  # :1517-1524
                self.lists[name][0].append(W[("gv", k, j)].of(res))
            self._lines.append("batch %s loss %s %s = %.3f dB %.3f dB , %.3f %.3f " % self._take_close_figures(      # :1547-1560
                res, W, j, files[j], files_trg[j]))
        for i in range(self.n_cyc):                                                                   # :1599-1622
            for j in range(B):
                src = self._is_src(files[j])
                for name, q in zip(WIN_SRC if src else WIN_TRG, range(5)):
                    self.lists[name][i].append(float(R[i, j, q]))
                for name, q in zip(DB_SRC if src else DB_TRG, (5, 6, 7, 8)):
                    self.lists[name][i].append(float(R[i, j, q]))
        self.loss.append(loss)                                                                        # :1655
        text = "%.3f ;; " % loss                                                                      # :1657-1662: means over every utterance
        for i in range(self.n_cyc):
            text += "[%d] %.3f %.3f %.3f ; %.3f %.3f ; %.3f dB %.3f dB , %.3f dB %.3f dB;; " % (
                (i + 1,) + tuple(float(np.mean(R[i, :, q])) for q in range(9)))
        line = "batch loss [%d] = %s" % (meta["c_idx"] + 1, text)                                     # :1663
        if meta["sec"] is not None:
            line += "  (%.3f sec)" % meta["sec"]
            self.total.append(float(meta["sec"]))
        self._lines.append(line)
