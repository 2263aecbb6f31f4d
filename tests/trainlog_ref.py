"""TEST INFRASTRUCTURE: numpy float64 restatement of what the stage-4 training loop does AROUND every step
(train_gru_cyclevae_gauss_batch.py; line numbers below are that script's), composed of oracle.mcd_aligned, oracle.dtw_org_to_trg
and numpy: the yardstick of cvae_trainlog_window and trainlog.TrainLog.

PARITY UNPINNED for the dtw_org_to_trg / calc_mcd halves (dtw_c is not in the reference tree; the oracle's written definitions
stand in, as in validation_ref).  Deliberate differences, the library's as well: the five loss figures of :1366-1371 are formed in
float64 from the fp32 trajectories (the script's are fp32 torch reductions), and so are the variances of :1342-1348.

A window's bookkeeping is the generator's: src_idx_s, select_utt_idx, flen_acc, spcidx_src_s_idx, spcidx_src_e_idx.  trajs is the
list over cycles of {"lat", "rec", "cv", "latcv", "reccyc"} arrays [B, T, C] (stage4.chain_forward)."""
import os

import numpy as np

from oracle import cyclevae_oracle as orc

SQRT2 = 1.4142135623730950488016887242097
f64 = lambda a: np.array(a, dtype=np.float64)


def window_record(trajs, x_win, stdim, lat_dim, spcidx, select, flen_acc, s_idx, e_idx, src_idx_s):
    """[n_cyc, B, 9]: per cycle and utterance the five loss figures of :1366-1371 and the four calc_mcd means of :1435-1439; NaN
    where the script forms none (utterance not selected; no speech frame in the window).  x_win: batch_src[:, s:e+1]."""
    B, T = x_win.shape[0], x_win.shape[1]
    L = lat_dim
    out = np.full((len(trajs), B, 9), np.nan)
    for i, tr in enumerate(trajs):
        for j in select:
            n = min(int(flen_acc[j]), T)                       # (a Python slice clips at the window's length)
            if n > 0:
                tgt = f64(x_win[j, :n, stdim:])
                for q, slot in enumerate(("rec", "reccyc", "cv")):                                      # :1366-1368, gru_vae.py:525-533
                    out[i, j, q] = np.mean(orc.MCD_K * SQRT2 * np.sum(np.abs(f64(tr[slot][j, :n]) - tgt), 1))
                for q, slot in ((3, "lat"), (4, "latcv")):                                              # :1370-1371, gru_vae.py:117-123
                    mu, s = f64(tr[slot][j, :n, :L]), f64(tr[slot][j, :n, L:])
                    out[i, j, q] = np.mean(0.5 * np.sum(np.exp(s) + mu * mu - s - 1.0, 1))
            if int(s_idx[j]) >= 0:                                                                      # :1432
                fr = np.asarray(spcidx[j, int(s_idx[j]):int(e_idx[j]) + 1], np.int64)
                rows = fr - src_idx_s
                if len(fr) == 0 or rows.min() < 0 or rows.max() >= T:
                    continue                                   # (the script would fault or wrap; the library answers NaN)
                tgt = f64(x_win[j][rows][:, stdim:])           # batch_src[j][f_k] IS the window's row f_k - src_idx_s
                for q, slot in ((5, "rec"), (7, "reccyc")):                                             # :1435-1439
                    y = f64(tr[slot][j][rows])
                    out[i, j, q] = orc.mcd_aligned(tgt, y, d0=0, L2=True)[1]
                    out[i, j, q + 1] = orc.mcd_aligned(tgt, y, d0=1, L2=True)[1]
    return out


def accumulate(acc, trajs, src_idx_s):
    """:1312-1316 / :1349-1353 -- the window's rows of cycle 0 behind the earlier ones (acc None: a fresh first window).  Whole rows
    are kept; the consumers of tmp_* take [:, 1:]."""
    new = {k: np.array(trajs[0][k]) for k in ("rec", "cv", "reccyc", "lat")}
    if acc is None or src_idx_s == 0:
        return new
    return {k: np.concatenate((acc[k], new[k]), axis=1) for k in new}


def _mean(v):
    return float(np.mean(v)) if len(v) else float("nan")


def _std(v):
    return float(np.std(v)) if len(v) else float("nan")


WIN_SRC = ("loss_mcd_src_src", "loss_mcd_src_trg_src", "loss_mcd_src_trg", "loss_lat_src", "loss_lat_src_cv")
WIN_TRG = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_lat_trg", "loss_lat_trg_cv")
DB_SRC = ("mcdpow_src_src", "mcd_src_src", "mcdpow_src_trg_src", "mcd_src_trg_src")
DB_TRG = ("mcdpow_trg_trg", "mcd_trg_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg")
CLOSE_SRC = ("mcdpow_src_trg", "mcd_src_trg", "lat_dist_srctrg1", "lat_dist_srctrg2")
CLOSE_TRG = ("mcdpow_trg_src", "mcd_trg_src", "lat_dist_trgsrc1", "lat_dist_trgsrc2")
GV_SRC = ("gv_src_src", "gv_src_trg", "gv_src_trg_src")
GV_TRG = ("gv_trg_trg", "gv_trg_src", "gv_trg_src_trg")


class RefTrainLog(object):
    """The lists of the training loop and what is printed from them: :660-704 (before), :1339-1353 and :1364-1472 (after), :719-739
    and the resets of :1202-1269 (epoch_end).  The network is not run here: every call is given the trajectories it is about."""

    def __init__(self, lat_dim, stdim, gv_src_mean, gv_trg_mean, n_cyc=2, spk_src=None, half_cyc=False):
        self.L, self.stdim, self.n_cyc, self.spk_src, self.half_cyc = lat_dim, stdim, n_cyc, spk_src, half_cyc
        self.gv_src_mean, self.gv_trg_mean = f64(gv_src_mean), f64(gv_trg_mean)
        self.epoch_idx = self.iter_idx = self.iter_count = 0
        self.prev = self.acc = self.prev_featfile = None
        self.lines = []
        self._reset()

    def _reset(self):                                          # :1202-1269
        self.lists = {k: [[] for _ in range(self.n_cyc)] for k in WIN_SRC + WIN_TRG + DB_SRC + DB_TRG + CLOSE_SRC + CLOSE_TRG + GV_SRC + GV_TRG}
        self.loss, self.total = [], []
        self.iter_count = 0

    def _is_src(self, featfile):
        return os.path.basename(os.path.dirname(featfile)) == self.spk_src

    def before(self, items, lat_srctrg=None):
        """items: the generator's 22-field yield, as numpy / host values.  lat_srctrg: the eval-form encoder pass over the PREVIOUS
        batch_src_trg (:675), needed when this call closes an utterance batch."""
        sentinel = items[9] < 0
        if self.iter_count > 0 and (sentinel or items[5] == 0):                                        # :672
            p, sd = self.prev, self.stdim
            feat_trg, spc, spc_trg, files, files_trg, ns, nsp = p[3], p[11], p[12], p[13], p[14], p[17], p[18]
            for i in range(p[21]):                                                                      # :678
                ix, ixp = spc[i, :int(ns[i])], spc_trg[i, :int(nsp[i])]
                trj, tgt = f64(self.acc["cv"][i][ix]), f64(feat_trg[i][:, sd:][ixp])
                mcdpow = orc.dtw_org_to_trg(trj, tgt)[2]                                                # :679
                mcd = orc.dtw_org_to_trg(trj[:, 1:], tgt[:, 1:])[2]                                     # :680
                par, own = f64(lat_srctrg[i][ixp]), f64(self.acc["lat"][i][ix])                         # :681-682
                d1 = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(own, par)[0] - par) ** 2, axis=0)))    # :683-684
                c1 = orc.dtw_org_to_trg(par, own, mcd=0)[2]                                             # :685
                d2 = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(par, own)[0] - own) ** 2, axis=0)))    # :686-687
                c2 = orc.dtw_org_to_trg(own, par, mcd=0)[2]                                             # :688
                vals = (mcdpow, mcd, (d1 + d2) / 2, (c1 + c2) / 2)
                src = self._is_src(files[i])
                for n, v in zip(CLOSE_SRC if src else CLOSE_TRG, vals):                                 # :689-703
                    self.lists[n][0].append(float(v))
                self.lines.append("batch %s loss %s %s = %.3f dB %.3f dB , %.3f %.3f" % (("srctrg" if src else "trgsrc", files[i], files_trg[i]) + vals))
        if sentinel:
            return
        fresh = not (items[5] > 0 and self.prev_featfile == list(items[13]) and self.iter_count > 0)   # :1298
        if fresh and self.iter_count > 0:                                                               # :1339-1348
            flens = self.prev[15]
            for j in range(min(items[21], self.prev[21])):
                names = GV_SRC if self._is_src(self.prev_featfile[j]) else GV_TRG
                for n, k in zip(names, ("rec", "cv", "reccyc")):
                    self.lists[n][0].append(np.var(f64(self.acc[k][j, :int(flens[j]), 1:]), axis=0))
        self._fresh = fresh

    def after(self, items, trajs, loss, sec=None):
        """trajs: numpy trajectories of the window's chain; loss: the step's batch loss (a float)."""
        s, e, s_idx, e_idx, files, sel, flen_acc = items[5], items[6], items[7], items[8], items[13], list(items[19]), items[20]
        self.acc = accumulate(None if self._fresh else self.acc, trajs, 0 if self._fresh else s)       # :1312-1316, :1349-1353
        self.prev_featfile, self.prev = list(files), items                                              # :1354
        if not sel:                                                                                     # :1356
            return
        R = window_record(trajs, items[0][:, s:e + 1], self.stdim, self.L, items[11], sel, flen_acc, s_idx, e_idx, s)
        means = []
        for i in range(self.n_cyc):
            for j in sel:                                                                               # :1373-1386
                names = WIN_SRC if self._is_src(files[j]) else WIN_TRG
                for n, q in zip(names, (0, 1, 2, 3, 4)):
                    self.lists[n][i].append(float(R[i, j, q]))
            kl, klcv = [R[i, j, 3] for j in sel], [R[i, j, 4] for j in sel]
            cvlist = klcv if len(sel) == 1 else kl + [klcv[-1]]                                         # :1393 (rebuilt from the lat list)
            means.append([_mean([R[i, j, 0] for j in sel]), _mean([R[i, j, 1] for j in sel]), _mean([R[i, j, 2] for j in sel]),
                          _mean(kl), _mean(cvlist)])                                                    # :1412-1416
        self.loss.append(float(loss))                                                                   # :1422
        spoken = [j for j in sel if int(s_idx[j]) >= 0]                                                 # :1431-1433
        for j in spoken:
            names = DB_SRC if self._is_src(files[j]) else DB_TRG
            for i in range(self.n_cyc):
                for n, q in zip(names, (5, 6, 7, 8)):                                                   # :1447-1458
                    self.lists[n][i].append(float(R[i, j, q]))
        text = "%.3f ;; " % float(loss)                                                                 # :1460-1471
        for i in range(self.n_cyc):
            text += "[%d] %.3f %.3f %.3f ; %.3f %.3f " % ((i + 1,) + tuple(means[i]))
            if spoken:
                text += "; %.3f dB %.3f dB , %.3f dB %.3f dB " % tuple(_mean([R[i, j, q] for j in spoken]) for q in (5, 6, 7, 8))
            text += ";; "
        line = "batch loss [%d] = %s" % (items[9] + 1, text)                                            # :1472
        if sec is not None:
            line += "  (%.3f sec)" % sec
            self.total.append(sec)
        self.lines.append(line)
        self.iter_idx += 1
        self.iter_count += 1

    def epoch_end(self):
        """:719-739 for n_ev_cyc = 1, then the resets."""
        l0 = lambda n: self.lists[n][0]
        s = {"loss": _mean(self.loss)}
        for n in WIN_SRC + WIN_TRG + DB_SRC + DB_TRG + CLOSE_SRC + CLOSE_TRG:
            s[n] = _mean(l0(n))
        for n in ("mcdpow_trg_src", "mcd_trg_src", "mcdpow_src_trg", "mcd_src_trg"):
            s[n.replace("_", "std_", 1)] = _std(l0(n))
        for g in GV_SRC + GV_TRG:                              # a conversion INTO a speaker is held against that speaker's statistics (:722-727)
            ref = self.gv_trg_mean if g in ("gv_trg_trg", "gv_src_trg", "gv_trg_src_trg") else self.gv_src_mean
            s["eval_" + g] = float(np.mean(np.sqrt(np.square(np.log(np.mean(l0(g), axis=0)) - np.log(ref))))) if l0(g) else float("nan")
        text = "%.3f ;; " % s["loss"] + epoch_text(s)
        line = "(EPOCH:%d) average optimization loss = %s" % (self.epoch_idx + 1, text)
        if self.total:
            line += "  (%.3f min., %.3f sec / batch)" % (np.sum(self.total) / 60.0, np.mean(self.total))
        s["line"] = line
        self._reset()
        self.epoch_idx += 1
        return s


def epoch_text(s):
    """The "[1] ..." part of :728-738 from the figures' dictionary."""
    order = ("loss_mcd_trg_trg", "loss_mcd_trg_src_trg", "loss_mcd_trg_src", "loss_mcd_src_src", "loss_mcd_src_trg_src", "loss_mcd_src_trg",
             "loss_lat_trg", "loss_lat_trg_cv", "loss_lat_src", "loss_lat_src_cv",
             "eval_gv_trg_trg", "mcdpow_trg_trg", "mcd_trg_trg", "eval_gv_trg_src_trg", "mcdpow_trg_src_trg", "mcd_trg_src_trg",
             "eval_gv_trg_src", "mcdpow_trg_src", "mcdpowstd_trg_src", "mcd_trg_src", "mcdstd_trg_src", "lat_dist_trgsrc1", "lat_dist_trgsrc2",
             "eval_gv_src_src", "mcdpow_src_src", "mcd_src_src", "eval_gv_src_trg_src", "mcdpow_src_trg_src", "mcd_src_trg_src",
             "eval_gv_src_trg", "mcdpow_src_trg", "mcdpowstd_src_trg", "mcd_src_trg", "mcdstd_src_trg", "lat_dist_srctrg1", "lat_dist_srctrg2")
    return ("[%d] %.3f %.3f %.3f %.3f %.3f %.3f ; %.3f %.3f %.3f %.3f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
            "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ; %.6f %.3f dB %.6f dB , %.3f %.3f dB %.3f dB , "
            "%.6f %.3f dB (+- %.3f) %.6f dB (+- %.3f) , %.6f %.6f ;; " % ((1,) + tuple(s[n] for n in order)))
