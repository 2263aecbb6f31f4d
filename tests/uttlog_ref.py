"""TEST INFRASTRUCTURE: numpy float64 restatement of what the stage-4 training loop does AROUND every step on utterance-length
mini-batches (train_gru_cyclevae_gauss_batch.py:705-706, :1476-1665; line numbers below are that script's), composed of
trainlog_ref.window_record (the nine figures of :1567-1582 are the window branch's figures with the whole utterance as the window),
oracle.dtw_org_to_trg and numpy: the yardstick of trainlog.UttLog.

PARITY UNPINNED for the dtw_org_to_trg / calc_mcd halves and float64 where the script reduces in fp32, as trainlog_ref states.

items: the generator's 16-field yield as numpy / host values.  trajs: the list over cycles of {"lat", "rec", "cv", "latcv", "reccyc"}
arrays [B, T, C] of the step's chain; lat_srctrg: the no-grad encoder pass over batch_src_trg with the weights before the step (:1490)."""
import numpy as np

from oracle import cyclevae_oracle as orc
import trainlog_ref as tref
from trainlog_ref import CLOSE_SRC, CLOSE_TRG, DB_SRC, DB_TRG, GV_SRC, GV_TRG, WIN_SRC, WIN_TRG, f64


class RefUttLog(tref.RefTrainLog):
    """The lists of the utterance branch and what is printed from them; epoch_end and the resets are the shared :719-739 and
    :1202-1269 of RefTrainLog."""

    def before(self, items):
        pass                                                   # (the sentinel: :707; the pass of :1490 is handed to after())

    def after(self, items, trajs, loss, lat_srctrg, sec=None):
        x, feat_trg, c_idx, spc, spc_trg, files, files_trg = items[0], items[3], items[5], items[7], items[8], items[9], items[10]
        flens, flens_trg, ns, nsp, B = items[11], items[12], items[13], items[14], int(items[15])
        sd = self.stdim
        for j in range(B):                                                                              # :1478
            self.lines.append("%s %s %d %d %d %d" % (files[j], files_trg[j], flens[j], flens_trg[j], ns[j], nsp[j]))
        t0 = trajs[0]
        for j in range(B):                                                                              # :1516
            n = int(flens[j])
            for name, k in zip(GV_SRC if self._is_src(files[j]) else GV_TRG, ("rec", "cv", "reccyc")):  # :1517-1524
                self.lists[name][0].append(np.var(f64(t0[k][j, :n, 1:]), axis=0))
            ix, ixp = spc[j, :int(ns[j])], spc_trg[j, :int(nsp[j])]
            par, own = f64(lat_srctrg[j][ixp]), f64(t0["lat"][j][ix])                                   # :1526-1527
            d1 = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(own, par)[0] - par) ** 2, axis=0)))        # :1528-1529
            c1 = orc.dtw_org_to_trg(par, own, mcd=0)[2]                                                 # :1530
            d2 = np.mean(np.sqrt(np.mean((orc.dtw_org_to_trg(par, own)[0] - own) ** 2, axis=0)))        # :1531-1532
            c2 = orc.dtw_org_to_trg(own, par, mcd=0)[2]                                                 # :1533
            trj, tgt = f64(t0["cv"][j][ix]), f64(feat_trg[j][:, sd:][ixp])
            mcdpow = orc.dtw_org_to_trg(trj, tgt)[2]                                                    # :1541
            mcd = orc.dtw_org_to_trg(trj[:, 1:], tgt[:, 1:])[2]                                         # :1542
            vals = (mcdpow, mcd, (d1 + d2) / 2, (c1 + c2) / 2)                                          # :1535-1536
            src = self._is_src(files[j])
            for name, v in zip(CLOSE_SRC if src else CLOSE_TRG, vals):                                  # :1549-1559
                self.lists[name][0].append(float(v))
            self.lines.append("batch %s loss %s %s = %.3f dB %.3f dB , %.3f %.3f " % (("srctrg" if src else "trgsrc", files[j], files_trg[j]) + vals))
        T = x.shape[1]
        R = tref.window_record(trajs, x, sd, self.L, spc, list(range(B)), flens, np.zeros(B, np.int64), np.asarray(ns, np.int64) - 1, 0)
        assert R.shape == (self.n_cyc, B, 9) and T >= max(int(n) for n in flens)
        for i in range(self.n_cyc):                                                                     # :1567-1627
            for j in range(B):
                src = self._is_src(files[j])
                for name, q in zip(DB_SRC if src else DB_TRG, (5, 6, 7, 8)):                            # :1600-1603 / :1612-1615
                    self.lists[name][i].append(float(R[i, j, q]))
                for name, q in zip(WIN_SRC if src else WIN_TRG, (0, 1, 2, 3, 4)):                       # :1605-1610 / :1617-1622
                    self.lists[name][i].append(float(R[i, j, q]))
        self.loss.append(float(loss))                                                                   # :1655
        text = "%.3f ;; " % float(loss)                                                                 # :1657-1662
        for i in range(self.n_cyc):
            text += "[%d] %.3f %.3f %.3f ; %.3f %.3f ; %.3f dB %.3f dB , %.3f dB %.3f dB;; " % (
                (i + 1,) + tuple(float(np.mean(R[i, :, q])) for q in range(9)))
        line = "batch loss [%d] = %s" % (c_idx + 1, text)                                               # :1663
        if sec is not None:
            line += "  (%.3f sec)" % sec
            self.total.append(sec)
        self.lines.append(line)
        self.iter_idx += 1
        self.iter_count += 1
        return R
