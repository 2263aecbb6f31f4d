"""TEST INFRASTRUCTURE shared by tests/test_trainlog_cpu.py (emulator build, numpy memory) and tests/test_trainlog_gpu.py (the
device): the kernel-alone fixture of cvae_trainlog_window and the end-to-end drive of trainlog.TrainLog around stage4.Stage4Step,
with runners that take a `backend` / a device so that one body serves both.  Yardstick: tests/trainlog_ref.py."""
import ctypes as C

import numpy as np

import _cabi
import synth
import windows
import trainlog_ref as tref
from validation_util import NpBackend, TorchBackend  # noqa: F401  (the two memories)

SLOTS = _cabi.TRAINLOG_SLOTS

# ---- (a) the kernel alone ------------------------------------------------------------------------------------------------------

A_DIMS = dict(n_cyc=2, D=26, L=8, stdim=4, batch_size=8)
A_FLENS = (23, 17, 9)
A_SPC = ((2, 3, 4, 5, 6, 17, 18, 19, 20, 21), (0, 1, 2, 3, 9, 10, 16), (4, 5, 6))


def kernel_problem(tag="tl/a", flens=A_FLENS, spc=A_SPC, **dims):
    """Three utterances in 8-frame windows: synthetic fp32 trajectories per window, the padded feature batch, the speech-frame
    index rows and the generator's bookkeeping (windows.iter_windows).  Returns (d, batch_src, spcidx, [window dicts])."""
    d = dict(A_DIMS)
    d.update(dims)
    B, F = len(flens), max(flens)
    x = (synth.normal(tag + "/x", (B, F, d["stdim"] + d["D"])) * 0.8).astype(np.float32)
    idx = np.zeros((B, max(len(s) for s in spc)), np.int64)
    for j, s in enumerate(spc):
        idx[j, :len(s)] = s
    wins = []
    for w, (s, e, s_idx, e_idx, sel, facc) in enumerate(windows.iter_windows(np.array(flens), idx, np.array([len(s) for s in spc]), d["batch_size"])):
        T = e - s + 1
        trajs = []
        for i in range(d["n_cyc"]):
            tr = {}
            for k in SLOTS:
                C_ = 2 * d["L"] if k in ("lat", "latcv") else d["D"]
                tr[k] = (synth.normal("%s/w%d/c%d/%s" % (tag, w, i, k), (B, T, C_)) * 0.7).astype(np.float32)
            trajs.append(tr)
        wins.append(dict(s=s, e=e, T=T, s_idx=np.array(s_idx), e_idx=np.array(e_idx), sel=list(sel), flen_acc=np.array(facc), trajs=trajs))
    return d, x, idx, wins


def window_args(be, d, dev, x, spc, w, acc, out, keep, rows=None):
    """TrainlogWindowArgs of window dict w over device copies; rows: the utterances (a list) to run, in that order."""
    rows = list(range(x.shape[0])) if rows is None else rows
    B = len(rows)
    a = _cabi.TrainlogWindowArgs()
    for i, tr in enumerate(w["trajs"]):
        for k, name in enumerate(SLOTS):
            t = be.put(tr[name][rows])
            keep.append(t)
            a.traj[i][k] = be.ptr(t)
    xw = be.put(x[rows][:, w["s"]:w["e"] + 1])
    sp = be.put(spc[rows])
    sel = np.array([1 if j in w["sel"] else 0 for j in rows], np.uint8)
    host = [np.ascontiguousarray(w[k][rows], np.int32) for k in ("flen_acc", "s_idx", "e_idx")] + [sel]
    keep += [xw, sp] + host
    a.x_win, a.x_row_stride, a.x_utt_stride = be.ptr(xw), x.shape[2], w["T"] * x.shape[2]
    a.spcidx, a.spc_ld = be.ptr(sp), spc.shape[1]
    a.flen_acc, a.s_idx, a.e_idx, a.selected = (h.ctypes.data for h in host)
    a.n_cyc, a.B, a.T, a.D, a.L, a.stdim, a.src_idx_s = d["n_cyc"], B, w["T"], d["D"], d["L"], d["stdim"], w["s"]
    if acc is not None:
        a.acc_rows = x.shape[1]
        for q in range(4):
            a.acc[q] = be.ptr(acc[q])
    a.rec_out = be.ptr(out)
    return a


def run_kernel_windows(be, d, x, spc, wins, rows=None, with_acc=True):
    """Every window through cvae_trainlog_window.  Returns ([records [n_cyc, B, 9]], {rec, cv, reccyc, lat: accumulator} or None)."""
    rows_ = list(range(x.shape[0])) if rows is None else rows
    B, F = len(rows_), x.shape[1]
    acc = None
    if with_acc:
        acc = [be.empty((B, F, d["D"]), np.float32) for _ in range(3)] + [be.empty((B, F, 2 * d["L"]), np.float32)]
    recs, keep = [], []
    for w in wins:
        out = be.empty((d["n_cyc"], B, 9), np.float64)
        be.lib.trainlog_window(window_args(be, d, None, x, spc, w, acc, out, keep, rows), be.stream)
        recs.append(be.get(out))
    return recs, (None if acc is None else dict(zip(("rec", "cv", "reccyc", "lat"), (be.get(a) for a in acc))))


def ref_records(d, x, spc, wins):
    return [tref.window_record(w["trajs"], x[:, w["s"]:w["e"] + 1], d["stdim"], d["L"], spc, w["sel"], w["flen_acc"], w["s_idx"], w["e_idx"], w["s"])
            for w in wins]


def assert_records(got, want, what):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern\n%s\n%s" % (what, np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    err = np.abs(got[m] - want[m]) / np.abs(want[m])
    print("%s: %d figures, max relative difference %.3e" % (what, int(m.sum()), float(err.max()) if err.size else 0.0))
    assert np.all(err <= 1e-12), (what, float(err.max()))


def check_kernel_alone(be):
    """(a): every record entry against trainlog_ref at 1e-12 relative, NaN exactly where the ref is NaN; the accumulators bit-equal
    to the concatenated windows; the windows are the ones the issue's table lists."""
    d, x, spc, wins = kernel_problem()
    assert [(w["s"], w["e"]) for w in wins] == [(0, 7), (8, 15), (16, 22)]
    assert wins[0]["sel"] == [0, 1, 2] and all(wins[0]["s_idx"] >= 0)
    assert wins[1]["sel"] == [0, 1] and wins[1]["s_idx"][0] == -1 and wins[1]["s_idx"][2] >= 0       # (utterance 2: stale bookkeeping)
    assert wins[2]["T"] == 7 and list(wins[2]["flen_acc"]) == [8, 1, 8]
    recs, acc = run_kernel_windows(be, d, x, spc, wins)
    want = ref_records(d, x, spc, wins)
    for k, (g, r) in enumerate(zip(recs, want)):
        assert_records(g, r, "window %d" % k)
    # what each window must have exercised
    assert np.all(np.isnan(recs[1][:, 2, :])) and np.all(np.isnan(recs[1][:, 0, 5:])) and np.all(np.isfinite(recs[1][:, 0, :5]))
    assert np.all(np.isfinite(recs[0])) and np.all(np.isfinite(recs[2][:, :2, :5]))
    for k, name in (("rec", "rec"), ("cv", "cv"), ("reccyc", "reccyc"), ("lat", "lat")):
        cat = np.concatenate([w["trajs"][0][name] for w in wins], axis=1)
        assert np.array_equal(acc[k], cat), "accumulator " + k
    return d, x, spc, wins, recs


def check_bad_index(be):
    """One speech index pointing outside the window: NaN for that utterance's four figures, and for nothing else."""
    d, x, spc, wins = kernel_problem()
    good, _ = run_kernel_windows(be, d, x, spc, wins[:1], with_acc=False)
    bad = spc.copy()
    bad[1, 2] = 11                      # utterance 1, window (0, 7): frames 0, 1, 11, 3
    got, _ = run_kernel_windows(be, d, x, bad, wins[:1], with_acc=False)
    assert np.all(np.isnan(got[0][:, 1, 5:]))
    keep = np.ones(got[0].shape, bool)
    keep[:, 1, 5:] = False
    assert np.array_equal(got[0][keep], good[0][keep]) and np.all(np.isfinite(got[0][keep]))
    bad[1, 2] = -3
    got, _ = run_kernel_windows(be, d, x, bad, wins[:1], with_acc=False)
    assert np.all(np.isnan(got[0][:, 1, 5:])) and np.array_equal(got[0][keep], good[0][keep])
    assert_records(got[0], ref_records(d, x, bad, wins[:1])[0], "bad index")


def check_grid_independence(be):
    """The utterance rows permuted, and one utterance alone: bit-identical per-utterance records."""
    d, x, spc, wins = kernel_problem()
    base, _ = run_kernel_windows(be, d, x, spc, wins, with_acc=False)
    for rows in ([2, 0, 1], [1]):
        got, _ = run_kernel_windows(be, d, x, spc, wins, rows=rows, with_acc=False)
        for g, b in zip(got, base):
            assert np.array_equal(g, b[:, rows], equal_nan=True), rows


def check_refusals(be):
    d, x, spc, wins = kernel_problem()
    import pytest
    keep = []
    out = be.empty((d["n_cyc"], 3, 9), np.float64)
    acc = [be.empty((3, 12, d["D"]), np.float32) for _ in range(3)] + [be.empty((3, 12, 2 * d["L"]), np.float32)]
    a = window_args(be, d, None, x, spc, wins[1], acc, out, keep)
    a.acc_rows = 12                      # rows 8 .. 15 do not fit
    with pytest.raises(_cabi.CvaeError):
        be.lib.trainlog_window(a, be.stream)
    a = window_args(be, d, None, x, spc, wins[0], None, out, keep)
    a.n_cyc = _cabi.TRAINLOG_MAX_CYC + 1
    with pytest.raises(_cabi.CvaeError):
        be.lib.trainlog_window(a, be.stream)


# ---- (b) TrainLog end to end ---------------------------------------------------------------------------------------------------

H64 = dict(in_dim=30, out_dim=26, lat_dim=8, hidden=64, n_cyc=2, bias_scale=0.1)
SPK_SRC = "SF1"


def e2e_batches(P, tag):
    """Two utterance batches of the (a) geometry as the generator's fields: batch 0 of the source speaker, batch 1 of the target
    speaker (other lengths for the parallel utterances)."""
    out = []
    for b, spk in enumerate((SPK_SRC, "TF1")):
        B, F = len(A_FLENS), max(A_FLENS)
        flens_trg = (19, 21, 12)
        feat = synth.features("%s/b%d/feat" % (tag, b), B, F, P.mu, P.sigma)
        par = synth.features("%s/b%d/par" % (tag, b), B, max(flens_trg), P.mu, P.sigma)
        cv = synth.features("%s/b%d/cv" % (tag, b), B, F, P.mu[:P.stdim], P.sigma[:P.stdim])
        own, other = synth.onehot_codes(B, F, src_is_first=(b == 0))
        spc = np.zeros((B, max(len(s) for s in A_SPC)), np.int64)
        for j, s in enumerate(A_SPC):
            spc[j, :len(s)] = s
        spc_trg = np.zeros((B, 12), np.int64)
        ns_trg = []
        for j, n in enumerate(flens_trg):
            keep = np.nonzero(synth.uniform01("%s/b%d/spcp%d" % (tag, b, j), (n,)) < 0.6)[0]
            keep = keep[:12] if len(keep) > 1 else np.arange(2)
            spc_trg[j, :len(keep)] = keep
            ns_trg.append(len(keep))
            par[j, n:] = 0
        for j, n in enumerate(A_FLENS):
            for a in (feat, cv, own, other):
                a[j, n:] = 0
        files = ["/data/%s/u%d%d.h5" % (spk, b, j) for j in range(B)]
        files_trg = ["/data/%s/u%d%d.h5" % ("TF1" if b == 0 else SPK_SRC, b, j) for j in range(B)]
        out.append(dict(feat=feat, own=own, other=other, par=par, cv=cv, spc=spc, spc_trg=spc_trg, files=files, files_trg=files_trg,
                        flens=np.array(A_FLENS), flens_trg=np.array(flens_trg), ns=np.array([len(s) for s in A_SPC]), ns_trg=np.array(ns_trg)))
    return out


def yields(batch, batch_size=8, put=lambda a: a):
    """The generator's 22-field yields of one utterance batch (loader.train_generator, batch_size > 0); put: host array -> device."""
    dev = {k: put(batch[k]) for k in ("feat", "own", "other", "par", "cv", "spc", "spc_trg")}
    for s, e, s_idx, e_idx, sel, facc in windows.iter_windows(batch["flens"], batch["spc"], batch["ns"], batch_size):
        yield (dev["feat"], dev["own"][:, s:e + 1], dev["other"][:, s:e + 1], dev["par"], dev["cv"], s, e, s_idx, e_idx, 0, 0, dev["spc"],
               dev["spc_trg"], batch["files"], batch["files_trg"], batch["flens"], batch["flens_trg"], batch["ns"], batch["ns_trg"], sel, facc,
               len(batch["files"]))


def sentinel():
    end = [[] for _ in range(22)]
    end[9] = end[10] = -1
    return tuple(end)


def host_items(items):
    """The same yield with numpy arrays (what trainlog_ref reads)."""
    return tuple(v.cpu().numpy() if hasattr(v, "cpu") else v for v in items)


def drive(dev, with_sentinel, monitor=True, P=None, tag="tl/e2e", sync=True, dims=H64, batch_size=8, drain_every_step=True):
    """Both batches through before / Stage4Step / after with injected eps and dropout masks.  Returns a dict: the monitor's lines and
    epoch summaries, the reference's (run on the library's own trajectories), and the parameters after the run."""
    import torch
    import stage4
    import trainlog
    from validation_util import modules
    P = P or synth.CycleVAEProblem(B=len(A_FLENS), T=batch_size, tag=tag, **dims)
    enc, dec = modules(P, dev)
    enc.train()
    dec.train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    real_step = dev.type == "cuda"
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-3, sync=sync) if real_step else None
    gv_src = synth.uniform(tag + "/gv_src", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    gv_trg = synth.uniform(tag + "/gv_trg", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, gv_src, gv_trg, n_cyc=P.n_cyc, spk_src=SPK_SRC) if monitor else None
    ref = tref.RefTrainLog(P.lat_dim, P.stdim, gv_src, gv_trg, n_cyc=P.n_cyc, spk_src=SPK_SRC)
    y_pp, y_dec = t(P.y_in_enc), t(P.y_in_dec)
    got_lines, summaries, ref_summaries = [], [], []
    seq = []
    for b, batch in enumerate(e2e_batches(P, tag)):
        seq += list(yields(batch, batch_size, t))
        if with_sentinel or b == 1:
            seq.append(sentinel())
    carry, n_win = None, 0
    for items in seq:
        end = items[9] < 0
        if monitor:
            tl.before(items, y_pp)
            ref.before(host_items(items), None if tl.last_lat_srctrg is None else tl.last_lat_srctrg.cpu().numpy())
        if end:
            if monitor:
                got_lines += tl.lines()
                summaries.append(tl.epoch_end())
                ref_summaries.append(ref.epoch_end())
            carry = None
            continue
        x, s, e = items[0], items[5], items[6]
        T = e - s + 1
        if s == 0:
            carry = None
        B = x.shape[0]
        eps = t(synth.normal("%s/eps%d" % (tag, n_win), (P.n_cyc, 3, B, T, P.lat_dim)))
        masks = {"enc": [], "dec": []}
        for kind, n, cin in (("enc", 2 * P.n_cyc, P.in_dim), ("dec", 3 * P.n_cyc, P.lat_dim + 2)):
            for i in range(n):
                cm = (synth.uniform01("%s/m%d/%s%d/c" % (tag, n_win, kind, i), (B, T, 9 * cin)) >= 0.5).astype(np.float32) * 2.0
                gm = (synth.uniform01("%s/m%d/%s%d/g" % (tag, n_win, kind, i), (T, B, P.hidden)) >= 0.5).astype(np.float32) * 2.0
                masks[kind].append((t(cm), t(gm)))
        if real_step:
            loss, carry = step(x[:, s:e + 1], items[4][:, s:e + 1], items[1], items[2], y_pp, y_dec, eps, masks=masks,
                               flen_acc=[int(v) for v in items[20]], select_utt_idx=list(items[19]), carry=carry, return_state=True)
            last_trajs = step.last_trajs
        else:
            # the emulated training step takes minutes at any size: under emulation the monitor is driven with stand-in
            # trajectories of the chain's shapes and a stand-in loss; the real step drives it in tests/test_trainlog_gpu.py
            last_trajs = [{k: t(synth.normal("%s/trj%d/%d/%s" % (tag, n_win, i, k), (B, T, 2 * P.lat_dim if k in ("lat", "latcv") else P.out_dim)) * 0.5)
                           for k in SLOTS} for i in range(P.n_cyc)]
            loss = t(np.float32(100.0 + n_win))
        if monitor:
            tl.after(items, last_trajs, loss)
            trajs = [{k: v.detach().cpu().numpy() for k, v in tr.items()} for tr in last_trajs]
            ref.after(host_items(items), trajs, float(loss))
            if drain_every_step:
                got_lines += tl.lines()
        n_win += 1
    if monitor:
        got_lines += tl.lines()
    if real_step:
        step.finish()
    params = [p.detach().cpu().numpy().copy() for m in (enc, dec) for p in m.parameters()]
    return dict(lines=got_lines, ref_lines=ref.lines, summaries=summaries, ref_summaries=ref_summaries, params=params, tl=tl)


def check_e2e(dev, with_sentinel):
    """(b): the monitor's figures against trainlog_ref on the library's own trajectories at 1e-10 relative, its text lines against
    the lines formatted from the ref's numbers, and the parameters against the same run without a monitor (bit-identical)."""
    got = drive(dev, with_sentinel)
    assert len(got["summaries"]) == (2 if with_sentinel else 1)
    for s, r in zip(got["summaries"], got["ref_summaries"]):
        assert set(s) == set(r)
        for k, v in r.items():
            if k == "line":
                continue
            if np.isnan(v):
                assert np.isnan(s[k]), (k, s[k])
            else:
                assert abs(s[k] - v) <= 1e-10 * abs(v), (k, s[k], v)
    gv = [k for k in got["ref_summaries"][-1] if k.startswith("eval_gv_")]
    fired = [k for k in gv if np.isfinite(got["ref_summaries"][-1][k])]
    # the GV rule of :1339-1348 needs a second utterance batch in ONE pass: never with a sentinel between the batches
    assert fired == ([] if with_sentinel else ["eval_gv_src_src", "eval_gv_src_trg", "eval_gv_src_trg_src"]), fired
    assert len(got["lines"]) == len(got["ref_lines"]) == 6 + 6       # six windows, three utterances closed twice
    for a, b in zip(got["lines"] + [s["line"] for s in got["summaries"]], got["ref_lines"] + [s["line"] for s in got["ref_summaries"]]):
        assert a == b, "\n%s\n%s" % (a, b)
    assert sum(l.startswith("batch srctrg loss") for l in got["lines"]) == 3 and sum(l.startswith("batch trgsrc loss") for l in got["lines"]) == 3
    assert all(" dB " in l for l in got["lines"] if l.startswith("batch loss"))                # (print_mcd_flag: every window holds a speech frame)
    if dev.type != "cuda":
        return                                # (no step under emulation: see drive)
    blind = drive(dev, with_sentinel, monitor=False)
    for a, b in zip(got["params"], blind["params"]):
        assert np.array_equal(a, b), "the monitor changed a parameter"
