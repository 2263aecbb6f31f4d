"""TEST INFRASTRUCTURE shared by tests/test_uttlog_cpu.py (emulator build) and tests/test_uttlog_gpu.py (the device): the
end-to-end drive of trainlog.UttLog around stage4.Stage4Step on utterance-length mini-batches (the generator's 16-field yields),
with one body for both.  Yardstick: tests/uttlog_ref.py.  The batches are trainlog_util.e2e_batches: utterances of 23 / 17 / 9
frames with parallel utterances of 19 / 21 / 12, batch 0 of the source speaker and batch 1 of the target speaker."""
import numpy as np

import synth
import uttlog_ref as uref
from trainlog_util import H64, SLOTS, SPK_SRC, NpBackend, e2e_batches, host_items  # noqa: F401

WHOLE = ((0, None), (1, None))                       # (batch of e2e_batches, rows or None for all three): the two-batch case
SMALL = ((0, [1]), (1, None), (0, [0, 2]))           # one utterance; a full batch; a last batch smaller than y_in_pp (the `_mod` case)


def utt_yield(batch, c_idx, rows=None, put=lambda a: a):
    """The generator's 16-field yield of one utterance batch (loader.train_generator, batch_size == 0), cut to the utterances `rows`
    and to their longest length, as the collate pads a batch; put: host array -> device."""
    rows = list(range(len(batch["files"]))) if rows is None else list(rows)
    F, Ft = int(batch["flens"][rows].max()), int(batch["flens_trg"][rows].max())
    cut = lambda k, n: put(np.ascontiguousarray(batch[k][rows][:, :n]))
    pick = lambda k: [batch[k][j] for j in rows]
    return (cut("feat", F), cut("own", F), cut("other", F), cut("par", Ft), cut("cv", F), c_idx, c_idx, put(np.ascontiguousarray(batch["spc"][rows])),
            put(np.ascontiguousarray(batch["spc_trg"][rows])), pick("files"), pick("files_trg"), batch["flens"][rows], batch["flens_trg"][rows],
            batch["ns"][rows], batch["ns_trg"][rows], len(rows))


def sentinel():
    end = [[] for _ in range(16)]
    end[5] = end[6] = -1
    return tuple(end)


def drive(dev, seq=WHOLE, monitor=True, tag="ul/e2e", sync=True, dims=H64, drain_every_step=True):
    """The batches of `seq` and a sentinel through before / Stage4Step / after with injected eps and dropout masks.  Returns a dict:
    the monitor's lines and epoch summary, the reference's (run on the library's own trajectories and encoder pass), the records
    of both, and the parameters after the run."""
    import torch
    import stage4
    import trainlog
    from validation_util import modules
    P = synth.CycleVAEProblem(B=3, T=8, tag=tag, **dims)
    enc, dec = modules(P, dev)
    enc.train()
    dec.train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    real_step = dev.type == "cuda"
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-3, sync=sync) if real_step else None
    gv_src = synth.uniform(tag + "/gv_src", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    gv_trg = synth.uniform(tag + "/gv_trg", (P.out_dim - 1,), 0.5, 1.5).astype(np.float64)
    ul = trainlog.UttLog(enc, dec, P.lat_dim, P.stdim, gv_src, gv_trg, n_cyc=P.n_cyc, spk_src=SPK_SRC) if monitor else None
    ref = uref.RefUttLog(P.lat_dim, P.stdim, gv_src, gv_trg, n_cyc=P.n_cyc, spk_src=SPK_SRC)
    y_pp, y_dec = t(P.y_in_enc), t(P.y_in_dec)                 # three rows: a smaller batch is the script's `_mod` case
    batches = e2e_batches(P, tag)
    got_lines, records, ref_records, losses = [], [], [], []
    for k, (b, rows) in enumerate(seq):
        items = utt_yield(batches[b], k, rows, t)
        B, T = items[0].shape[0], items[0].shape[1]
        if monitor:
            ul.before(items, y_pp)
        eps = t(synth.normal("%s/eps%d" % (tag, k), (P.n_cyc, 3, B, T, P.lat_dim)))
        masks = {"enc": [], "dec": []}
        for kind, n, cin in (("enc", 2 * P.n_cyc, P.in_dim), ("dec", 3 * P.n_cyc, P.lat_dim + 2)):
            for i in range(n):
                cm = (synth.uniform01("%s/m%d/%s%d/c" % (tag, k, kind, i), (B, T, 9 * cin)) >= 0.5).astype(np.float32) * 2.0
                gm = (synth.uniform01("%s/m%d/%s%d/g" % (tag, k, kind, i), (T, B, P.hidden)) >= 0.5).astype(np.float32) * 2.0
                masks[kind].append((t(cm), t(gm)))
        if real_step:
            loss = step(y_in_enc=y_pp[:B], y_in_dec=y_dec[:B], eps=eps, masks=masks, **stage4.utterance_step_args(items))
            last_trajs = step.last_trajs
        else:
            # the emulated training step takes minutes: under emulation the monitor is driven with stand-in trajectories of the
            # chain's shapes and a stand-in loss (as trainlog_util.drive does); the real step drives it in tests/test_uttlog_gpu.py
            last_trajs = [{s: t(synth.normal("%s/trj%d/%d/%s" % (tag, k, i, s), (B, T, 2 * P.lat_dim if s in ("lat", "latcv") else P.out_dim)) * 0.5)
                           for s in SLOTS} for i in range(P.n_cyc)]
            loss = t(np.float32(100.0 + k))
        losses.append(float(loss))
        if monitor:
            ul.after(items, last_trajs, loss)
            records.append(ul.last_record.cpu().numpy().copy())
            trajs = [{s: v.detach().cpu().numpy() for s, v in tr.items()} for tr in last_trajs]
            ref_records.append(ref.after(host_items(items), trajs, float(loss), ul.last_lat_srctrg.cpu().numpy()))
            if drain_every_step:
                got_lines += ul.lines()
    summary = ref_summary = None
    if monitor:
        ul.before(sentinel(), y_pp)
        ref.before(sentinel())
        got_lines += ul.lines()
        summary, ref_summary = ul.epoch_end(), ref.epoch_end()
        got_lines += ul.lines()
    if real_step:
        step.finish()
    params = [p.detach().cpu().numpy().copy() for m in (enc, dec) for p in m.parameters()]
    return dict(lines=got_lines, ref_lines=ref.lines, summary=summary, ref_summary=ref_summary, records=records, ref_records=ref_records,
                params=params, ul=ul, losses=losses, fallbacks=step.fallbacks if real_step else 0)


def assert_figures(got, what=""):
    """The summary and every record against the restatement at 1e-10 relative (tests/test_trainlog_cpu.py's end-to-end tolerance),
    NaN exactly where the ref is NaN; every text line, and the epoch line, equal to the line formatted from the ref's numbers."""
    s, r = got["summary"], got["ref_summary"]
    assert set(s) == set(r)
    worst = 0.0
    for k, v in r.items():
        if k == "line":
            continue
        if np.isnan(v):
            assert np.isnan(s[k]), (k, s[k])
        else:
            worst = max(worst, abs(s[k] - v) / abs(v))
            assert abs(s[k] - v) <= 1e-10 * abs(v), (k, s[k], v)
    for a, b in zip(got["records"], got["ref_records"]):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        m = ~np.isnan(b)
        err = float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))
        worst = max(worst, err)
        assert err <= 1e-10, err
    print("%s: %d summary figures and %d records, max relative difference %.3e" % (what, len(r) - 1, len(got["records"]), worst))
    assert len(got["lines"]) == len(got["ref_lines"])
    for a, b in zip(got["lines"] + [s["line"]], got["ref_lines"] + [r["line"]]):
        assert a == b, "\n%s\n%s" % (a, b)


def check_e2e(dev):
    """Two utterance batches, one of each speaker: figures and lines against uttlog_ref; the six GV figures finite (the window
    branch prints nan behind a sentinel); on the device also the parameters against the same run without a monitor."""
    got = drive(dev)
    assert_figures(got, "two batches")
    s = got["summary"]
    gv = sorted(k for k in s if k.startswith("eval_gv_"))
    assert len(gv) == 6 and all(np.isfinite(s[k]) for k in gv), [(k, s[k]) for k in gv]
    assert all(np.isfinite(v) for k, v in s.items() if k != "line"), s
    L = got["lines"]
    assert len(L) == 2 * (3 + 3 + 1)                           # per step: three utterance lines, three alignment lines, the batch line
    assert sum(l.startswith("batch srctrg loss") for l in L) == 3 and sum(l.startswith("batch trgsrc loss") for l in L) == 3
    assert [l.split(" = ")[0] for l in L if l.startswith("batch loss")] == ["batch loss [1]", "batch loss [2]"]
    assert all(l.count(" dB") == 8 for l in L if l.startswith("batch loss"))      # (the dB part is always present: two cycles of four)
    assert L[0] == "/data/SF1/u00.h5 /data/TF1/u00.h5 23 19 10 %d" % int(e2e_batches(synth.CycleVAEProblem(B=3, T=8, tag="ul/e2e", **H64), "ul/e2e")[0]["ns_trg"][0])
    if dev.type != "cuda":
        return got
    blind = drive(dev, monitor=False)
    for a, b in zip(got["params"], blind["params"]):
        assert np.array_equal(a, b), "the monitor changed a parameter"
    return got
