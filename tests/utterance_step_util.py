"""TEST INFRASTRUCTURE of tests/test_utterance_step_gpu.py and tools/utterance_step_f64dist.py: the stage-4 step on whole padded
utterances (train_gru_cyclevae_gauss_batch.py:1491-1653) on synthetic 16-field yields, for the device (stage4.Stage4Step through
stage4.utterance_step_args) and for the stock-torch checker (oracle/torch_stock.py, fp32 or float64) with the same dropout masks
(p = 0.5) and eps.

The cases: hu64 on pad_len = 2200 frames with three rows (the word-exchange recurrences, Bp = B) and five (one 16-row tile, M = 35200
rows through every GEMM and split); hu1024 at T = 200 / B = 2 and T = 96 / B = 5, the smallest that leave T = 80 behind on the
H = 1024 instances while the checker stays a matter of seconds.

Bounds.  Loss: 1e-5 relative (test_stage4_step_vs_cpu_checker's).  Gradients: relative to each tensor's largest entry,
TIGHT_REL = 8e-6 (tests/test_gpu_train.py) -- set at T <= 80.  tests/golden/utterance_step_f64dist.json holds, per case and tensor, the
distance of the checker's fp32 step from its own float64 step (tools/utterance_step_f64dist.py, computed on a CPU); by the rule of
frontend_util.bound_for a tensor whose distance exceeds TIGHT_REL / 4 is held to four times its distance, every other to TIGHT_REL.

Padding.  A frame of a pass's output depends on its input up to 4 frames ahead (the front-end's reach: kernel 3, dilations 1 and 3)
and on everything before (the recurrence).  The ten passes chain -- the deepest loss term, cycle 2's rec_cyc, is 8 passes from
batch_src -- so the loss of the frames [0, flens[j]) reads batch_src up to frame flens[j] - 1 + 8 * 4.  Refilling the padding from
flens[j] + 4 on does change the loss (as it does in the script); from flens[j] + PAD_REACH on, loss and every gradient must be
bit-identical: the loss weights there are zero, the reverse recurrences start from zero behind the last frame that reaches a loss
frame, and the weight-gradient sums only gain exact zeros."""
import json
import os

import numpy as np

import synth

TIGHT_REL = 8e-6               # tests/test_gpu_train.py
PAD_REACH = 8 * 4              # passes between batch_src and the deepest loss term x the front-end's reach
FLENS_2200 = (2200, 1501, 205)
CASES = {
    "hu64_b3_t2200": dict(hidden=64, B=3, T=2200, flens=FLENS_2200),
    "hu64_b5_t2200": dict(hidden=64, B=5, T=2200, flens=FLENS_2200 + (2200, 1501)),
    "hu1024_b2_t200": dict(hidden=1024, B=2, T=200, flens=(200, 113)),
    "hu1024_b5_t96": dict(hidden=1024, B=5, T=96, flens=(96, 77, 96, 40, 61)),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "utterance_step_f64dist.json")


def problem(name, refill=False):
    """(P, items, masks): the synthetic problem of a case, its 16-field yield (numpy; features, conversion features and codes zero
    behind an utterance's end, as the dataset pads) and the ten passes' masks.  refill: batch_src and batch_cv_src hold OTHER
    finite values of the features' law from frame flens[j] + PAD_REACH on."""
    c = CASES[name]
    kw = dict(B=c["B"], T=c["T"], hidden=c["hidden"], n_cyc=2, bias_scale=0.05, tag="uttstep/" + name)
    P = synth.CycleVAEProblem(**kw) if c["hidden"] >= 1024 else synth.CycleVAEProblem(in_dim=10, out_dim=6, lat_dim=4, **kw)
    x, cvx, cs, ct = P.x.copy(), P.cvx.copy(), P.code_src.copy(), P.code_trg.copy()
    other = synth.features("uttstep/%s/other" % name, P.B, P.T, P.mu, P.sigma)
    for j, n in enumerate(c["flens"]):
        for a in (x, cvx, cs, ct):
            a[j, n:] = 0.0
        if refill and n + PAD_REACH < P.T:
            x[j, n + PAD_REACH:] = other[j, n + PAD_REACH:]
            cvx[j, n + PAD_REACH:] = other[j, n + PAD_REACH:, :P.stdim]
    B = P.B
    spc = np.tile(np.arange(4, dtype=np.int64), (B, 1))
    files = ["/data/SF1/s%d.h5" % j for j in range(B)]
    files_trg = ["/data/TF1/s%d.h5" % j for j in range(B)]
    flens = np.array(c["flens"])
    items = (x, cs, ct, x[:, :8].copy(), cvx, 0, 0, spc, spc.copy(), files, files_trg, flens, np.full(B, 8), np.full(B, 4), np.full(B, 4), B)
    masks = {"enc": [], "dec": []}
    for kind, n, cin in (("enc", 4, P.in_dim), ("dec", 6, P.lat_dim + 2)):
        for i in range(n):
            cm = (synth.uniform01("uttstep/%s/%s%d/c" % (name, kind, i), (B, P.T, 9 * cin)) >= 0.5).astype(np.float32) * 2.0
            gm = (synth.uniform01("uttstep/%s/%s%d/g" % (name, kind, i), (P.T, B, P.hidden)) >= 0.5).astype(np.float32) * 2.0
            masks[kind].append((cm, gm))
    return P, items, masks


def checker_step(P, items, masks, dtype="float32"):
    """Loss and gradients of the step from the stock-torch checker on the CPU: the reference's ten separate passes
    (torch_stock.train_forward_t), stage4.chain_loss with the arguments of stage4.utterance_step_args."""
    import torch
    import stage4
    from oracle import torch_stock as ts
    dt = getattr(torch, dtype)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        leaf = {k: {n: t(v).requires_grad_(n in stage4.TRAINABLE) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}
        run_pass = lambda kind, x, y_in, clamp, mk: ts.train_forward_t(leaf[kind], x, y_in, t(mk[0]), t(mk[1]), clamp)
        kw = stage4.utterance_step_args(tuple(t(v) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v for v in items))
        kw.pop("carry")
        loss = stage4.chain_loss(run_pass, y_in_enc=t(P.y_in_enc), y_in_dec=t(P.y_in_dec), eps=t(P.eps), lat_dim=P.lat_dim, n_cyc=2,
                                 masks=masks, **kw)
        loss.backward()
        return float(loss.item()), {"%s/%s" % (k, n): leaf[k][n].grad.numpy().astype(np.float64) for k in leaf for n in stage4.TRAINABLE}
    finally:
        torch.set_default_dtype(old)


def device_step(P, items, masks, dev):
    """The same step through fresh drop-in modules and stage4.Stage4Step (fused, sync=True).  Returns (loss, {tensor: gradient},
    Stage4Step.fallbacks)."""
    import torch
    import gru_vae
    import stage4

    def mod(sd, i, o, enc):
        m = gru_vae.GRU_RNN(in_dim=i, out_dim=o, hidden_units=P.hidden, kernel_size=3, dilation_size=2, do_prob=0.5, scale_in_flag=enc,
                            scale_out_flag=not enc)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(dev).train()
    mods = {"enc": mod(P.enc, P.in_dim, 2 * P.lat_dim, True), "dec": mod(P.dec, P.lat_dim + 2, P.out_dim, False)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    step = stage4.Stage4Step(mods["enc"], mods["dec"], lat_dim=P.lat_dim, n_cyc=2, lr=1e-6)
    dm = {k: [(t(c), t(g)) for c, g in v] for k, v in masks.items()}
    kw = stage4.utterance_step_args(tuple(t(v) if isinstance(v, np.ndarray) and v.ndim >= 2 else v for v in items))
    loss = step(y_in_enc=t(P.y_in_enc), y_in_dec=t(P.y_in_dec), eps=t(P.eps), masks=dm, **kw)
    torch.cuda.synchronize()
    grads = {"%s/%s" % (k, n): dict(m.named_parameters())[n].grad.detach().cpu().numpy().copy() for k, m in mods.items() for n in stage4.TRAINABLE}
    return float(loss.item()), grads, step.fallbacks


def recorded(name):
    return os.path.join(os.path.dirname(GOLDEN), "utterance_step_%s.npz" % name)


def reference(name, P, items, masks):
    """The fp32 checker's (loss, gradients) of a case: recorded by tools/utterance_step_f64dist.py for the cases on 2200 frames (the
    checker walks them for ten seconds and more), computed here otherwise."""
    if os.path.exists(recorded(name)):
        g = np.load(recorded(name))
        return float(g["loss"]), {k.replace("__", "/"): g[k].astype(np.float64) for k in g.files if k != "loss"}
    return checker_step(P, items, masks, "float32")


def distance(a, ref):
    """max |a - ref| relative to the tensor's largest entry (tests/test_gpu_train.py's rel_err)."""
    return float(np.max(np.abs(a.astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def bounds(name):
    """{tensor: (bound, the checker's fp32-vs-float64 distance)} of a case by the rule of frontend_util.bound_for."""
    with open(GOLDEN) as f:
        d = json.load(f)[name]["grads"]
    return {k: ((4.0 * v if v > TIGHT_REL / 4 else TIGHT_REL), v) for k, v in d.items()}
