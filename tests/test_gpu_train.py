"""GPU tests of the training path through the drop-in module: train-mode passes and their autograd backward against
gradients recorded from the reference, and a whole stage-4 step (cyc2 chain + loss + backward + Adam) against the
stock-torch CPU checker with identical dropout masks and eps.

Tolerances: outputs and gradients relative to each tensor's largest entry, TIGHT_REL = 8e-6 everywhere (fp32, sums over thousands
of terms in different summation orders; measured 7e-8 .. 3.0e-6); loss 1e-5 relative (2e-6 in the window-by-window test).
"""
import os

import numpy as np
import pytest

import _cabi
import synth
from train_util import TRAINABLE, chain_loss, cpu_step, make_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "gpurun_out", "gpu_parity_report.txt")


def note(msg):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(msg + "\n")
    print(msg)


# Regression-grade tolerance of every comparison against recorded reference gradients / the stock-torch checker: relative error
# (max|d| / max|ref|) of outputs, carried state, dx and every parameter gradient.  Measured on the MI355X: 7e-8 .. 3.0e-6 (the
# largest: dW_hh at hu2048, 5120 rows contracted in another order than torch's).  The old bounds (1e-4 .. 1e-3) would have let a
# 100x loss of accuracy through.
TIGHT_REL = 8e-6


def rel_err(a, ref, name):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    assert np.all(np.isfinite(a)), name
    e = float(np.max(np.abs(a.astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))
    note("%-48s rel err = %.3e" % (name, e))
    return e


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


def module(gv, sd, i, o, h, enc, dev, do_prob=0.5):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, kernel_size=3, dilation_size=2, do_prob=do_prob, scale_in_flag=enc,
                   scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).train()
    for n, p in m.named_parameters():
        p.requires_grad_(n in TRAINABLE)     # scale_in / scale_out frozen (train...:369-372)
    return m


@pytest.mark.parametrize("tag,hid,B,T", [("train_h32", 32, 3, 10), ("train_h64", 64, 18, 7)])
def test_train_pass_autograd_vs_reference(gv, dev, golden, tag, hid, B, T):
    g = golden(tag)
    P = synth.CycleVAEProblem(B=B, T=T, in_dim=6, out_dim=4, lat_dim=4, hidden=hid, n_cyc=1, bias_scale=0.1, tag=tag)
    x_dec = np.concatenate([P.code_src, synth.normal(tag + "/z", (B, T, 4))], 2)
    x2 = synth.features(tag + "/x2", B, T, P.mu, P.sigma)
    enc, dec = module(gv, P.enc, 6, 8, hid, True, dev), module(gv, P.dec, 6, 4, hid, False, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cases = [("enc", enc, P.x, P.y_in_enc, None, True), ("dec", dec, x_dec, P.y_in_dec, None, False),
             ("enc2", enc, x2, g["enc_y_last"], g["enc_h_last"], True)]
    for name, m, x, y_in, h_in, clamp in cases:
        for p in m.parameters():
            p.grad = None
        cot = synth.normal(tag + "/cot_" + name.replace("2", ""), (B, T, m.out_dim))
        xt = t(x).requires_grad_(True)
        m._debug_masks = (t(g[name + "_cmask"]), t(g[name + "_gmask"]))
        out, yl, hl = m(xt, t(y_in), h_in=None if h_in is None else t(h_in), do=True, clamp_vae=clamp, lat_dim=4)
        assert not yl.requires_grad and not hl.requires_grad
        (out * t(cot)).sum().backward()
        assert rel_err(out, g[name + "_out"], tag + " " + name + " out") <= TIGHT_REL
        assert rel_err(hl, g[name + "_h_last"], tag + " " + name + " h_last") <= TIGHT_REL
        assert rel_err(xt.grad, g[name + "_dx"], tag + " " + name + " dx") <= TIGHT_REL
        for k in TRAINABLE:
            assert rel_err(dict(m.named_parameters())[k].grad, g[name + "_g_" + k], tag + " " + name + " d" + k) <= TIGHT_REL
        assert m.scale_in.weight.grad is None if name.startswith("enc") else m.scale_out.weight.grad is None


@pytest.mark.parametrize("hid,B,T,stack,ncyc", [(64, 4, 12, False, 2), (1024, 2, 16, False, 2), (64, 50, 6, False, 2), (2048, 2, 5, False, 2),
                                                (64, 4, 12, True, 2), (1024, 12, 16, True, 2), (64, 50, 6, True, 2), (2048, 2, 4, True, 4),
                                                (1024, 1, 40, True, 2)])
# 50 rows: 4 row tiles, split GEMMs; 2048: stress config dims (BASELINE configs[4]; the last case with its n_cyc = 4: 8 encoder + 12
# decoder passes; the full-size single pass is test_train_pass_full_size_hu2048 -- the CPU checker needs 8 minutes for a full-window
# cyc4 step); (1024, 1, 40): the recipe's own batch of ONE utterance, every pass on the word-exchange recurrences; stack: rec || cv as one decoder launch of 2B rows
def test_stage4_step_vs_cpu_checker(gv, dev, hid, B, T, stack, ncyc):
    """cyc2 chain in train mode (dropout 0.5) + loss + backward + Adam through the drop-in modules vs stock torch on CPU
    (the checker always runs the reference's ten separate passes)."""
    big = hid >= 1024
    kw = dict(B=B, T=T, hidden=hid, n_cyc=ncyc, bias_scale=0.05, tag="step%d_%d" % (hid, ncyc))
    if hid == 2048:      # BASELINE configs[4] dims (hu2048 / ld64): the any-H kernels (per-step launches) carry this size
        P = synth.CycleVAEProblem(lat_dim=64, **kw)
    else:
        P = synth.CycleVAEProblem(**kw) if big else synth.CycleVAEProblem(in_dim=10, out_dim=6, lat_dim=4, **kw)
    masks = make_masks(P, 2 * ncyc, 3 * ncyc)
    ref_loss, ref_grads = cpu_step(P, masks, ncyc)
    ed, eo, dd, do_ = (54, 128, 66, 50) if hid == 2048 else ((54, 64, 34, 50) if big else (10, 8, 6, 6))
    enc, dec = module(gv, P.enc, ed, eo, hid, True, dev), module(gv, P.dec, dd, do_, hid, False, dev)
    mods = {"enc": enc, "dec": dec}

    def run_pass(kind, x, y_in, clamp, mk):
        m = mods[kind.rstrip("2")]
        m._debug_masks = (torch.from_numpy(mk[0]).to(dev), torch.from_numpy(mk[1]).to(dev))
        return m(x, y_in, do=True, clamp_vae=clamp >= 0, lat_dim=P.lat_dim)[0]

    opt = torch.optim.Adam([p for m in mods.values() for p in m.parameters() if p.requires_grad], lr=1e-4)
    opt.zero_grad()
    loss = chain_loss(run_pass, P, dev, masks, ncyc, stack_rec_cv=stack)
    loss.backward()
    note("stage-4 step hu%d cyc%d: loss gpu %.6f cpu %.6f" % (hid, ncyc, loss.item(), ref_loss))
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    for kind, m in mods.items():
        for k in TRAINABLE:
            gr = dict(m.named_parameters())[k].grad
            assert rel_err(gr, ref_grads[kind][k], "step hu%d %s d%s" % (hid, kind, k)) <= TIGHT_REL
    before = {k: v.detach().clone() for k, v in enc.named_parameters()}
    opt.step()
    # Adam's first step moves every trainable entry with a non-zero gradient by ~lr; frozen layers stay put
    assert torch.equal(before["scale_in.weight"], enc.scale_in.weight)
    d = (enc.gru.weight_hh_l0.detach() - before["gru.weight_hh_l0"]).abs()
    assert 0.5e-4 < d.max().item() <= 1.01e-4
    # the next forward sees the updated weights (train image is rebuilt)
    loss2 = chain_loss(run_pass, P, dev, masks, ncyc, stack_rec_cv=stack)
    assert loss2.item() < loss.item()


@pytest.mark.parametrize("stack", [False, True], ids=["ten_passes", "rec_cv_stacked"])
def test_two_reference_recorded_steps(gv, dev, golden, stack):
    """tests/golden/stage4_step.npz: two consecutive stage-4 steps executed by the reference's own statements (forward
    :1298-1354 with the fresh-window and the carry branch, loss :1356-1410 with ragged flen_acc / select_utt_idx, update
    :1418-1420).  The drop-in modules + stage4.chain_loss + torch.optim.Adam must land on the same losses, gradients and
    post-step weights."""
    import train_util
    g = golden("stage4_step")
    P, x, cvx = train_util.golden_step_problem(g)
    mods = {"enc": module(gv, P.enc, 10, 8, 32, True, dev), "dec": module(gv, P.dec, 6, 6, 32, False, dev)}
    opt = torch.optim.Adam([p for k in ("enc", "dec") for p in mods[k].parameters() if p.requires_grad], lr=1e-4)

    def run_pass(kind, xin, y_in, clamp, mk, h_in=None):
        m = mods[kind.rstrip("2")]
        m._debug_masks = (torch.from_numpy(mk[0]).to(dev), torch.from_numpy(mk[1]).to(dev))
        return m(xin, y_in, h_in=h_in, do=True, clamp_vae=clamp >= 0, lat_dim=P.lat_dim)

    for w, loss, trajs in train_util.run_golden_windows(g, P, x, cvx, run_pass, opt, dev, stack):
        ref_loss = float(g["w%d_loss" % w])
        note("reference-recorded step %d: loss gpu %.6f reference %.6f" % (w, loss.item(), ref_loss))
        assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
        for kind in ("enc", "dec"):
            for n in TRAINABLE:
                gr = dict(mods[kind].named_parameters())[n].grad
                ref_norm = float(g["w%d_%s_gnorm_%s" % (w, kind, n)])
                assert abs(float(gr.double().norm()) - ref_norm) <= 1e-3 * ref_norm, (w, kind, n)
                # every gradient tensor of BOTH windows (window 1: the carry branch, on the weights window 0's update left)
                assert rel_err(gr, g["w%d_%s_g_%s" % (w, kind, n)], "recorded step, window %d: %s d%s" % (w, kind, n)) <= TIGHT_REL
    for kind in ("enc", "dec"):
        for n in TRAINABLE:
            v = dict(mods[kind].named_parameters())[n].detach().double().cpu().numpy()
            got = np.array([v.sum(), (v * v).sum(), v.ravel()[0], v.ravel()[-1]])
            assert np.allclose(got, g["w1_%s_after_%s" % (kind, n)], rtol=2e-5, atol=2e-6), (kind, n)


def test_train_pass_full_window_hu1024(gv, dev):
    """BASELINE configs[2] shape: ONE train-mode encoder pass over a full 80-frame window at hu1024 (the 80-step persistent
    train recurrence and its tape) against the stock-torch checker, forward and every gradient."""
    from oracle import torch_stock as ts
    B, T = 4, 80
    P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="train80")
    masks = make_masks(P, 1, 0, tag="train80m")["enc"][0]
    cot = synth.normal("train80/cot", (B, T, 64))
    out_r, _, h_r, Pr, xr = ts.train_forward(P.enc, P.x, P.y_in_enc, None, masks[0], masks[1], 32)
    (out_r * torch.from_numpy(cot)).sum().backward()
    enc = module(gv, P.enc, 54, 64, 1024, True, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = t(P.x).requires_grad_(True)
    enc._debug_masks = (t(masks[0]), t(masks[1]))
    out, yl, hl = enc(xt, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=32)
    (out * t(cot)).sum().backward()
    assert rel_err(out, out_r.detach().numpy(), "train T=80 hu1024 out") <= TIGHT_REL
    assert rel_err(hl[0], h_r.detach().numpy(), "train T=80 hu1024 h_last") <= TIGHT_REL
    assert rel_err(xt.grad, xr.grad.numpy(), "train T=80 hu1024 dx") <= TIGHT_REL
    for k in TRAINABLE:
        assert rel_err(dict(enc.named_parameters())[k].grad, Pr[k].grad.numpy(), "train T=80 hu1024 d" + k) <= TIGHT_REL


def test_adam_step_kernel_vs_torch(gv, dev):
    """cvae_adam_step (torch.optim.Adam semantics, reference train...:377 / :1420) on the device against torch.optim.Adam for
    three consecutive steps, sizes that are not multiples of the block."""
    lib = gv._lib()
    for n in (1, 1000, 3 * 1024 * 1024 + 17):
        p0 = torch.from_numpy(synth.normal("adam/p%d" % n, (n,))).to(dev)
        p_ref = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p_ref], lr=1e-4)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for step in (1, 2, 3):
            g = torch.from_numpy(synth.normal("adam/g%d_%d" % (n, step), (n,))).to(dev) * (0.1 if step == 2 else 3.0)
            p_ref.grad = g.clone()
            opt.step()
            lib.adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-4, 0.9, 0.999, 1e-8, step,
                          torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            d = float(((p - p_ref.detach()).abs() / p_ref.detach().abs().clamp(min=1.0)).max())
            assert d <= 2.4e-7, (n, step, d)           # one fp32 ulp: torch applies the bias corrections in another order


def test_dropout_masks_keyed_by_global_row(gv, dev):
    """Train-mode passes with on-device Philox masks: rows 20..39 of a 40-row job, run alone with the draw origin set, see the
    masks they would see inside the 40-row batch (same seed from torch's generator)."""
    P = synth.CycleVAEProblem(B=40, T=10, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=1, bias_scale=0.1, tag="origin_t")
    enc = module(gv, P.enc, 10, 8, 64, True, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        with torch.no_grad():
            gv.set_draw_origin(0, 40, 10)
            torch.manual_seed(5)
            whole = enc(t(P.x), t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=4)[0]
            gv.set_draw_origin(20, 40, 10)
            torch.manual_seed(5)
            hi = enc(t(P.x[20:]), t(P.y_in_enc[20:]), do=True, clamp_vae=True, lat_dim=4)[0]
            gv.set_draw_origin(0, 0, 0)
            torch.manual_seed(5)
            hi_local = enc(t(P.x[20:]), t(P.y_in_enc[20:]), do=True, clamp_vae=True, lat_dim=4)[0]
        torch.cuda.synchronize()
        d = float((whole[20:] - hi).abs().max())
        note("global-row masks: rows 20..39 alone vs inside the 40-row batch max|d| = %.3e" % d)
        assert d <= 1e-5                                   # same masks; GEMM tilings differ with the batch size
        assert float((hi - hi_local).abs().max()) > 1e-3   # numbered from 0 they draw other masks
        # two stacked copies (rec || cv of one decoder launch, cvae_set_draw_parts): rank 1's stack [rows 20..39 | rows 20..39]
        # sees, copy by copy, the masks of the one-rank stack [rows 0..39 | rows 0..39]
        with torch.no_grad():
            x2, y2 = torch.cat((t(P.x), t(P.x)), 0), torch.cat((t(P.y_in_enc), t(P.y_in_enc)), 0)
            gv.set_draw_parts(2)
            gv.set_draw_origin(0, 40, 10)
            torch.manual_seed(6)
            whole2 = enc(x2, y2, do=True, clamp_vae=True, lat_dim=4)[0]
            gv.set_draw_origin(20, 40, 10)
            torch.manual_seed(6)
            hi2 = enc(torch.cat((x2[20:40], x2[60:80]), 0), torch.cat((y2[20:40], y2[60:80]), 0), do=True, clamp_vae=True, lat_dim=4)[0]
        torch.cuda.synchronize()
        d2 = max(float((whole2[20:40] - hi2[:20]).abs().max()), float((whole2[60:80] - hi2[20:]).abs().max()))
        assert d2 <= 1e-5, d2
        assert float((whole2[:40] - whole2[40:]).abs().max()) > 1e-3    # the two copies draw different masks
    finally:
        gv.set_draw_origin(0, 0, 0)
        gv.set_draw_parts(1)


@pytest.mark.parametrize("hid,B,T", [(1024, 6, 12), (64, 20, 9)])
def test_stage4step_forms_agree(gv, dev, hid, B, T):
    """stage4.Stage4Step: the reference's ten passes on one stream, rec || cv stacked, stacked + weight-gradient GEMMs on the
    side stream (gradients accumulated straight into the flat buffer), and the fused form (cvae_sample_cat, cvae_stage4_loss,
    cvae_adam_step over the flat parameter buffer instead of torch ops and torch.optim.Adam) are the same step: same loss, same
    gradients, same weights after Adam.  Injected masks, so all forms see identical dropout."""
    import stage4
    big = hid >= 1024
    kw = dict(B=B, T=T, hidden=hid, n_cyc=2, bias_scale=0.05, tag="forms%d" % hid)
    P = synth.CycleVAEProblem(**kw) if big else synth.CycleVAEProblem(in_dim=10, out_dim=6, lat_dim=4, **kw)
    masks_np = make_masks(P, 4, 6)
    masks = {k: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in v] for k, v in masks_np.items()}
    ed, eo, dd, do_ = (54, 64, 34, 50) if big else (10, 8, 6, 6)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), t(P.eps)]
    res = []
    forms = ((False, False, False), (True, False, False), (True, True, False), (False, True, False), (True, True, True), (False, False, True))
    for stack, overlap, fused in forms:
        enc, dec = module(gv, P.enc, ed, eo, hid, True, dev), module(gv, P.dec, dd, do_, hid, False, dev)
        step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=2, lr=1e-4, stack_rec_cv=stack, overlap_wgrad=overlap, fused=fused)
        losses, g1 = [], None
        for k in range(2):                                   # two steps: the second sees the updated weights
            losses.append(float(step(*args, masks=masks).item()))
            torch.cuda.synchronize()
            if k == 0:
                g1 = step.grads.flat.detach().cpu().numpy().copy()
        res.append((losses, g1, enc.gru.weight_hh_l0.detach().cpu().numpy().copy()))
    base = res[0]
    names = ("stacked", "stacked + side stream", "side stream", "fused glue + flat Adam, stacked + side stream", "fused glue + flat Adam")
    for (losses, flat, whh), name in zip(res[1:], names):
        assert np.allclose(losses, base[0], rtol=2e-6), (name, losses, base[0])
        assert rel_err(flat, base[1].astype(np.float64), "step forms hu%d %s: flat gradient of step 1" % (hid, name)) <= 2e-6
        # Adam's first steps move an entry by lr * g / (|g| + eps): entries whose gradient is rounding noise may go either way, all
        # others must agree
        d = np.abs(whh - base[2])
        note("step forms hu%d %s: W_hh after two steps: max|d| %.3e, entries off by more than 1e-6: %.2e of all" %
             (hid, name, float(d.max()), float((d > 1e-6).mean())))
        assert float(d.max()) <= 4.2e-4 and float((d > 1e-6).mean()) <= 2e-3
    assert base[0][1] < base[0][0]


@pytest.mark.parametrize("fixture", ["stage4_step", "stage4_step_cyc4"])
def test_fused_step_reproduces_the_reference_recorded_windows(gv, dev, golden, fixture):
    """tests/golden/stage4_step.npz through stage4.Stage4Step in its fused form: ragged flen_acc, select_utt_idx, the carry of the
    second window (train...:1299-1311), cvae_stage4_loss and the flat cvae_adam_step -- same losses, gradients and post-step weights
    as the reference's own statements produced; with n_cyc = 2 (the recipe) and n_cyc = 4 (BASELINE configs[4])."""
    import stage4
    import train_util
    g = golden(fixture)
    P, x, cvx = train_util.golden_step_problem(g)
    enc, dec = module(gv, P.enc, 10, 8, 32, True, dev), module(gv, P.dec, 6, 6, 32, False, dev)
    step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=P.n_cyc, lr=1e-4, fused=True)
    assert step.fused and step.opt is None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    carry = None
    for w in range(2):
        s0, e0 = (int(v) for v in g["w%d_se" % w])
        masks = {k: [(t((g["w%d_%s%d_cmask" % (w, k, i)] * 2.0).astype(np.float32)), t((g["w%d_%s%d_gmask" % (w, k, i)] * 2.0).astype(np.float32)))
                     for i in range(n)] for k, n in (("enc", 2 * P.n_cyc), ("dec", 3 * P.n_cyc))}
        loss, carry = step(t(x[:, s0:e0 + 1]), t(cvx[:, s0:e0 + 1]), t(P.code_src[:, s0:e0 + 1]), t(P.code_trg[:, s0:e0 + 1]),
                           t(P.y_in_enc), t(P.y_in_dec), t(P.eps[:, :, :, s0:e0 + 1]), masks=masks,
                           flen_acc=[int(v) for v in g["w%d_flen_acc" % w]], select_utt_idx=[int(v) for v in g["w%d_select" % w]],
                           carry=carry, return_state=True)
        ref_loss = float(g["w%d_loss" % w])
        note("fused step, reference-recorded window %d: loss gpu %.6f reference %.6f" % (w, loss.item(), ref_loss))
        assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
        for kind, m in (("enc", enc), ("dec", dec)):
            for n in TRAINABLE:
                gr = dict(m.named_parameters())[n].grad
                ref_norm = float(g["w%d_%s_gnorm_%s" % (w, kind, n)])
                assert abs(float(gr.double().norm()) - ref_norm) <= 1e-3 * ref_norm, (w, kind, n)
                if "w%d_%s_g_%s" % (w, kind, n) in g.files:
                    assert rel_err(gr, g["w%d_%s_g_%s" % (w, kind, n)], "fused step %s, window %d: %s d%s" % (fixture, w, kind, n)) <= TIGHT_REL
    for kind, m in (("enc", enc), ("dec", dec)):
        for n in TRAINABLE:
            v = dict(m.named_parameters())[n].detach().double().cpu().numpy()
            got = np.array([v.sum(), (v * v).sum(), v.ravel()[0], v.ravel()[-1]])
            assert np.allclose(got, g["w1_%s_after_%s" % (kind, n)], rtol=2e-5, atol=2e-6), (kind, n)


def test_update_is_skipped_on_the_device_when_the_status_word_is_raised(gv, dev):
    """A step whose kernels report a failure must not touch parameters or moments: with the status sink raised before the update
    kernel runs, Stage4Step raises and the flat parameter buffer, exp_avg and exp_avg_sq are bit-identical to before."""
    import stage4
    import _cabi
    P = synth.CycleVAEProblem(B=4, T=6, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="gate")
    enc, dec = module(gv, P.enc, 10, 8, 64, True, dev), module(gv, P.dec, 6, 6, 64, False, dev)
    step = stage4.Stage4Step(enc, dec, lat_dim=4, n_cyc=2, lr=1e-3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), t(P.eps)]
    step(*args)
    torch.cuda.synchronize()
    before = [v.clone() for v in (step.flat_p, step.exp_avg, step.exp_avg_sq)]
    orig = step._forward_backward

    def failing(*a):
        out = orig(*a)
        torch.cuda.synchronize()
        gv._SINK[0] = 3           # what a timed-out hand-off of the forward recurrence leaves behind
        return out

    step._forward_backward = failing
    lib = gv._lib()
    try:
        with pytest.raises(_cabi.CvaeError):
            step(*args)
        torch.cuda.synchronize()
        for a, b in zip(before, (step.flat_p, step.exp_avg, step.exp_avg_sq)):
            assert torch.equal(a, b)
        assert step.step_no == 1 and int(gv._SINK[0]) == 0          # (the counter lives on the device: skipped steps do not count)
        # the first time-out switched the all-resident kernels to cooperative launches and repeated the step once before giving up
        assert step.coop_fallback and lib.get_option("coop_launch") == 1
        step._forward_backward = orig
        l2 = step(*args)              # and the next step works (now through hipLaunchCooperativeKernel)
        assert np.isfinite(float(l2.item())) and step.step_no == 2
    finally:
        lib.set_option("coop_launch", 0)


def test_step_outside_the_exchange_range_is_repeated_on_the_fp32_reverse_recurrence(gv, dev):
    """Status 5 (a gate gradient outside the range of the limb exchange of the persistent reverse recurrence) must not kill the
    step: the device skips the update, Stage4Step repeats the step on the fp32 reverse recurrence (same masks and eps) and applies
    THAT result.  (1) mechanism on a well-conditioned problem: the threshold is lowered (option bwd_overflow_at) so that an ordinary
    step trips it; gradients of the applied step against the stock-torch checker.  (2) a real overflow: with the decoder's out_1
    scaled by 30 the gate gradients pass 234 and the step is repeated as well."""
    import stage4
    lib = gv._lib()
    P = synth.CycleVAEProblem(B=4, T=6, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="huge")
    masks_np = make_masks(P, 4, 6)
    ref_loss, ref_grads = cpu_step(P, masks_np, 2)
    masks = {k: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in v] for k, v in masks_np.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = lambda Q: [t(Q.x), t(Q.cvx), t(Q.code_src), t(Q.code_trg), t(Q.y_in_enc), t(Q.y_in_dec), t(Q.eps)]
    try:
        lib.set_option("bwd_overflow_at", 2)           # |v| >= 2/256: every step "overflows" on the persistent path
        enc, dec = module(gv, P.enc, 10, 8, 64, True, dev), module(gv, P.dec, 6, 6, 64, False, dev)
        step = stage4.Stage4Step(enc, dec, lat_dim=4, n_cyc=2, lr=1e-4)
        before = step.flat_p.clone()
        loss = step(*args(P), masks=masks)
        torch.cuda.synchronize()
        note("repeated step: fallbacks %d, loss gpu %.6f cpu %.6f" % (step.fallbacks, float(loss), ref_loss))
        assert step.fallbacks == 1 and step.step_no == 1
        assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
        for kind, m in (("enc", enc), ("dec", dec)):
            for k in TRAINABLE:
                assert rel_err(dict(m.named_parameters())[k].grad, ref_grads[kind][k], "repeated step %s d%s" % (kind, k)) <= TIGHT_REL
        assert not torch.equal(before, step.flat_p)          # the repeated step WAS applied
        assert lib.get_option("train_bwd_per_step") == 0
    finally:
        lib.set_option("bwd_overflow_at", 60000)
    Q = synth.CycleVAEProblem(B=4, T=6, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="huge")
    Q.dec = dict(Q.dec)
    Q.dec["out_1.weight"] = (Q.dec["out_1.weight"] * 30.0).astype(np.float32)
    enc, dec = module(gv, Q.enc, 10, 8, 64, True, dev), module(gv, Q.dec, 6, 6, 64, False, dev)
    step = stage4.Stage4Step(enc, dec, lat_dim=4, n_cyc=2, lr=1e-6)
    loss = step(*args(Q), masks=masks)
    torch.cuda.synchronize()
    assert step.fallbacks == 1 and step.step_no == 1 and np.isfinite(float(loss)) and bool(torch.isfinite(step.grads.flat).all())


# (B, train_kernel) -> [Bp, fwd, fwd_rts, fwd_tiles, bwd, bwd_rts, bwd_per_launch, bwd_tiles] of test_train_pass_many_row_tiles
MANY_TILE_PLANS = {(200, 0): [224, _cabi.TRAIN_FWD_W3, 4, 4, _cabi.TRAIN_BWD_W3, 4, 8, 2],
                   (200, 1): [224, _cabi.TRAIN_FWD_PAIR, 2, 7, _cabi.TRAIN_BWD_PAIR, 2, 0, 7],
                   (100, 0): [128, _cabi.TRAIN_FWD_X3H, 2, 4, _cabi.TRAIN_BWD_W3, 4, 0, 2],
                   (100, 1): [128, _cabi.TRAIN_FWD_PAIR, 2, 4, _cabi.TRAIN_BWD_PAIR, 2, 0, 4]}


@pytest.mark.parametrize("B,tile", [(200, 0), (100, 16)])
def test_train_pass_many_row_tiles(gv, dev, B, tile):
    """One train-mode encoder pass at hu1024 with many row tiles, in the forms the plan gives (asserted with cvae_plan_train_pass):
    B=200 at default options = fourteen 16-row tiles on the 16-unit forms -- forward k_train_fwd_steps_w3 on four block rows with 4/4/3/3
    tiles (the own h re-read from the fp32 copy), reverse k_train_bwd_steps_w3 in launches of 8 + 6 tiles, at most two per block -- and
    B=100 forced to x3_tile 16 = eight 16-row tiles: forward k_train_fwd_steps_x3h with four per block on two block rows, reverse
    k_train_bwd_steps_w3 in one launch, two per block.  (The 32-row-tile forward k_train_fwd_steps_x3<16> and the 8-unit reverse over
    several launches run in tests/test_train_forms_gpu.py.)  Sampled rows against the stock-torch checker run on those rows alone (rows
    are independent), outputs and dx; parameter gradients against the same pass on the fp16-pair kernels (seven / four tiles per block
    both ways)."""
    from oracle import torch_stock as ts
    T = 4
    P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="manytrain%d" % B)
    masks = make_masks(P, 1, 0, tag="manytrain%d" % B)["enc"][0]
    cot = synth.normal("manytrain/cot%d" % B, (B, T, 64))
    rows = [0, 33, B // 2, B - 1]
    out_r, _, h_r, Pr, xr = ts.train_forward(P.enc, P.x[rows], P.y_in_enc[rows], None, masks[0][rows], masks[1][:, rows], 32)
    (out_r * torch.from_numpy(cot[rows])).sum().backward()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lib = gv._lib()
    res = {}
    try:
        for kern in (0, 1):
            lib.set_option("train_kernel", kern)
            lib.set_option("x3_tile", tile)
            enc = module(gv, P.enc, 54, 64, 1024, True, dev)
            plan = lib.plan_train_pass(lib.desc(54, 64, 1024, 3, 2, True, False), B, T)
            got = [plan[k] for k in ("Bp", "fwd", "fwd_rts", "fwd_tiles", "bwd", "bwd_rts", "bwd_per_launch", "bwd_tiles")]
            assert got == MANY_TILE_PLANS[(B, kern)], (B, kern, plan)
            xt = t(P.x).requires_grad_(True)
            enc._debug_masks = (t(masks[0]), t(masks[1]))
            out, yl, hl = enc(xt, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=32)
            (out * t(cot)).sum().backward()
            torch.cuda.synchronize()
            gv.check_status()
            res[kern] = (out.detach(), hl.detach(), xt.grad.detach(), {k: dict(enc.named_parameters())[k].grad.detach().clone() for k in TRAINABLE})
    finally:
        lib.set_option("train_kernel", 0)
        lib.set_option("x3_tile", 0)
    out, hl, dx, grads = res[0]
    assert rel_err(out[rows], out_r.detach().numpy(), "train B=%d rows out" % B) <= TIGHT_REL
    assert rel_err(hl[0][rows], h_r.detach().numpy(), "train B=%d rows h_last" % B) <= TIGHT_REL
    assert rel_err(dx[rows], xr.grad.numpy(), "train B=%d rows dx" % B) <= TIGHT_REL
    for k in TRAINABLE:
        assert rel_err(grads[k], res[1][3][k].double().cpu().numpy(), "train B=%d d%s exact vs pair kernels" % (B, k)) <= 2e-5


@pytest.mark.parametrize("B", [1, 2, 3])
def test_train_pass_up_to_three_rows_hu1024(gv, dev, B):
    """The recipe's own batch_size_utt = 1 (run.sh:172) and the rec || cv pair stacked from it: one train-mode encoder pass at hu1024
    over a full 80-frame window on the word-exchange kernels (cvae_train_ll.h) against the stock-torch checker -- outputs, carried
    state, dx, every parameter gradient -- and against the tile kernels (option no_ll)."""
    from oracle import torch_stock as ts
    T = 80
    P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="lltrain%d" % B)
    masks = make_masks(P, 1, 0, tag="lltrain%d" % B)["enc"][0]
    cot = synth.normal("lltrain/cot%d" % B, (B, T, 64))
    out_r, _, h_r, Pr, xr = ts.train_forward(P.enc, P.x, P.y_in_enc, None, masks[0], masks[1], 32)
    (out_r * torch.from_numpy(cot)).sum().backward()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lib = gv._lib()
    res = {}
    try:
        for no_ll in (0, 1):
            lib.set_option("no_ll", no_ll)
            enc = module(gv, P.enc, 54, 64, 1024, True, dev)
            xt = t(P.x).requires_grad_(True)
            enc._debug_masks = (t(masks[0]), t(masks[1]))
            out, yl, hl = enc(xt, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=32)
            (out * t(cot)).sum().backward()
            torch.cuda.synchronize()
            gv.check_status()
            res[no_ll] = (out.detach(), hl.detach(), xt.grad.detach(), {k: dict(enc.named_parameters())[k].grad.detach().clone() for k in TRAINABLE})
    finally:
        lib.set_option("no_ll", 0)
    for no_ll, (out, hl, dx, grads) in res.items():
        assert rel_err(out, out_r.detach().numpy(), "train B=%d no_ll=%d out" % (B, no_ll)) <= TIGHT_REL
        assert rel_err(hl[0], h_r.detach().numpy(), "train B=%d no_ll=%d h_last" % (B, no_ll)) <= TIGHT_REL
        assert rel_err(dx, xr.grad.numpy(), "train B=%d no_ll=%d dx" % (B, no_ll)) <= TIGHT_REL
        for k in TRAINABLE:
            assert rel_err(grads[k], Pr[k].grad.numpy(), "train B=%d no_ll=%d d%s" % (B, no_ll, k)) <= TIGHT_REL
    assert not torch.equal(res[0][0], res[1][0])


def test_train_pass_full_size_hu2048(gv, dev):
    """BASELINE configs[4]'s per-GPU shape: ONE train-mode encoder pass at hu2048 / ld64 over 64 utterances x a full 80-frame window
    (80 forward and 80 reverse per-step launches, the any-H training path) against the stock-torch checker on the whole batch:
    outputs, carried state, dx and every parameter gradient (sums over all 5,120 frames)."""
    from oracle import torch_stock as ts
    B, T = 64, 80
    P = synth.CycleVAEProblem(B=B, T=T, lat_dim=64, hidden=2048, n_cyc=1, bias_scale=0.05, tag="train2048")
    masks = make_masks(P, 1, 0, tag="train2048m")["enc"][0]
    cot = synth.normal("train2048/cot", (B, T, 128))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    out_r, _, h_r, Pr, xr = ts.train_forward(P.enc, P.x, P.y_in_enc, None, masks[0], masks[1], 64)
    (out_r * torch.from_numpy(cot)).sum().backward()
    enc = module(gv, P.enc, 54, 128, 2048, True, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt = t(P.x).requires_grad_(True)
    enc._debug_masks = (t(masks[0]), t(masks[1]))
    out, yl, hl = enc(xt, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=64)
    (out * t(cot)).sum().backward()
    torch.cuda.synchronize()
    gv.check_status()
    assert rel_err(out, out_r.detach().numpy(), "train B=64 T=80 hu2048 out") <= TIGHT_REL
    assert rel_err(hl[0], h_r.detach().numpy(), "train B=64 T=80 hu2048 h_last") <= TIGHT_REL
    assert rel_err(xt.grad, xr.grad.numpy(), "train B=64 T=80 hu2048 dx") <= TIGHT_REL
    for k in TRAINABLE:
        assert rel_err(dict(enc.named_parameters())[k].grad, Pr[k].grad.numpy(), "train B=64 T=80 hu2048 d" + k) <= TIGHT_REL


@pytest.mark.parametrize("kind,B", [("enc", 64), ("dec2", 128)], ids=["enc_64_rows", "rec_cv_stacked_128_rows"])
def test_train_pass_full_size_hu1024(gv, dev, kind, B):
    """The geometry bench.py's train leg TIMES (BASELINE configs[2], reference gru_vae.py:376-382, train...:1326-1338): one train-mode
    pass at hu1024 over 64 utterances x a full 80-frame window (forward k_train_fwd_steps_w3: four 16-row tiles, one per block row;
    reverse k_train_bwd_steps_w3: two block rows with two tiles each) and the stacked rec || cv decoder pass of 128 rows (eight tiles:
    two per block on four block rows, forward and reverse, one launch), default options; the plan is asserted with
    cvae_plan_train_pass.  Against the stock-torch checker on the WHOLE batch: outputs, carried state, dx and every parameter gradient
    (sums over all 5,120 / 10,240 frames) -- first as a plain autograd backward, then as stage4.Stage4Step runs it: gradients
    accumulated into existing p.grad, weight-gradient GEMMs on the side stream, two backward passes in flight on alternating
    scratch buffers (the second pass re-uses the first one's scratch only after its side-stream work)."""
    from oracle import torch_stock as ts
    T = 80
    enc_like = kind == "enc"
    P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="full1024" + kind)
    sd = P.enc if enc_like else P.dec
    cin, cout = (54, 64) if enc_like else (34, 50)
    x = P.x if enc_like else np.concatenate([P.code_src, synth.normal("full1024/z", (B, T, 32))], 2).astype(np.float32)
    y_in = P.y_in_enc if enc_like else P.y_in_dec
    mk = make_masks(P, 1, 1, tag="full1024m" + kind)["enc" if enc_like else "dec"][0]
    cot = synth.normal("full1024/cot" + kind, (B, T, cout))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    out_r, _, h_r, Pr, xr = ts.train_forward(sd, x, y_in, None, mk[0], mk[1], 32 if enc_like else -1)
    (out_r * torch.from_numpy(cot)).sum().backward()
    m = module(gv, sd, cin, cout, 1024, enc_like, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lib = gv._lib()
    plan = lib.plan_train_pass(lib.desc(cin, cout, 1024, 3, 2, enc_like, not enc_like), B, T)
    assert [plan[k] for k in ("Bp", "fwd", "fwd_rts", "fwd_tiles", "bwd", "bwd_rts", "bwd_per_launch", "bwd_tiles")] == \
        [B, _cabi.TRAIN_FWD_W3, 4, B // 64, _cabi.TRAIN_BWD_W3, B // 32, 0, 2], plan
    assert plan["fwd_full_writes"] == 1 and plan["bwd_writes_gates"] == 1

    def one_pass():
        xt = t(x).requires_grad_(True)
        m._debug_masks = (t(mk[0]), t(mk[1]))
        out, yl, hl = m(xt, t(y_in), do=True, clamp_vae=enc_like, lat_dim=32)
        return xt, out, hl

    name = "train %s B=%d T=80 hu1024" % (kind, B)
    xt, out, hl = one_pass()
    (out * t(cot)).sum().backward()
    torch.cuda.synchronize()
    gv.check_status()
    assert rel_err(out, out_r.detach().numpy(), name + " out") <= TIGHT_REL
    assert rel_err(hl[0], h_r.detach().numpy(), name + " h_last") <= TIGHT_REL
    assert rel_err(xt.grad, xr.grad.numpy(), name + " dx") <= TIGHT_REL
    for k in TRAINABLE:
        assert rel_err(dict(m.named_parameters())[k].grad, Pr[k].grad.numpy(), name + " d" + k) <= TIGHT_REL
    # the form the timed step runs: accumulate into p.grad, weight-gradient GEMMs on the side stream; TWO passes back to back, so
    # the accumulated gradients are twice the checker's and the second backward alternates to the other scratch buffer
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()
    side = torch.cuda.Stream()
    gv.set_side_stream(side)
    m._grad_sink = True
    try:
        pairs = [one_pass() for _ in range(2)]
        for xt2, out2, _ in pairs:
            (out2 * t(cot)).sum().backward()
        gv.join_side_stream()
    finally:
        gv.set_side_stream(None)
        m._grad_sink = False
    torch.cuda.synchronize()
    gv.check_status()
    for xt2, out2, hl2 in pairs:
        assert torch.equal(out2, out) and torch.equal(hl2, hl)
        assert rel_err(xt2.grad, xr.grad.numpy(), name + " dx (side stream)") <= TIGHT_REL
    for k in TRAINABLE:
        assert rel_err(dict(m.named_parameters())[k].grad, 2.0 * Pr[k].grad.numpy(), name + " d%s (side stream, two passes)" % k) <= TIGHT_REL


def test_unsynchronised_steps_skip_on_the_device_and_recover(gv, dev):
    """Stage4Step(sync=False): the host never waits for a step and never clears the status sink while steps are in flight.  With the
    exchange-range threshold lowered every persistent reverse recurrence raises status 5: the device must skip those updates -- of
    the failing step AND of every step enqueued before the host noticed (the latch stays raised) -- without advancing Adam's step
    counter, the host must switch to the fp32 reverse recurrence, and from then on steps must be applied with the right bias
    correction: the parameters end up where a synchronous run of as many APPLIED steps on the same batch and masks ends up."""
    import stage4
    lib = gv._lib()
    P = synth.CycleVAEProblem(B=4, T=6, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="lagged")
    masks_np = make_masks(P, 4, 6)
    masks = {k: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in v] for k, v in masks_np.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), t(P.eps)]

    def build(sync):
        enc, dec = module(gv, P.enc, 10, 8, 64, True, dev), module(gv, P.dec, 6, 6, 64, False, dev)
        return stage4.Stage4Step(enc, dec, lat_dim=4, n_cyc=2, lr=1e-3, sync=sync)

    n_total = 12
    try:
        lib.set_option("bwd_overflow_at", 2)           # |v| >= 2/256: every persistent reverse recurrence "overflows"
        lag = build(False)
        for _ in range(n_total):
            lag(*args, masks=masks)
        torch.cuda.synchronize()
        lag._drain()
        applied = lag.step_no
        note("unsynchronised steps: %d enqueued, %d skipped on the device, %d applied, fallbacks %d" % (n_total, lag.skipped, applied, lag.fallbacks))
        assert lag.fallbacks >= 1 and lag.skipped >= 1
        assert applied + lag.skipped == n_total and 1 <= applied < n_total
        assert int(gv._SINK[0]) == 0 and int(lag.status_dev[0].item()) == 0
        assert lib.get_option("train_bwd_per_step") == 1            # still inside the fp32 window
        w_lag = lag.mods["enc"].gru.weight_hh_l0.detach().clone()
        lag._fp32_left = 1
        lag(*args, masks=masks)                                     # the window ends: the caller's setting comes back
        torch.cuda.synchronize()
        assert lib.get_option("train_bwd_per_step") == 0
    finally:
        lib.set_option("bwd_overflow_at", 60000)
        lib.set_option("train_bwd_per_step", 0)
    ref = build(True)
    for _ in range(applied):
        ref(*args, masks=masks)
    torch.cuda.synchronize()
    assert ref.step_no == applied
    # `applied` updates through the fp32 reverse recurrence vs `applied` through the persistent one: the same gradients to ~1e-6 and
    # the same step counter, hence the same bias corrections
    dmax = float((w_lag - ref.mods["enc"].gru.weight_hh_l0.detach()).abs().max())
    note("unsynchronised vs synchronous run after %d applied steps: max |dW_hh| = %.3e" % (applied, dmax))
    assert dmax <= 2e-4          # lr 1e-3 x `applied` steps; entries whose gradient is rounding noise may differ by a step or two


def test_stage4step_in_a_process_group_of_one_rank(gv, dev):
    """The data-parallel code path on ONE GPU: init_process_group('nccl') (RCCL), the flat gradient all-reduce and the MAX-reduce
    of the status latch issued for real (force_collectives) -- losses, gradients and post-Adam parameters bit-identical to the run
    without a process group (a SUM / MAX over one rank is the identity)."""
    import socket
    import stage4
    import torch.distributed as dist
    P = synth.CycleVAEProblem(B=6, T=12, hidden=1024, n_cyc=2, bias_scale=0.05, tag="world1")
    masks_np = make_masks(P, 4, 6)
    masks = {k: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in v] for k, v in masks_np.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), t(P.eps)]

    def run(d):
        enc, dec = module(gv, P.enc, 54, 64, 1024, True, dev), module(gv, P.dec, 34, 50, 1024, False, dev)
        step = stage4.Stage4Step(enc, dec, lat_dim=32, n_cyc=2, lr=1e-4, dist=d, force_collectives=d is not None)
        step.time_allreduce = d is not None
        losses = [float(step(*args, masks=masks).item()) for _ in range(2)]
        torch.cuda.synchronize()
        return losses, step.grads.flat.clone(), step.flat_p.clone(), step

    base = run(None)
    own_group = not dist.is_initialized()
    if own_group:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        assert dist.get_backend() == "nccl"
        got = run(dist)
        assert len(got[3].allreduce_ms) == 2                      # the all-reduce WAS issued, twice
        ms = [a.elapsed_time(b) for a, b in got[3].allreduce_ms]
        note("one-rank RCCL group: flat all-reduce of %d floats %.3f / %.3f ms" % (got[1].numel(), ms[0], ms[1]))
        import shard
        assert shard.max_over_ranks(1.25, dist, dev, force=True) == 1.25
        dist.barrier()
    finally:
        if own_group:
            dist.destroy_process_group()
    assert got[0] == base[0]
    assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])


@pytest.mark.parametrize("B,hid", [(1, 64), (3, 64), (5, 64), (20, 64), (1, 1024), (8, 1024)])
def test_windows_of_changing_length_with_carry(gv, dev, B, hid):
    """What a real epoch looks like (train...:1299-1311, windows.plan_windows): consecutive frame windows of ONE utterance batch with
    different lengths -- full windows, then a short tail, down to a single frame -- every pass continuing from the state of the
    window before.  The fused step runs them back to back on the same modules (scratch buffers grown and reused across shapes, the
    word-exchange layout for <= 3 rows next to the tile layout, T = 1 on the per-step path) and must give, window by window, the loss
    of the stock-torch checker that carries the same state and applies the same Adam updates.
    hid = 1024: the PRODUCT dims hu1024 / ld32 -- the recipe's one-utterance batch (word-exchange kernels) and its
    batch_size_utt = 8 (one 16-row tile of the exact tile kernels), tails of 1 and 2 frames on the per-step fallback, the grow-only
    scratch across shapes (train...:71-72,102-106 produces such tails at the end of every utterance batch)."""
    import stage4
    from oracle import torch_stock as ts
    lens = [12, 12, 5, 1, 2, 9]
    Ttot = sum(lens)
    dims = dict(in_dim=10, out_dim=6, lat_dim=4) if hid == 64 else dict(in_dim=54, out_dim=50, lat_dim=32)
    Cin, Co, L = dims["in_dim"], dims["out_dim"], dims["lat_dim"]
    P = synth.CycleVAEProblem(B=B, T=Ttot, hidden=hid, n_cyc=2, bias_scale=0.05, tag="ragged%d_%d" % (B, hid) if hid != 64 else "ragged%d" % B, **dims)
    enc, dec = module(gv, P.enc, Cin, 2 * L, hid, True, dev), module(gv, P.dec, L + 2, Co, hid, False, dev)
    step = stage4.Stage4Step(enc, dec, lat_dim=L, n_cyc=2, lr=1e-3)
    leaf = {k: {n: torch.from_numpy(v.copy()).requires_grad_(n in TRAINABLE) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}
    opt = torch.optim.Adam([leaf[k][n] for k in ("enc", "dec") for n in stage4.TRAINABLE if n in leaf[k]], lr=1e-3)
    # (parameter order of Stage4Step: encoder then decoder, module order; Adam is element-wise, the order does not matter)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    carry_g = carry_c = None
    s0 = 0
    for w, n in enumerate(lens):
        sl = slice(s0, s0 + n)
        masks_np = make_masks(synth.CycleVAEProblem(B=B, T=n, hidden=hid, n_cyc=2, tag="raggedm%d_%d" % (B, w), **dims), 4, 6)
        gm = {k: [(t(a), t(b)) for a, b in v] for k, v in masks_np.items()}
        loss_g, carry_g = step(t(P.x[:, sl]), t(P.cvx[:, sl]), t(P.code_src[:, sl]), t(P.code_trg[:, sl]), t(P.y_in_enc), t(P.y_in_dec),
                               t(P.eps[:, :, :, sl]), masks=gm, carry=carry_g, return_state=True)

        def run_pass(kind, xin, y_in, clamp, mk, h_in=None):
            return ts.train_forward_t(leaf[kind], xin, y_in, torch.from_numpy(mk[0]), torch.from_numpy(mk[1]), clamp, h_in=h_in, with_state=True)

        opt.zero_grad()
        loss_c, carry_c, _ = stage4.chain_loss(run_pass, c(P.x[:, sl]), c(P.cvx[:, sl]), c(P.code_src[:, sl]), c(P.code_trg[:, sl]),
                                               c(P.y_in_enc), c(P.y_in_dec), c(P.eps[:, :, :, sl]), L, 2, masks_np, carry=carry_c,
                                               return_state=True)
        loss_c.backward()
        opt.step()
        note("ragged windows B=%d hu%d window %d (T=%d): loss gpu %.6f cpu %.6f" % (B, hid, w, n, float(loss_g), float(loss_c)))
        assert abs(float(loss_g) - float(loss_c)) <= 2e-6 * abs(float(loss_c)), (w, n)      # (measured: <= 3e-7 relative)
        s0 += n
    torch.cuda.synchronize()
    w_g = enc.gru.weight_hh_l0.detach().cpu().numpy()
    d = float(np.max(np.abs(w_g - leaf["enc"]["gru.weight_hh_l0"].detach().numpy())))
    note("ragged windows B=%d hu%d: W_hh after %d updates max|d| %.3e" % (B, hid, len(lens), d))
    assert d <= 3e-3       # lr 1e-3 x 6 Adam steps; entries whose gradient is rounding noise may go either way
    # one scratch buffer per slot, whatever the shapes were
    assert all(len(m._prep_train.scratch) <= 2 for m in (enc, dec))


def test_sampling_vae_batch_autograd_is_one_launch_each_way(gv, dev):
    """sampling_vae_batch under autograd (what the training script calls between the encoder and the decoder, gru_vae.py:85-98): the
    draw is reproducible from torch's seed, z = mu + exp(s/2) eps for the eps the kernel drew, and the gradient equals the one torch
    derives for that map."""
    torch.manual_seed(21)
    p = (0.3 * torch.randn(5, 7, 8, device=dev)).requires_grad_(True)
    torch.manual_seed(4)
    z = gv.sampling_vae_batch(p, lat_dim=4)
    cot = torch.randn_like(z)
    (z * cot).sum().backward()
    torch.manual_seed(4)
    with torch.no_grad():
        z_again = gv.sampling_vae_batch(p.detach(), lat_dim=4)      # the no-grad path draws the same eps from the same seed
    assert torch.equal(z.detach(), z_again)
    eps = (z.detach() - p.detach()[..., :4]) / torch.exp(p.detach()[..., 4:] / 2)
    q = p.detach().clone().requires_grad_(True)
    zt = q[..., :4] + torch.exp(q[..., 4:] / 2) * eps
    (zt * cot).sum().backward()
    d = float((p.grad - q.grad).abs().max())
    note("sampling_vae_batch autograd: max |d grad| vs torch = %.3e" % d)
    assert d <= 2e-6 * max(1.0, float(q.grad.abs().max()))
    with pytest.raises(ValueError):
        gv.sampling_vae_batch(p, lat_dim=3)


@pytest.mark.parametrize("n", [1, 7, 300])
def test_script_loss_calls_fused_on_the_device(gv, dev, n):
    """TWFSEloss(x, y, L2=False, GV=False) and loss_vae on device tensors (the training script's per-utterance calls, train...:1366-1372)
    run as one launch each way: same values and same gradients as the torch-op form on the CPU, for sliced (strided) operands."""
    torch.manual_seed(n)
    D, L, st = 6, 4, 2
    xb = torch.randn(3, n + 2, D)
    src = torch.randn(3, n + 5, st + D)
    lat = 0.5 * torch.randn(3, n + 1, 2 * L)
    crit = gv.TWFSEloss()

    def run(device):
        x = xb.detach().clone().to(device).requires_grad_(True)
        p = lat.detach().clone().to(device).requires_grad_(True)
        y = src.to(device)[1, 3:3 + n, st:]
        s_, m_, sd_ = crit(x[1, :n], y, L2=False, GV=False)
        kl = gv.loss_vae(p[2, :n], lat_dim=L)
        tot = 0.3 * s_ + 2.0 * m_ + kl * 1.5
        if n > 1:
            tot = tot + 0.7 * sd_
        tot.backward()
        return [float(s_), float(m_), float(sd_), float(kl)], x.grad.cpu(), p.grad.cpu()

    ref, gx_r, gp_r = run(torch.device("cpu"))
    got, gx, gp = run(dev)
    for a, b in zip(got, ref):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 2e-6 * max(1.0, abs(b)), (got, ref)
    assert float((gx - gx_r).abs().max()) <= 2e-6 * max(1.0, float(gx_r.abs().max()))
    assert float((gp - gp_r).abs().max()) <= 2e-6 * max(1.0, float(gp_r.abs().max()))


def test_plain_backward_accumulates_into_p_grad_on_a_side_stream(gv, dev):
    """The unchanged training script's `batch_loss.backward()` (train...:1419): every GRU_RNN pass adds its parameter gradients straight
    into p.grad and runs its weight-gradient GEMMs on a side stream, joined by a callback of the autograd engine before backward()
    returns (gru_vae.set_backward_overlap, default on).  Same gradients as the flow that hands them to autograd, whether p.grad was
    None (optimizer.zero_grad(set_to_none=True)) or held values; torch.autograd.grad / backward(inputs=...) still get theirs."""
    P = synth.CycleVAEProblem(B=5, T=20, tag="autosink")
    enc = module(gv, P.enc, 54, 64, 1024, True, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    masks = (t((synth.uniform01("autosink/c", (5, 20, 486)) >= 0.5).astype(np.float32) * 2), t((synth.uniform01("autosink/g", (20, 5, 1024)) >= 0.5).astype(np.float32) * 2))
    cot = t(synth.normal("autosink/cot", (5, 20, 64)).astype(np.float32))

    def run(x):
        # two passes through the same module (as the chain applies each net several times): the second consumes the first's output
        enc._debug_masks = masks
        a = enc(x, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=32)[0]
        enc._debug_masks = masks
        b = enc(torch.cat((x[:, :, :4], a[:, :, :50]), 2), t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=32)[0]
        return ((a + b) * cot).sum()

    res = {}
    for overlap in (False, True):
        prev = gv.set_backward_overlap(overlap)
        try:
            for p in enc.parameters():
                p.grad = None
            x = t(P.x).requires_grad_(True)
            run(x).backward()
            torch.cuda.synchronize()
            g1 = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
            x2 = t(P.x).requires_grad_(True)
            run(x2).backward()                      # accumulates on top
            torch.cuda.synchronize()
            res[overlap] = (x.grad.clone(), g1, {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None})
        finally:
            gv.set_backward_overlap(prev)
    gv.check_status()
    assert set(res[True][1]) == set(res[False][1]) == set(TRAINABLE)
    assert rel_err(res[True][0], res[False][0].cpu().numpy().astype(np.float64), "auto sink dx") <= 1e-6
    for n in TRAINABLE:
        assert rel_err(res[True][1][n], res[False][1][n].cpu().numpy().astype(np.float64), "auto sink d%s" % n) <= 2e-6
        assert rel_err(res[True][2][n], res[False][2][n].cpu().numpy().astype(np.float64), "auto sink d%s, second backward on top" % n) <= 2e-6
        assert rel_err(res[True][2][n], 2.0 * res[False][1][n].cpu().numpy().astype(np.float64), "auto sink 2x d%s" % n) <= 4e-6
    # callers that ask for the gradients get them, and p.grad stays untouched
    for p in enc.parameters():
        p.grad = None
    x3 = t(P.x).requires_grad_(True)
    w = enc.gru.weight_hh_l0
    gx, gw = torch.autograd.grad(run(x3), [x3, w])
    assert w.grad is None and rel_err(gw, res[False][1]["gru.weight_hh_l0"].cpu().numpy().astype(np.float64), "autograd.grad dW_hh") <= 2e-6
    assert rel_err(gx, res[False][0].cpu().numpy().astype(np.float64), "autograd.grad dx") <= 1e-6
    x4 = t(P.x).requires_grad_(True)
    run(x4).backward(inputs=[x4])
    assert all(p.grad is None for p in enc.parameters()) and rel_err(x4.grad, res[False][0].cpu().numpy().astype(np.float64), "backward(inputs=[x])") <= 1e-6


def test_philox_masks_do_not_depend_on_the_side_stream(gv, dev):
    """A train-mode pass that draws its own dropout masks (Philox, seeded from torch's CPU generator) draws the feedback operand's
    mask on the side stream when one is set and T*B*H >= 2^20, and both masks in one launch on its own stream otherwise
    (draw_train_masks, csrc/cvae_train.inc).  64 rows x 256 frames at H = 64 is the smallest such shape: the same seed gives the same
    bits of out, h_last, dx and every parameter gradient either way.  No gradient sink and no direct accumulation: both runs return
    their gradients to autograd, so the mask branch of the forward is the only difference between them."""
    B, T = 64, 256
    P = synth.CycleVAEProblem(B=B, T=T, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=1, bias_scale=0.1, tag="philox_side")
    enc = module(gv, P.enc, 10, 8, 64, True, dev)
    assert B * T * 64 == 1 << 20 and gv._lib().get_option("masks_on_side") == 1      # (else the second run would not take the side branch)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cot = t(synth.normal("philox_side/cot", (B, T, 8)).astype(np.float32))
    rng, prev = torch.random.get_rng_state(), gv.set_backward_overlap(False)
    res = {}
    try:
        for side in (None, torch.cuda.Stream()):
            gv.set_side_stream(side)
            for p in enc.parameters():
                p.grad = None
            torch.manual_seed(20261021)
            x = t(P.x).requires_grad_(True)
            out, _, hl = enc(x, t(P.y_in_enc), do=True, clamp_vae=True, lat_dim=4)
            (out * cot).sum().backward()
            gv.join_side_stream()
            torch.cuda.synchronize()
            res[side is not None] = [out.detach(), hl.detach(), x.grad] + [dict(enc.named_parameters())[k].grad for k in TRAINABLE]
    finally:
        gv.set_side_stream(None)
        gv.set_backward_overlap(prev)
        torch.random.set_rng_state(rng)
    gv.check_status()
    assert float(res[False][0].abs().max()) > 0 and all(bool(torch.isfinite(a).all()) for a in res[False])
    for name, a, b in zip(["out", "h_last", "dx"] + ["d" + k for k in TRAINABLE], res[False], res[True]):
        assert torch.equal(a, b), "%s differs with a side stream set (max|d| %.3e)" % (name, float((a - b).abs().max()))


def test_fused_step_at_the_timed_geometry(gv, dev):
    """BASELINE configs[2] AT ITS TIMED GEOMETRY inside the suite: stage4.Stage4Step in its default form (fused glue, rec || cv
    stacked, weight-gradient GEMMs on the side stream, flat Adam) on 64 utterances x 80 frames, hu1024 / ld32 / cyc2 -- every
    launch of the step runs at the size bench.py times.  The stock-torch checker would need minutes for the whole batch, so the
    generator's own selection mechanism (select_utt_idx, train...:1363: the other rows are computed and ignored) restricts the loss:
    16 utterances for the loss value, 4 utterances for EVERY parameter gradient and the weights after the update (eval-mode chain,
    MCD).  Rows are independent recurrences, so a selected row's contribution is what the checker computes on that row alone."""
    import stage4
    import gru_vae
    from oracle import cyclevae_oracle as orc
    from oracle import torch_stock as ts
    B, T, L, NC, H = 64, 80, 32, 2, 1024
    P = synth.CycleVAEProblem(B=B, T=T, hidden=H, n_cyc=NC, bias_scale=0.05, tag="timed64")
    gen = torch.Generator().manual_seed(7)
    mk = lambda shape: (torch.rand(shape, generator=gen) >= 0.5).float() * 2.0
    masks = {"enc": [(mk((B, T, 9 * 54)), mk((T, B, H))) for _ in range(2 * NC)],
             "dec": [(mk((B, T, 9 * (2 + L))), mk((T, B, H))) for _ in range(3 * NC)]}
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    sub = lambda r: {k: [(a[r].contiguous(), b[:, r].contiguous()) for a, b in v] for k, v in masks.items()}
    inp = lambda r: [c(P.x[r]), c(P.cvx[r]), c(P.code_src[r]), c(P.code_trg[r]), c(P.y_in_enc[r]), c(P.y_in_dec[r]), c(P.eps[:, :, r])]
    gmasks = {k: [(a.to(dev), b.to(dev)) for a, b in v] for k, v in masks.items()}
    gin = [v.to(dev) for v in inp(list(range(B)))]

    def gpu_step(rows):
        enc, dec = module(gv, P.enc, 54, 2 * L, H, True, dev), module(gv, P.dec, 2 + L, 50, H, False, dev)
        step = stage4.Stage4Step(enc, dec, lat_dim=L, n_cyc=NC, lr=1e-4)
        assert step.fused and step.stack_rec_cv and step.overlap_wgrad
        loss = float(step(*gin, masks=gmasks, select_utt_idx=rows).item())
        torch.cuda.synchronize()
        gv.check_status()
        return loss, enc, dec

    def cpu_leaves():
        return {k: {n: torch.from_numpy(v.copy()).requires_grad_(n in TRAINABLE) for n, v in sd.items()} for k, sd in (("enc", P.enc), ("dec", P.dec))}

    def cpu_loss(leaf, rows):
        return stage4.chain_loss(lambda kind, xin, y_in, clamp, m_: ts.train_forward_t(leaf[kind], xin, y_in, m_[0], m_[1], clamp),
                                 *inp(rows), L, NC, sub(rows))

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    # (a) the loss over 16 utterances spread over all four 16-row tiles
    rows16 = [0, 3, 7, 12, 16, 21, 27, 31, 32, 38, 41, 47, 48, 52, 59, 63]
    loss_g, _, _ = gpu_step(rows16)
    with torch.no_grad():
        loss_c = float(cpu_loss(cpu_leaves(), rows16).item())
    note("timed geometry (64 x 80, hu1024, cyc2), 16 utterances in the loss: gpu %.6f cpu %.6f rel %.2e" % (loss_g, loss_c, abs(loss_g - loss_c) / abs(loss_c)))
    assert abs(loss_g - loss_c) <= 2e-6 * abs(loss_c)
    # (b) every gradient, and the weights after the update, with 4 utterances in the loss
    rows4 = [5, 30, 33, 62]
    loss_g4, enc, dec = gpu_step(rows4)
    leaf = cpu_leaves()
    opt = torch.optim.Adam([leaf[k][n] for k in leaf for n in TRAINABLE], lr=1e-4)
    l4 = cpu_loss(leaf, rows4)
    l4.backward()
    assert abs(loss_g4 - float(l4.item())) <= 2e-6 * abs(float(l4.item()))
    for kind, m in (("enc", enc), ("dec", dec)):
        for k in TRAINABLE:
            gr = dict(m.named_parameters())[k].grad
            assert rel_err(gr, leaf[kind][k].grad.numpy(), "timed geometry, 4 utterances in the loss: %s d%s" % (kind, k)) <= TIGHT_REL
    opt.step()
    after = {k: {n: v.detach().numpy() for n, v in leaf[k].items()} for k in leaf}
    ce, cd = ts.StockGRURNN(after["enc"], 54, 2 * L, H), ts.StockGRURNN(after["dec"], 2 + L, 50, H)
    cpu_eval = ts.cycle_chain(ce, cd, *inp(rows4), NC, L)
    enc.eval(); dec.eval()
    ein = [v.to(dev) for v in inp(rows4)]
    with torch.no_grad():
        g = gru_vae.CycleChain(enc, dec, lat_dim=L, n_cyc=NC)(*ein[:6], eps=ein[6])
    for k in ("rec", "cv", "reccyc"):
        a = g[k].cpu().numpy().reshape(-1, 50)
        b = np.stack([v.numpy() for v in cpu_eval[k]]).reshape(-1, 50)
        mcd = float(np.mean(orc.mcd_frames(a, b)))
        note("timed geometry, eval chain with the weights after the step: MCD(%s) vs the checker %.2e dB" % (k, mcd))
        assert mcd <= 5e-5, (k, mcd)


def test_side_streams_are_probed_for_real_concurrency(gv, dev):
    """HIP multiplexes streams onto a few hardware queues; a stream that lands on the launch stream's queue serialises with it (measured:
    one of the first ten streams torch hands out does, and a stage-4 step with its weight-gradient GEMMs on that stream takes 27.0
    instead of 22.7 ms).  gru_vae.concurrent_stream probes its candidates with a spin kernel and must return one that overlaps --
    wherever in torch's stream pool the process happens to be."""
    import time
    lib = gv._lib()
    cur = torch.cuda.current_stream()

    def wall(a, b):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lib.selftest_occupy(1, 1024, 1000000, a.cuda_stream)
        lib.selftest_occupy(1, 1024, 1000000, b.cuda_stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    wall(cur, cur)
    alone = min(wall(cur, cur) for _ in range(3)) / 2.0
    pool = [torch.cuda.Stream() for _ in range(16)]                 # walk the pool: some of these share the launch stream's queue
    ratios = [min(wall(cur, s) for _ in range(2)) / alone for s in pool]
    note("streams from torch's pool, (spin on launch stream + spin on stream k) / one spin: " + " ".join("%.2f" % r for r in ratios))
    gv._concurrent.clear()
    for slot in range(3):
        s = gv.concurrent_stream(slot=slot)
        r = min(wall(cur, s) for _ in range(3)) / alone
        note("concurrent_stream(slot=%d): %.2f" % (slot, r))
        assert r < 1.5, (slot, r)
    a = gv.concurrent_stream(slot=1)
    b = gv.concurrent_stream(slot=2, beside=[a])
    assert min(wall(a, b) for _ in range(3)) / alone < 1.5
    assert gv.concurrent_stream(slot=0) is gv.concurrent_stream(slot=0)          # cached
