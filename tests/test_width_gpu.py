"""Device stage of the hidden-width tests: EVERY row of the case table of tests/width_util.py on the MI355X, against the float64
references of tests/width_ref.py, and two whole paths at widths no other test builds a module at.  python -m pytest tests -m gpu

What the emulator stage (tests/test_width_cpu.py) cannot see is the device build itself -- wave masks and votes with idle waves,
the grid barrier behind 252 blocks (H = 1008: the largest resident grid of 256 CUs), residency, the compiler -- and every width
above 192: 272 (partial second block of k_gru_step_bwd), 320 / 960 (partly filled waves of k_gru_steps_ll), 1040 / 2064 (per-step
launches by residency; 32-33 and 64-65 chunks per wave of k_gru_step_train; a round plus a tail in k_bwd_step_gemm).

Every buffer is a view of exactly the size the library asks for inside one NaN-filled device allocation (width_util's header): a
pass that reads or writes past a buffer fails the comparison or the guard check, it cannot fault.

Bounds: the device bounds the project already uses, unchanged -- TIGHT_PASS = 5e-6 per eval pass and TIGHT_CHAIN = 5e-6 for the chain
(tests/stacked_util.py), TIGHT_REL = 8e-6 relative to each tensor's largest entry for every training tensor (tests/test_gpu_train.py);
the stage-4 step's loss within 1e-5 relative of the checker's and its two forms within 2e-6 of each other, as
test_stage4_step_vs_cpu_checker and test_stage4step_forms_agree ask there.
Every measured distance is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to width_gpu_report.txt;
profiles/width_notes.md keeps the per-width maxima."""
import numpy as np
import pytest

import synth
import width_util as wu
from train_util import TRAINABLE, cpu_step, make_masks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_train import TIGHT_REL      # noqa: E402  (the project's device bound for training tensors)

note = wu.make_note("width_gpu_report.txt")
ids = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


@pytest.fixture(scope="module")
def lib(gv, dev):
    """A context of its own on the loaded library: options and the status sink set here never reach the passes of other tests."""
    ctx = gv._lib().new_context()
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(scope="module")
def mem(lib, dev):
    return wu.TorchMem(lib, dev)


@pytest.fixture(scope="module")
def refs():
    """case -> float64 reference, computed once per case and module."""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = wu.train_reference(c) if isinstance(c, wu.TrainCase) else wu.eval_reference(c)
        return cache[c]
    return get


@pytest.mark.parametrize("c", wu.EVAL_CASES, ids=ids(wu.EVAL_CASES))
def test_eval_pass_at_width(mem, refs, c):
    """Whole pass (planned form asserted), two windows with the carried state, h_in with an off-manifold y_in, T = 1; at the six
    GENERIC widths also the per-step launches, bit for bit."""
    wu.run_eval_case(mem, c, refs(c), note, wu.TIGHT_PASS)


@pytest.mark.parametrize("c", wu.PROJ_CASES, ids=["%s-out%d" % (c.id, 2 * c.lat) for c in wu.PROJ_CASES])
def test_projection_classes_at_width(mem, refs, c):
    wu.run_proj_case(mem, c, refs(c), note, wu.TIGHT_PASS)


@pytest.mark.parametrize("c", wu.DEEP_CASES, ids=ids(wu.DEEP_CASES))
def test_stacked_gru_at_width(mem, refs, c):
    """hidden_layers = 2 through the _deep entry points, against frontend_ref.forward."""
    wu.run_eval_case(mem, c, refs(c), note, wu.TIGHT_PASS)


@pytest.mark.parametrize("c", wu.TRAIN_CASES, ids=ids(wu.TRAIN_CASES))
def test_train_pass_at_width(mem, refs, options, c):
    """Forward + backward of one train-mode pass with injected masks: outputs, carried state, dx and the ten gradients."""
    options(**dict(c.opts))
    wu.run_train_case(mem, c, refs(c), note, TIGHT_REL, TIGHT_REL)


# ---- whole paths ---------------------------------------------------------------------------------------------------------------

def module(gv, sd, i, o, h, enc, dev, train=False):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, kernel_size=3, dilation_size=2, do_prob=0.5, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev)
    return m.train() if train else m.eval()


def test_cycle_chain_h128(gv, dev):
    """CycleChain at H = 128, B = 2, T = 8, cyc2 against the stock-torch chain: the encoder passes (2 rows) plan the word-exchange
    kernel with waves 1-3 idle, the stacked rec || cv decoder pass (4 rows) the any-H kernel behind its grid barrier."""
    from oracle import torch_stock as ts
    H, B, T, L = 128, 2, 8, 4
    P = synth.CycleVAEProblem(B=B, T=T, in_dim=10, out_dim=6, lat_dim=L, hidden=H, n_cyc=2, bias_scale=0.1, tag="width/chain128")
    lib = gv._lib()
    assert lib.plan_pass(lib.desc(10, 8, H, 3, 2, True, False), B, T, gv._flags()) == wu.LL
    assert lib.plan_pass(lib.desc(6, 6, H, 3, 2, False, True), 2 * B, T, gv._flags()) == wu.GENERIC
    enc, dec = module(gv, P.enc, 10, 8, H, True, dev), module(gv, P.dec, 6, 6, H, False, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    chain = gv.CycleChain(enc, dec, lat_dim=L, n_cyc=2)
    with torch.no_grad():
        out = chain(t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), eps=t(P.eps))
    torch.cuda.synchronize()
    assert chain.status()[0] == 0
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ref = ts.cycle_chain(ts.StockGRURNN(P.enc, 10, 8, H), ts.StockGRURNN(P.dec, 6, 6, H), c(P.x), c(P.cvx), c(P.code_src), c(P.code_trg),
                         c(P.y_in_enc), c(P.y_in_dec), c(P.eps), 2, L)
    for k in ref:
        got = out[k].cpu().numpy()
        assert np.all(np.isfinite(got)), k
        d = float(np.max(np.abs(got.astype(np.float64) - torch.stack(ref[k]).numpy())))
        note("device    chain h128 cyc2 %-7s max|d| = %.3e" % (k, d))
        assert d <= wu.TIGHT_CHAIN, (k, d)


def test_stage4_step_h48(gv, dev):
    """stage4.Stage4Step at H = 48, B = 3, T = 5, cyc2 -- every pass on the per-step training kernels, rec || cv stacked -- in the
    torch-glue form and the fused form, against the stock-torch checker: loss, every gradient, and the two forms against each other."""
    import stage4
    H, B, T = 48, 3, 5
    P = synth.CycleVAEProblem(B=B, T=T, in_dim=10, out_dim=6, lat_dim=4, hidden=H, n_cyc=2, bias_scale=0.05, tag="width/step48")
    masks_np = make_masks(P, 4, 6, tag="width/step48/masks")
    ref_loss, ref_grads = cpu_step(P, masks_np, 2)
    masks = {k: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in v] for k, v in masks_np.items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = [t(P.x), t(P.cvx), t(P.code_src), t(P.code_trg), t(P.y_in_enc), t(P.y_in_dec), t(P.eps)]
    res = {}
    for fused in (False, True):
        mods = {"enc": module(gv, P.enc, 10, 8, H, True, dev, train=True), "dec": module(gv, P.dec, 6, 6, H, False, dev, train=True)}
        step = stage4.Stage4Step(mods["enc"], mods["dec"], lat_dim=4, n_cyc=2, lr=1e-4, fused=fused)
        loss = float(step(*args, masks=masks).item())
        torch.cuda.synchronize()
        note("device    stage-4 step h48 fused=%s: loss %.6f, checker %.6f" % (fused, loss, ref_loss))
        assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
        grads = {}
        for kind, m in mods.items():
            for k in TRAINABLE:
                g = dict(m.named_parameters())[k].grad.detach().cpu().numpy()
                assert np.all(np.isfinite(g)), (kind, k)
                e = wu.rel_err(g, ref_grads[kind][k].astype(np.float64))
                note("device    stage-4 step h48 fused=%-5s %s d%-20s rel err = %.3e" % (fused, kind, k, e))
                assert e <= TIGHT_REL, (fused, kind, k, e)
                grads[(kind, k)] = g
        res[fused] = (loss, grads)
    assert abs(res[True][0] - res[False][0]) <= 2e-6 * abs(res[False][0])
    for key, g in res[True][1].items():
        assert wu.rel_err(g, res[False][1][key].astype(np.float64)) <= 2e-6, key
