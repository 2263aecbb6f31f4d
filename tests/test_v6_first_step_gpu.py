"""Frame 0 of a fresh k_gru_steps_v6 pass without its recurrent product (library option v6_skip_t0, csrc/cvae_exact3.h;
profiles/v6_launch_ramp_notes.md), on the device.

T = 3 frames of a hu1024 network: the encoder (KFW 8) at 64 rows, the decoder (KFW 6) at 64 and 128 rows (one and two 32-row tiles per
block), the encoder at 160 rows (a block with three tiles), and one H = 2048 pass (33 rows: the form whose third weight limb is
streamed).  Each fresh and with a carried-in state: v6_skip_t0 = 1 (default) and = 0 must
give the same bits -- every product left out is an exact +0 -- the plan must name the same form under both, and rows 0, 31, 32 and the
last one are compared with the oracle at the bound of tests/test_v6_hot_loop_gpu.py (5e-6 for one pass of this size)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclevae-vc_amd")]
import synth
from oracle import cyclevae_oracle as orc

pytestmark = pytest.mark.gpu
TIGHT_PASS = 5e-6
T = 3
BMAX = 160
V6 = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


@pytest.fixture
def skip_t0(gv):
    """skip_t0(v): the option for this test; back to its default afterwards"""
    yield lambda v: gv._lib().set_option("v6_skip_t0", v)
    gv._lib().set_option("v6_skip_t0", 1)


@pytest.fixture(scope="module")
def problem():
    """ONE 160-row problem; the smaller passes take its first rows.  The decoder's input: codes + a stand-in latent (unit normal)."""
    P = synth.CycleVAEProblem(B=BMAX, T=T, bias_scale=0.05, tag="v6t0")
    P.dec_x = np.ascontiguousarray(np.concatenate((P.code_src, P.eps[0, 0]), axis=2).astype(np.float32))
    P.h0 = np.tanh(synth.normal("v6t0/h0", (1, BMAX, 1024), synth.SEED)).astype(np.float32)
    return P


def _mod(gv, dev, sd, i, o, h, enc):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, kernel_size=3, dilation_size=2, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def nets(gv, dev, problem):
    return {"enc": _mod(gv, dev, problem.enc, 54, 64, 1024, True), "dec": _mod(gv, dev, problem.dec, 34, 50, 1024, False)}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(gv, dev, skip_t0, net, sd, x, y, h0, kw, what):
    B = x.shape[0]

    def run():
        with torch.no_grad():
            out = net(_t(x, dev), _t(y, dev), h_in=None if h0 is None else _t(h0, dev), **kw)
        torch.cuda.synchronize()
        gv.check_status()
        return [o.clone() for o in out]

    plan = lambda: gv._lib().plan_pass(net.prepared(dev)[0], B, T, gv._flags())
    skip_t0(1)
    form_on, on = plan(), run()
    skip_t0(0)
    form_off, off = plan(), run()
    assert form_on == form_off == V6, (what, form_on, form_off)
    names = ("trj_out", "y_last", "h")
    for name, a, b in zip(names, on, off):
        assert torch.equal(a, b), "%s %s: v6_skip_t0 changes the bits" % (what, name)
    rows = [0, 31, 32, B - 1]
    ref = orc.gru_rnn_forward(sd, x[rows], y[rows], h_in=None if h0 is None else h0[:, rows], **kw)
    for name, got, want in zip(names, on, ref):
        g = got.cpu().numpy()
        g = g[:, rows] if name == "h" else g[rows]
        assert np.all(np.isfinite(g)), (what, name)
        d = float(np.max(np.abs(g.astype(np.float64) - want.astype(np.float64))))
        print("%s %s: max|d| = %.3e" % (what, name, d))
        assert d <= TIGHT_PASS, (what, name, d)


@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "h_in"])
@pytest.mark.parametrize("which,B", [("enc", 64), ("dec", 64), ("dec", 128), ("enc", 160)])
def test_h1024_option_on_off_and_oracle(gv, dev, problem, nets, skip_t0, which, B, carry):
    P = problem
    x = (P.x if which == "enc" else P.dec_x)[:B]
    y = (P.y_in_enc if which == "enc" else P.y_in_dec)[:B]
    kw = dict(clamp_vae=True, lat_dim=32) if which == "enc" else {}
    _check(gv, dev, skip_t0, nets[which], getattr(P, which), x, y, P.h0[:, :B] if carry else None, kw,
           "%s B=%d %s" % (which, B, "h_in" if carry else "fresh"))


@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "h_in"])
def test_h2048_streamed_third_limb_form(gv, dev, skip_t0, carry):
    B = 33
    Q = synth.CycleVAEProblem(B=B, T=T, hidden=2048, bias_scale=0.05, tag="v6t0_2048")
    enc = _mod(gv, dev, Q.enc, 54, 64, 2048, True)
    h0 = np.tanh(synth.normal("v6t0_2048/h0", (1, B, 2048), synth.SEED)).astype(np.float32) if carry else None
    _check(gv, dev, skip_t0, enc, Q.enc, Q.x, Q.y_in_enc, h0, dict(clamp_vae=True, lat_dim=32),
           "enc2048 B=33 %s" % ("h_in" if carry else "fresh"))
