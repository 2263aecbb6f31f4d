"""k_gru_steps_v6 at H = 1024 with its weights consumed from accumulator registers, its front-end weights read one 16-k step ahead
and its phase counters compiled out (csrc/cvae_exact3.h; profiles/v6_hot_loop_notes.md).

Every pass is T = 4 frames of a hu1024 network: the encoder (in_dim 54: KFW 8) and the decoder (in_dim 34: KFW 6) at 64 rows (one
32-row tile per block) and at 128 rows (two tiles per block: h_{t-1} kept in registers per tile), the encoder at 160 rows (a block with
three tiles: the path that re-reads its own state from the exchange buffer); each with and without a carried-in state.  Rows 0, 31, 32,
63 and the last one (both ends of the first two tiles, and the last tile) are compared with the oracle at the project's bound for one
pass of this size (tests/test_gpu_parity.py: TIGHT_PASS = 5e-6), and the same pass launched through the PROFILING instantiation
(CVAE_FLAG_STEP_TIMING) must give the same bits: the two instantiations are the same arithmetic on differently allocated registers,
so an operand bound to the wrong register shows here."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclevae-vc_amd")]
import _cabi
import synth
from oracle import cyclevae_oracle as orc

pytestmark = pytest.mark.gpu
TIGHT_PASS = 5e-6
T = 4
BMAX = 160


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


@pytest.fixture(scope="module")
def problem():
    """ONE 160-row problem; the smaller passes take its first rows.  The decoder's input: codes + a stand-in latent (unit normal)."""
    P = synth.CycleVAEProblem(B=BMAX, T=T, bias_scale=0.05, tag="v6hot")
    P.dec_x = np.ascontiguousarray(np.concatenate((P.code_src, P.eps[0, 0]), axis=2).astype(np.float32))
    P.h0 = np.tanh(synth.normal("v6hot/h0", (1, BMAX, 1024), synth.SEED)).astype(np.float32)      # a state a pass could have left
    return P


@pytest.fixture(scope="module")
def nets(gv, dev, problem):
    def mod(sd, i, o, enc):
        m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=1024, kernel_size=3, dilation_size=2, scale_in_flag=enc, scale_out_flag=not enc)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(dev).eval()
    return {"enc": mod(problem.enc, 54, 64, True), "dec": mod(problem.dec, 34, 50, False)}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "h_in"])
@pytest.mark.parametrize("which,B", [("enc", 64), ("dec", 64), ("enc", 128), ("dec", 128), ("enc", 160)])
def test_pass_vs_oracle_and_profiling_instance(gv, dev, problem, nets, monkeypatch, which, B, carry):
    P, net = problem, nets[which]
    x = (P.x if which == "enc" else P.dec_x)[:B]
    y = (P.y_in_enc if which == "enc" else P.y_in_dec)[:B]
    h0 = P.h0[:, :B] if carry else None
    kw = dict(clamp_vae=True, lat_dim=32) if which == "enc" else {}

    def run():
        with torch.no_grad():
            out = net(_t(x, dev), _t(y, dev), h_in=None if h0 is None else _t(h0, dev), **kw)
        torch.cuda.synchronize()
        gv.check_status()
        return [o.clone() for o in out]

    plain = run()
    monkeypatch.setattr(gv, "_flags_extra", _cabi.FLAG_STEP_TIMING)
    prof = run()
    monkeypatch.setattr(gv, "_flags_extra", 0)

    rows = [0, 31, 32, 63, B - 1]
    ref = orc.gru_rnn_forward(getattr(P, which), x[rows], y[rows],
                              h_in=None if h0 is None else h0[:, rows], **kw)
    names = ("trj_out", "y_last", "h")
    for name, got, want in zip(names, plain, ref):
        g = got.cpu().numpy()
        g = g[:, rows] if name == "h" else g[rows]
        assert np.all(np.isfinite(g)), name
        d = float(np.max(np.abs(g.astype(np.float64) - want.astype(np.float64))))
        print("%s B=%d %s %s: max|d| = %.3e" % (which, B, "h_in" if carry else "fresh", name, d))
        assert d <= TIGHT_PASS, (which, B, carry, name, d)
    for name, a, b in zip(names, plain, prof):
        assert torch.equal(a, b), "%s: the profiling instantiation gives other bits" % name
