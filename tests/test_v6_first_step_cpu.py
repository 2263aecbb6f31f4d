"""Frame 0 of a fresh k_gru_steps_v6 pass without its recurrent product (library option v6_skip_t0, csrc/cvae_exact3.h), on the
host-fiber build of the same statements (H = 64 instances).

A pass no cell of which carries a state in starts from an all-zero slot 0; the tasks of frame 0 then request no state operand and
issue no recurrent MFMA (Step6Params::h0_zero).  Every product left out is an exact +0 added to a sum that started at +0, so the
outputs must be the SAME BITS with the option on (default) and off, at T = 2 and 3, with one, two and three row tiles per block
(4 / 32 rows, 64, 96 rows under max_rt = 1), in the three-limb, two-limb, streamed-third-limb and hoisted forms.  With a carried-in
state both settings run the same path, within the oracle bound of tests/test_emu_library.py::test_exact3_recurrence_h64 (5e-6).  One
fresh case overwrites slot 0 of both state buffers with NaN patterns behind the prologue (exp bit 7): the skipping kernel reads none
of it, the multiplying one returns NaN."""
import numpy as np
import pytest

import _cabi
import synth
from emu_util import NpNet, emu_lib
from frontend_util import NpFrontNet, problem_h64
from oracle import cyclevae_oracle as orc

FL = _cabi.FLAG_PERSISTENT | _cabi.FLAG_EXACT3
V6, V6H = 5, 7
BOUND = 5e-6
ROWS = (4, 32, 64, 96)
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def case(lib, B, T):
    """One problem per (B, T), built once: net, inputs (y_in off the manifold of out_1(h_in): the frame-0 correction is non-zero)."""
    if (B, T) not in _CACHE:
        P = synth.CycleVAEProblem(B=B, T=T, in_dim=6, out_dim=4, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1, tag="t0_%d_%d" % (B, T))
        y_in = (P.y_in_enc + 0.21).astype(np.float32)
        h_in = (0.3 * synth.normal("t0_h/%d" % B, (1, B, 64))).astype(np.float32)
        _CACHE[(B, T)] = (P, NpNet(lib, P.enc, 6, 8, 64), y_in, h_in)
    return _CACHE[(B, T)]


def both(lib, options, run):
    """run() with v6_skip_t0 = 1 and = 0"""
    options(v6_skip_t0=1)
    on = run()
    options(v6_skip_t0=0)
    off = run()
    options(v6_skip_t0=1)
    return on, off


def test_option_is_listed_and_on_by_default(lib):
    lib.reset_options()
    assert lib.get_option("v6_skip_t0") == 1


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("B", ROWS)
def test_fresh_pass_same_bits_and_oracle(lib, options, B, T):
    options(max_rt=1)
    P, net, y_in, _ = case(lib, B, T)
    assert lib.plan_pass(net.d, B, T, FL) == V6
    on, off = both(lib, options, lambda: net.forward(P.x, y_in, clamp_lat_dim=4, flags=FL))
    want = orc.gru_rnn_forward(P.enc, P.x, y_in, clamp_vae=True, lat_dim=4)
    for name, a, b, w in zip(("trj_out", "y_last", "h_last"), on, off, want):
        assert np.all(np.isfinite(a)), name
        assert np.array_equal(a, b), "%s: v6_skip_t0 changes the bits (max|d| = %.3e)" % (name, float(np.max(np.abs(a - b))))
        d = float(np.max(np.abs(a.astype(np.float64) - w.astype(np.float64))))
        assert d <= BOUND, (name, d)


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("B", ROWS)
def test_carried_state_runs_the_same_path(lib, options, B, T):
    options(max_rt=1)
    P, net, y_in, h_in = case(lib, B, T)
    on, off = both(lib, options, lambda: net.forward(P.x, y_in, h_in=h_in, clamp_lat_dim=4, flags=FL))
    want = orc.gru_rnn_forward(P.enc, P.x, y_in, h_in=h_in, clamp_vae=True, lat_dim=4)
    for name, a, b, w in zip(("trj_out", "y_last", "h_last"), on, off, want):
        assert np.array_equal(a, b), name
        d = float(np.max(np.abs(a.astype(np.float64) - w.astype(np.float64))))
        assert d <= BOUND, (name, d)


@pytest.mark.parametrize("opts", [{"v6_limbs_h64": 2}, {"v6_w2s_h64": 1}], ids=["two_limbs", "streamed_third_limb"])
@pytest.mark.parametrize("B", [4, 96])
def test_other_forms_same_bits(lib, options, opts, B):
    options(max_rt=1, **opts)
    P, net, y_in, _ = case(lib, B, 3)
    on, off = both(lib, options, lambda: net.forward(P.x, y_in, clamp_lat_dim=4, flags=FL))
    for a, b in zip(on, off):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_hoisted_form_same_bits(lib, options):
    """k_gru_steps_v6<1, 0>: a front-end too wide for the LDS image (27 taps), gate inputs from the GEMM in front of the launch"""
    P = problem_h64(3, 3)
    net = NpFrontNet(lib, P.enc, 30, 8, 64, 3, 3)
    B, T = P.x.shape[0], 3
    assert lib.plan_pass(net.d, B, T, FL) == V6H
    x, y_in = P.x[:, :T], (P.y_in_enc + 0.21).astype(np.float32)
    on, off = both(lib, options, lambda: net.forward(x, y_in, clamp_lat_dim=4, flags=FL))
    for a, b in zip(on, off):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


@pytest.mark.parametrize("B", [64, 96])
def test_skipping_kernel_reads_nothing_of_slot_0(lib, options, B):
    """slot 0 = NaN patterns behind the prologue (two and three tiles per block): same bits as the clean pass with the option on;
    with it off the kernel multiplies the poisoned slot and says so"""
    options(max_rt=1)
    P, net, y_in, _ = case(lib, B, 3)
    clean = net.forward(P.x, y_in, clamp_lat_dim=4, flags=FL)
    options(exp=128)
    poisoned = net.forward(P.x, y_in, clamp_lat_dim=4, flags=FL)
    for a, b in zip(clean, poisoned):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)
    options(v6_skip_t0=0)
    assert not np.all(np.isfinite(net.forward(P.x, y_in, clamp_lat_dim=4, flags=FL)[0]))
