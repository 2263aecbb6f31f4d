"""Many-to-many chains on the host-fiber emulator (the real library's kernels compiled for the host, CPU tensors): per-cycle target
codes and converted excitation through CycleChain (fresh and carry form, both posteriors), stage 4 and the C entry point;
loader_m2m.chain_inputs; stage6.convert_targets; the plan at the many-to-many decoder widths.  tests/m2m_util.py holds the float64
reference and the checks; tests/test_m2m_gpu.py runs them on the device.

Every test asks for the feature before it launches (m2m_util.require_feature) and FAILS without it: a tree without per-cycle inputs
would read a 4-D tensor as its first slice.  Off the device Stage4Step always runs its unfused form; the fused step is on the device
side."""
import numpy as np
import pytest

import m2m_util as M
from emu_util import bind_emulator, emu_lib
from stacked_util import EMU_CHAIN, EMU_PASS

torch = pytest.importorskip("torch")


@pytest.fixture
def gv(monkeypatch):
    return bind_emulator(monkeypatch)


@pytest.fixture
def dev():
    return torch.device("cpu")


def test_the_feature_is_announced_and_the_abi_stays_10(gv):
    import _cabi
    M.require_feature(gv)
    assert _cabi.ABI_VERSION == 10 and gv._lib().lib.cvae_abi_version() == 10
    assert "cvae_cycle_forward_m2m" in _cabi.ADDITIVE


@pytest.mark.parametrize("posterior", ["gauss", "laplace"])
def test_equal_slices_are_the_3d_call_bit_for_bit(gv, dev, posterior):
    M.check_chain_identity(gv, dev, M.problem_h64(2, posterior == "laplace"), posterior)


def test_entry_point_with_strides_0_is_cvae_cycle_forward(gv, dev):
    M.check_entry_identity(gv, dev, M.problem_h64(2))


def test_step_with_equal_slices_is_the_3d_step_bit_for_bit(gv, dev):
    M.check_step_identity(gv, dev, M.problem_h64(2), fused=False)


@pytest.mark.parametrize("n_cyc,posterior", [(2, "gauss"), (3, "gauss"), (2, "laplace")])
def test_chain_against_the_float64_reference(gv, dev, n_cyc, posterior):
    P = M.problem_h64(n_cyc, posterior == "laplace")
    M.check_chain_parity(gv, dev, P, posterior, EMU_CHAIN, "emulator H64 cyc%d" % n_cyc)


def test_carry_chain_against_the_float64_reference(gv, dev):
    M.check_chain_carry_parity(gv, dev, M.problem_h64(2), "gauss", EMU_CHAIN, "emulator H64")


def test_step_against_the_float64_reference(gv, dev):
    """H 64, B 5, T 12, n_cyc 2 (unfused: the form Stage4Step has off the device), rec || cv as one stacked pass; apart: on the
    device."""
    M.check_step_parity(gv, dev, M.problem_h64(2), forms=(False,), what="emulator H64", stack=True)


def test_chain_loss_takes_the_shapes_on_plain_torch(gv, dev):
    M.check_chain_forward_unfused_matches(gv, dev, M.problem_h64(2))


def test_cycle_selection(gv, dev):
    M.check_cycle_selection(gv, dev, M.problem_h64(2))


def test_shape_errors(gv, dev):
    M.check_shape_errors(gv, dev, M.problem_h64(2))


def test_bad_strides_are_refused_before_anything_runs(gv, dev):
    M.check_bad_strides(gv, dev, M.problem_h64(2))


def test_chain_inputs(gv, dev):
    M.check_chain_inputs(gv, dev, run_step=False)


def test_convert_targets(gv, dev):
    M.check_convert_targets(gv, dev, 64, EMU_PASS)


def test_plan_at_the_many_to_many_decoder_widths():
    M.check_plan(emu_lib())


def test_stacked_chain_takes_per_cycle_inputs(gv, dev):
    """hidden_layers 2 (CycleChain._call_deep): the pass-by-pass chain reads code_trg[i] / cvx[i]; equal slices give the 3-D call's
    bits, and cycle 1 follows its own code."""
    import synth
    from laplace_chain_util import N, T, module
    M.require_feature(gv)
    P = M.Problem(5, 6, 10, 6, 4, 64, 5, 2, "m2m64/deep")          # (six frames: three chains of stacked passes on the emulator)
    sd_e = synth.gru_rnn_state("m2m/deep/enc", P.in_dim, 2 * P.lat_dim, 64, scale_in=(P.mu, P.sigma), bias_scale=0.1, hidden_layers=2)
    sd_d = synth.gru_rnn_state("m2m/deep/dec", P.ncode + P.lat_dim, P.out_dim, 64, scale_out=(P.mu[P.stdim:], P.sigma[P.stdim:]),
                               bias_scale=0.1, hidden_layers=2)
    enc = module(gv, sd_e, P.in_dim, 2 * P.lat_dim, 64, True, dev, layers=2)
    dec = module(gv, sd_d, P.ncode + P.lat_dim, P.out_dim, 64, False, dev, layers=2)
    chain = gv.CycleChain(enc, dec, P.lat_dim, 2)
    eps = T(P.eps, dev)
    base = chain(*M.chain_args(P, dev, P.cvx[0], P.code_trg[0]), eps=eps)
    rep = chain(*M.chain_args(P, dev, M.repeat_cycles(P.cvx[0], 2), M.repeat_cycles(P.code_trg[0], 2)), eps=eps)
    out = chain(*M.chain_args(P, dev), eps=eps)
    for k in M.KEYS:
        M.same(rep[k], base[k], "stacked chain, equal slices, " + k)
        M.same(out[k][0], base[k][0], "stacked chain, cycle 0, " + k)
    assert not np.array_equal(N(out["cv"][1]), N(base["cv"][1])) and not np.array_equal(N(out["latcv"][1]), N(base["latcv"][1]))
    with pytest.raises(ValueError):
        chain(*M.chain_args(P, dev, code_trg=M.repeat_cycles(P.code_trg[0], 3)), eps=eps)
