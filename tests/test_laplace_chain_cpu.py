"""The Laplace posterior (posterior="laplace", CVAE_DRAW_LAPLACE) through the fused chain, stage 6 and the stage-4 step, without a
GPU: the real library on the host-fiber emulator (CPU tensors; H <= 64).

Yardsticks: tests/golden/laplace_chain.npz, recorded from the reference's own GRU_RNN / sampling_vae_laplace / loss_vae_laplace
(tests/golden/make_golden_laplace_chain.py), and tests/laplace_chain_ref.py, the float64 reference on oracle/torch_stock.  Bounds:
EMU_PASS / EMU_CHAIN / TIGHT_KERNELS of tests/stacked_util.py through frontend_util.bound_for; the training bounds of
tests/test_gpu_train.py (tests/laplace_chain_util.py).  Stage4Step runs its unfused form here -- off the device it always does; the
fused step's two kernels are checked on their own (cases 5 and 6), the fused step itself in tests/test_laplace_chain_gpu.py."""
import numpy as np
import pytest

import _cabi
import laplace_chain_util as U
import synth
from emu_util import bind_emulator
from frontend_util import EMU_CHAIN, EMU_PASS, TIGHT_KERNELS


@pytest.fixture
def gv(monkeypatch):
    return bind_emulator(monkeypatch)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cpu")


@pytest.fixture(scope="module")
def G():
    return U.golden()


@pytest.fixture(scope="module")
def train64():
    P, eps = U.train_problem(64)
    return (P, eps) + U.reference_step(P, eps)


def test_the_abi_stays_10_and_the_flag_is_bit_30():
    assert _cabi.ABI_VERSION == 10 and _cabi.DRAW_LAPLACE == 1 << 30 == _cabi.CLAMP_LAPLACE


def test_the_fixture_sits_on_the_floor_and_above_it_with_eps_of_both_signs(G):
    """The golden's conditions: encoder log-scales exactly on the Laplace floor and above it, supplied eps of both signs; the weights
    are the synth seeds' (SHA-256)."""
    P = U.problem_h64()
    assert str(G["sha_enc"]) == synth.sha256_state(P.enc) and str(G["sha_dec"]) == synth.sha256_state(P.dec)
    for pre in ("chain_", "carry_"):
        s = np.concatenate([G[pre + k][..., P.lat_dim:].ravel() for k in ("lat", "latcv")])
        assert np.any(s == np.float32(U.FLOOR)) and np.any(s > np.float32(U.FLOOR)) and np.all(s >= np.float32(U.FLOOR))
        assert np.any(G[pre + "eps"] < 0) and np.any(G[pre + "eps"] > 0)
        assert G[pre + "eps"].min() >= -0.4999 and G[pre + "eps"].max() < 0.5
    for k in ("s6_eps_src", "s6_eps_trg"):
        assert G[k].shape == (U.N_SMPL, 12, P.lat_dim) and np.any(G[k] < 0) and np.any(G[k] > 0)
    assert abs(float(np.exp(U.FLOOR)) - 1.0 / np.sqrt(2.0e6)) < 1e-12          # the floor: a scale of 1e-3 / sqrt(2)


def test_pass_supplied_eps_against_the_golden(gv, dev, G):
    U.check_pass_supplied_eps(gv, dev, G, EMU_PASS)


@pytest.mark.parametrize("L", [4, 6])
def test_pass_philox_draw_is_cvae_sample_laplace_bit_for_bit(gv, dev, L):
    U.check_pass_philox(gv, dev, L)


def test_chain_fresh_and_carry_against_the_golden(gv, dev, G):
    U.check_chain_golden(gv, dev, G, EMU_CHAIN)


def test_chain_philox_is_the_pass_by_pass_composition(gv, dev):
    U.check_chain_philox(gv, dev, TIGHT_KERNELS)


def test_posterior_gauss_is_the_default_call_bit_for_bit(gv, dev):
    U.check_chain_default(gv, dev)


def test_stage6_convert_pair_against_the_golden(gv, dev, G):
    U.check_stage6_golden(gv, dev, G, EMU_PASS)


@pytest.mark.parametrize("L", [4, 6])
def test_latent_mean_with_the_flag(gv, dev, L):
    U.check_latent_mean(gv, dev, L)


@pytest.mark.parametrize("parts", [1, 2])
def test_sample_cat_forward_and_backward(gv, dev, parts):
    U.check_sample_cat(gv, dev, parts)


@pytest.mark.parametrize("half,select,flen_acc", U.LOSS_ROWS)
def test_stage4_loss_with_the_flag(gv, dev, half, select, flen_acc):
    U.check_stage4_loss(gv, dev, half, select, flen_acc)


def test_stage4step_unfused_against_the_float64_reference(gv, dev, train64):
    """H 64, B 3, T 10.  Loss: 1e-5 relative; gradients: 8e-6; weights after Adam (see U.check_step)."""
    P, eps, masks, ref = train64
    U.check_step(gv, dev, P, eps, masks, ref, forms=(False,))


def test_library_refuses_the_flag_where_a_dimension_is_missing(gv, dev):
    """The flag alone is no dimension: lat_dim = 0 | flag fails like lat_dim = 0."""
    with pytest.raises(_cabi.CvaeError):
        gv._lib().latent_mean([_cabi.LatMeanJob(1, None, 0, 1, 0, 1)], _cabi.DRAW_LAPLACE, 2)


def test_refusals(gv):
    U.check_refusals(gv)
