"""The Laplace posterior (posterior="laplace", CVAE_DRAW_LAPLACE) on the device, through gru_vae -> ctypes -> libcyclevae_hip.so:
the cases of tests/test_laplace_chain_cpu.py at the device bounds, and what needs the device -- the chain and stage 6 at H = 1024 (the
32-row-tile prologue of the exact-operand recurrence, the word-exchange kernels' single rows, the windowed wavefront) and the fused
stage-4 step.  python -m pytest tests -m gpu

Yardsticks: tests/golden/laplace_chain.npz (the reference's own functions) and tests/laplace_chain_ref.py (float64, on
oracle/torch_stock).  Bounds: TIGHT_PASS / TIGHT_CHAIN 5e-6 and TIGHT_KERNELS 3e-6 (tests/stacked_util.py) through
frontend_util.bound_for; training: loss 1e-5 relative, gradients 8e-6, forms 2e-6 relative on the flat gradient
(tests/test_gpu_train.py).  Every measured difference is printed (run with -s)."""
import pytest

import laplace_chain_util as U
import synth
from frontend_util import TIGHT_CHAIN, TIGHT_KERNELS, TIGHT_PASS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


@pytest.fixture(scope="module")
def G():
    return U.golden()


@pytest.fixture(autouse=True)
def status_checked(gv):
    yield
    torch.cuda.synchronize()
    gv.check_status()


def test_pass_supplied_eps_against_the_golden(gv, dev, G):
    U.check_pass_supplied_eps(gv, dev, G, TIGHT_PASS)


@pytest.mark.parametrize("L", [4, 6])
def test_pass_philox_draw_is_cvae_sample_laplace_bit_for_bit(gv, dev, L):
    U.check_pass_philox(gv, dev, L)


def test_chain_fresh_and_carry_against_the_golden(gv, dev, G):
    U.check_chain_golden(gv, dev, G, TIGHT_CHAIN)


def test_chain_philox_is_the_pass_by_pass_composition(gv, dev):
    U.check_chain_philox(gv, dev, TIGHT_KERNELS)


def test_posterior_gauss_is_the_default_call_bit_for_bit(gv, dev):
    U.check_chain_default(gv, dev)


def test_chain_hu1024_against_the_float64_reference(gv, dev):
    """B 4, T 12: the rec || cv pass is two cells in one half-empty 32-row tile of k_gru_steps_v6, whose prologue draws per tile."""
    U.check_chain_f64(gv, dev, TIGHT_CHAIN)


def test_stacked_chain_philox_is_the_pass_by_pass_composition(gv, dev):
    """hidden_layers = 2, H 64: CycleChain._call_deep."""
    P = synth.CycleVAEProblem(tag="lapdeep", hidden_layers=2, **dict(U.H64, bias_scale=0.1))
    U.check_chain_philox(gv, dev, TIGHT_KERNELS, layers=2, P=P)


def test_stage6_convert_pair_against_the_golden(gv, dev, G):
    U.check_stage6_golden(gv, dev, G, TIGHT_PASS)


def test_stage6_convert_pair_hu1024(gv, dev):
    """H 1024, T 12, three draws (single-row cells: the 256-thread mean of the draws), against the float64 reference."""
    U.check_stage6_f64(gv, dev, TIGHT_PASS)


def test_stage6_convert_pair_hu1024_windowed(gv, dev):
    """The windowed wavefront: the unwindowed values bit for bit, and the float64 reference.  window=8 on the 12-frame pair is refused
    by the window rule itself (each window must exceed twice the front-end's reach, 8 frames), so this call cuts 20 frames at 10."""
    with pytest.raises(ValueError, match="reach"):
        U.check_stage6_f64(gv, dev, TIGHT_PASS, window=8)
    U.check_stage6_f64(gv, dev, TIGHT_PASS, T_=20, window=10)


def test_stage6_convert_pairs_hu1024_row_tile(gv, dev):
    """Two pairs in one call: the mean of the draws in the 32-row-tile prologue."""
    U.check_stage6_pairs_f64(gv, dev, TIGHT_PASS)


@pytest.mark.parametrize("L", [4, 6])
def test_latent_mean_with_the_flag(gv, dev, L):
    U.check_latent_mean(gv, dev, L)


@pytest.mark.parametrize("parts", [1, 2])
def test_sample_cat_forward_and_backward(gv, dev, parts):
    U.check_sample_cat(gv, dev, parts)


@pytest.mark.parametrize("half,select,flen_acc", U.LOSS_ROWS)
def test_stage4_loss_with_the_flag(gv, dev, half, select, flen_acc):
    U.check_stage4_loss(gv, dev, half, select, flen_acc)


@pytest.mark.parametrize("hidden", [64, 1024])
def test_stage4step_fused_and_unfused_against_the_float64_reference(gv, dev, hidden):
    """H 64, B 3, T 10 and H 1024, B 4, T 12: both step forms against the float64 reference and against each other."""
    P, eps = U.train_problem(hidden)
    masks, ref = U.reference_step(P, eps)
    U.check_step(gv, dev, P, eps, masks, ref, forms=(True, False))


def test_refusals(gv):
    U.check_refusals(gv)
