"""Many-to-many chains on the device, through gru_vae -> ctypes -> libcyclevae_hip.so: the cases of tests/test_m2m_cpu.py at the
device bounds, the fused Stage4Step, the H = 1024 shapes, and each new instance of the exact-operand recurrence
(k_gru_steps_v6<16, KFW, 3>, KFW 5 / 7 / 9 / 11) on a decoder-shaped pass.  python -m pytest tests -m gpu

Yardstick: tests/m2m_util.py (float64, on oracle/torch_stock).  Bounds: TIGHT_CHAIN / TIGHT_PASS 5e-6 and TIGHT_KERNELS 3e-6
(tests/stacked_util.py); Stage4Step loss 2e-6 relative, gradients 8e-6 (tests/test_gpu_train.py).  Every measured difference is
printed (run with -s)."""
import pytest

import m2m_util as M
from stacked_util import TIGHT_CHAIN, TIGHT_PASS

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


@pytest.fixture(autouse=True)
def status_checked(gv):
    yield
    torch.cuda.synchronize()
    gv.check_status()


@pytest.mark.parametrize("hidden", [64, 1024])
@pytest.mark.parametrize("posterior", ["gauss", "laplace"])
def test_equal_slices_are_the_3d_call_bit_for_bit(gv, dev, hidden, posterior):
    P = M.problem_h64(2, posterior == "laplace") if hidden == 64 else M.problem_h1024(posterior == "laplace")
    M.check_chain_identity(gv, dev, P, posterior)


def test_entry_point_with_strides_0_is_cvae_cycle_forward(gv, dev):
    M.check_entry_identity(gv, dev, M.problem_h64(2))


@pytest.mark.parametrize("fused", [True, False])
def test_step_with_equal_slices_is_the_3d_step_bit_for_bit(gv, dev, fused):
    M.check_step_identity(gv, dev, M.problem_h64(2), fused=fused)


@pytest.mark.parametrize("n_cyc,posterior", [(2, "gauss"), (3, "gauss"), (2, "laplace")])
def test_chain_against_the_float64_reference(gv, dev, n_cyc, posterior):
    P = M.problem_h64(n_cyc, posterior == "laplace")
    M.check_chain_parity(gv, dev, P, posterior, TIGHT_CHAIN, "device H64 cyc%d" % n_cyc)


def test_carry_chain_against_the_float64_reference(gv, dev):
    M.check_chain_carry_parity(gv, dev, M.problem_h64(2), "gauss", TIGHT_CHAIN, "device H64")


@pytest.mark.parametrize("stack", [True, False])
def test_step_against_the_float64_reference(gv, dev, stack):
    """H 64, B 5, T 12, n_cyc 2: the fused and the unfused step, rec || cv stacked and apart."""
    M.check_step_parity(gv, dev, M.problem_h64(2), forms=(True, False), what="device H64", stack=stack)


def test_cycle_selection(gv, dev):
    M.check_cycle_selection(gv, dev, M.problem_h64(2))


def test_shape_errors(gv, dev):
    M.check_shape_errors(gv, dev, M.problem_h64(2))


def test_bad_strides_are_refused_before_anything_runs(gv, dev):
    M.check_bad_strides(gv, dev, M.problem_h64(2))


def test_chain_inputs(gv, dev):
    M.check_chain_inputs(gv, dev)


@pytest.mark.parametrize("hidden", [64, 1024])
def test_convert_targets(gv, dev, hidden):
    M.check_convert_targets(gv, dev, hidden, TIGHT_PASS)


@pytest.mark.parametrize("in_dim,kfw", M.NEW_WIDTHS)
def test_new_instance_on_a_decoder_shaped_pass(gv, dev, in_dim, kfw):
    """8 rows x 8 frames (one quarter-full row tile); KFW 11, the instance with the largest LDS image, also at 40 rows: a second row
    tile of which 8 rows live."""
    import width_util as W
    ctx = gv._lib().new_context()       # (no status sink: the pass reports into its workspace, which EvalNet reads back)
    try:
        mem = W.TorchMem(ctx, dev)
        M.check_new_instance(mem, in_dim, kfw, 8)
        if kfw == 11:
            M.check_new_instance(mem, in_dim, kfw, 40)
    finally:
        torch.cuda.synchronize()
        ctx.close()


def test_chain_hu1024_twelve_speakers_against_the_float64_reference(gv, dev):
    """B 4, T 8, decoder in_dim 44 (KFW 7): fresh chain with per-cycle inputs."""
    M.check_chain_parity(gv, dev, M.problem_h1024(), "gauss", TIGHT_CHAIN, "device H1024 12 speakers")


def test_step_hu1024_twelve_speakers_against_the_float64_reference(gv, dev):
    M.check_step_parity(gv, dev, M.problem_h1024(), forms=(True,), what="device H1024 12 speakers")
