"""The Laplace posterior in the metric passes on the MI355X: tests/test_laplace_metrics_cpu.py's cases on the device (bounds and
their derivation there), the logs around the FUSED Stage4Step(posterior="laplace"), and two cases the emulator is too slow for: one
ValidationPass.batch at H = 1024 with Philox draws, and a CvgvPass of two-layer networks against stage6.convert_pairs."""
import pytest

import _cabi
import laplace_metrics_util as U
import validation_util as VU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    import gru_vae
    return VU.TorchBackend(gru_vae._lib(), dev)


@pytest.fixture(scope="module")
def trainlog_run(dev):
    return U.run_trainlog_e2e(dev)


@pytest.fixture(scope="module")
def uttlog_run(dev):
    return U.run_uttlog_e2e(dev)


def test_abi_stays_10_and_the_kind_is_8(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10 and _cabi.STAT_KL_LAPLACE == 8


def test_stat_kind_against_numpy_float64(be):
    U.check_stat_kind(be)


def test_window_kernel_with_the_flag(be):
    U.check_window_kernel(be)


def test_validation_pass_end_to_end(dev):
    U.run_validation_e2e(dev)


def test_cvgv_pass_end_to_end_and_convert_pairs_bits(dev):
    U.run_pairs_e2e("cvgv", dev)


def test_decode_pass_end_to_end_and_convert_pairs_bits(dev):
    U.run_pairs_e2e("decode", dev)


def test_trainlog_end_to_end(trainlog_run):
    """Two utterance batches of three windows each around the fused Laplace step; the figures, lines and the epoch line."""
    assert len(trainlog_run["records"]) == 6


def test_trainlog_window_loss_is_the_sum_of_the_logged_terms(trainlog_run):
    U.check_window_loss_is_the_logged_sum(trainlog_run)


def test_uttlog_end_to_end(uttlog_run):
    assert len(uttlog_run["records"]) == 2


def test_uttlog_step_loss_is_the_sum_of_the_logged_terms(uttlog_run):
    U.check_utt_loss_is_the_logged_sum(uttlog_run)


def test_validation_posterior_gauss_is_the_default_bit_for_bit(dev):
    U.check_validation_gauss_is_default(dev)


@pytest.mark.parametrize("kind", ["cvgv", "decode"])
def test_pairs_posterior_gauss_is_the_default_bit_for_bit(dev, kind):
    U.check_pairs_gauss_is_default(kind, dev)


def test_logs_posterior_gauss_is_the_default_bit_for_bit(dev):
    U.check_logs_gauss_is_default(dev)


def test_unknown_posterior_is_refused():
    U.check_refusals()


def test_validation_pass_h1024_philox_finite_and_row_independent(dev):
    U.run_validation_h1024(dev)


def test_cvgv_pass_two_layer_networks_are_convert_pairs_bit_for_bit(dev):
    """hidden_layers = 2 at H = 64: the five trajectories of every pair equal stage6.convert_pairs(posterior="laplace"), the figures
    the restatement's on them, and grouping changes nothing (no float64 twin of the stacked network: the bits are the check)."""
    U.run_pairs_e2e("cvgv", dev, layers=2, check_net=False)
