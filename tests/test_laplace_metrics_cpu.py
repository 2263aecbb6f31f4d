"""The Laplace posterior in the metric passes without a GPU: CVAE_STAT_KL_LAPLACE and cvae_trainlog_window's flag in the real library
on the host-fiber emulator, and validation.ValidationPass, stage5.CvgvPass, decode.DecodePass, trainlog.TrainLog / UttLog with
posterior="laplace" end to end on it.  The cases and their bounds are tests/laplace_metrics_util.py's; the yardstick is
tests/laplace_metrics_ref.py (the existing restatements with the Laplace clamp, draw and KL).

Bounds.  The two kernels against float64 numpy at 1e-12 (validation_util.assert_stats', trainlog_util.assert_records'), relative to
max(|ref|, mean_t sum_l (|s| + b exp(-|mu|/b) + |mu| + 1)) for a KL figure: the terms of one summand cancel, so the summand's
condition and not the result alone is what rounding is relative to.  End to end: a pass output within delta of the fp32 oracle
network, delta = 5e-6 (TIGHT_PASS, as the Gaussian end-to-end tests of both backends), or four times the oracle's own distance to
its float64 twin where that exceeds 1.25e-6 (frontend_util.bound_for's rule); a loss_mcd_* term then moves by at most K sqrt2 D delta
and a loss_lat_* term by at most L delta (2 + (1 + 1/e) exp(s_max + delta)) (|d/dmu| <= 1, |d/ds| <= 1 + b + b/e), plus 1e-6
relative for the reference's own fp32 sums.  Figures of the metric half on the library's own trajectories: 1e-10 relative.

As in tests/test_trainlog_cpu.py the emulated training step is slow, so the logs' end-to-end cases run around stand-in
trajectories; the step itself (unfused) stands in the two loss-identity cases, on one window / one utterance."""
import pytest

import _cabi
import laplace_metrics_util as U
import validation_util as VU
from emu_util import bind_emulator, emu_lib


@pytest.fixture(scope="module")
def be():
    return VU.NpBackend(emu_lib())


@pytest.fixture
def dev(monkeypatch):
    import torch
    bind_emulator(monkeypatch)
    return torch.device("cpu")


def test_abi_stays_10_and_the_kind_is_8(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10 and _cabi.STAT_KL_LAPLACE == 8


def test_stat_kind_against_numpy_float64(be):
    """1. rows 1, 17 and 300 (two rows for some threads), L = 5 in rows of 13, mu == 0, log-scales on the floor and up to +3."""
    U.check_stat_kind(be)


def test_window_kernel_with_the_flag(be):
    """2. entries [3], [4] against the restatement, everything else and the accumulators bit-identical to the call without the
    flag, every utterance alone against the launch of three, and the flag without a dimension refused."""
    U.check_window_kernel(be)


def test_validation_pass_end_to_end(dev):
    U.run_validation_e2e(dev)


def test_cvgv_pass_end_to_end_and_convert_pairs_bits(dev):
    U.run_pairs_e2e("cvgv", dev)


def test_decode_pass_end_to_end_and_convert_pairs_bits(dev):
    U.run_pairs_e2e("decode", dev)


def test_trainlog_end_to_end(dev):
    U.run_trainlog_e2e(dev)


def test_uttlog_end_to_end(dev):
    U.run_uttlog_e2e(dev)


def test_trainlog_window_loss_is_the_sum_of_the_logged_terms(dev):
    """4. TrainLog around an unfused Stage4Step(posterior="laplace"), one window of three utterances."""
    got = U.drive_trainlog(dev, real_step=True, fused=False, n_batches=1, windows_per_batch=1, close=False)
    assert len(got["records"]) == 1 and got["floor"] > 0
    U.check_window_loss_is_the_logged_sum(got)


def test_uttlog_step_loss_is_the_sum_of_the_logged_terms(dev):
    """4. UttLog around an unfused Stage4Step(posterior="laplace"), one utterance of nine frames."""
    got = U.drive_uttlog(dev, seq=((0, [2]),), real_step=True, fused=False)
    assert len(got["records"]) == 1 and got["floor"] > 0
    U.check_utt_loss_is_the_logged_sum(got)


def test_validation_posterior_gauss_is_the_default_bit_for_bit(dev):
    U.check_validation_gauss_is_default(dev)


@pytest.mark.parametrize("kind", ["cvgv", "decode"])
def test_pairs_posterior_gauss_is_the_default_bit_for_bit(dev, kind):
    U.check_pairs_gauss_is_default(kind, dev)


def test_logs_posterior_gauss_is_the_default_bit_for_bit(dev):
    U.check_logs_gauss_is_default(dev)


def test_unknown_posterior_is_refused():
    U.check_refusals()
