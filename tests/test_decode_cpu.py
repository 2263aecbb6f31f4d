"""Stage 6 (post-processing and metrics of decode_gru-cyclevae_gauss.py) without a GPU: cvae_mc2e_batch and cvae_decode_jobs of the
real library on the host-fiber emulator, and decode.DecodePass end to end on it.

Yardsticks: oracle.mc2e (1e-11 relative, the project's bound for cvae_mc2e), oracle.mod_pow_dpow / gv_postfilter (1e-11 / 1e-10
absolute, the bounds of test_mc2e_and_mod_pow_on_device), the oracle network (trajectories, 5e-6) and tests/decode_ref.py, the
restatement of decode...:328-475 and :606-644, run on the library's own trajectories (1e-10 relative to an array's scale).  PARITY
UNPINNED for the DTW, calc_mcd and mc2e parts (decode_ref)."""
import pytest

import _cabi
import decode_util as U
import validation_util as VU
from emu_util import bind_emulator, emu_lib


@pytest.fixture(scope="module")
def be():
    return VU.NpBackend(emu_lib())


@pytest.fixture
def emu_gru_vae(monkeypatch):
    return bind_emulator(monkeypatch)


def test_abi_stays_10_and_the_exports_are_bound(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10
    for name in ("cvae_mc2e_batch", "cvae_mc2e_batch_work_bytes", "cvae_decode_jobs"):
        assert name in _cabi.EXPORTS and hasattr(be.lib.lib, name)


@pytest.mark.parametrize("D", [2, 25, 50])
@pytest.mark.parametrize("irlen", [2, 3, 63, 64, 65, 130])
def test_mc2e_batch_against_the_oracle(be, irlen, D):
    """1. jobs of 1, 7 and 33 frames in one call, fp32 and f64 mixed, ld > D; guard values behind every e_out survive."""
    U.check_mc2e_batch(be, irlen, D)


def test_mc2e_batch_at_the_recipe_irlen(be):
    """1. irlen = 1024, D = 50, 3 + 9 frames."""
    U.check_mc2e_batch(be, 1024, 50, frames=(3, 9))


def test_mc2e_batch_24_jobs(be):
    """1. 24 jobs of different D in one call."""
    U.check_mc2e_many_jobs(be)


def test_mc2e_batch_refuses_bad_arguments(be):
    """7. irlen 1 / 4001 and bad jobs: status -1 with a message."""
    U.check_mc2e_refusals(be)


@pytest.mark.parametrize("T", [1, 2, 37])
def test_decode_jobs_mod_pow_postfilter_difference(be, T):
    """2. jobs with and without the post-filter, both rounds, guard rows intact."""
    U.check_decode_jobs(be, T)


def test_decode_jobs_gather_and_refusals(be):
    U.check_decode_gather(be)
    U.check_decode_refusals(be)


def test_decode_pass_end_to_end(emu_gru_vae):
    """3. three pairs as 2 + 1 at H = 64 (bounds in decode_util.run_e2e), and as one call of three: bit for bit."""
    import torch
    U.run_e2e(torch.device("cpu"))


def test_log_lines_are_the_scripts(emu_gru_vae):
    """8."""
    import torch
    U.run_log_lines(torch.device("cpu"))


def test_library_calls_do_not_depend_on_the_number_of_pairs(emu_gru_vae, monkeypatch):
    """4."""
    import torch
    U.run_launch_count(torch.device("cpu"), monkeypatch)


def test_cvgv_mean_of_stage5_closes_the_loop(emu_gru_vae):
    """5."""
    import torch
    U.run_closing_the_loop(torch.device("cpu"))


def test_bad_speech_frame_index_gives_nan_for_that_pair_only(emu_gru_vae):
    """6."""
    import torch
    U.run_bad_spcidx(torch.device("cpu"))


def test_argument_checks_before_anything_is_launched(emu_gru_vae):
    """7."""
    import torch
    U.run_argument_checks(torch.device("cpu"))
