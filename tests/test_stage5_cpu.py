"""Stage 5 (converted-GV statistics) without a GPU: cvae_latent_mean and the two stage-5 statistics kinds of the real library on
the host-fiber emulator, and stage5.CvgvPass end to end on it.

Yardsticks: oracle.sampling_vae_batch(...).mean(0) (the latent mean, 2e-6: the bound tests/test_oracle_golden.py holds the
oracle's own z to; the mean adds at most one fp32 rounding of the eps mean), numpy float64 (statistics kinds, 1e-12 relative),
the oracle network (trajectories, 5e-6) and tests/stage5_ref.py, the restatement of calc_cvgv_gru-cyclevae_gauss.py:179-283 and
:320-344, run on the library's own trajectories (figures, 1e-10 relative).  PARITY UNPINNED for the DTW and calc_mcd halves
(stage5_ref)."""
import numpy as np
import pytest
from conftest import have_hdf5

import _cabi
import stage5_util as S
import validation_util as VU
from emu_util import bind_emulator, emu_lib


@pytest.fixture(scope="module")
def be():
    return VU.NpBackend(emu_lib())


@pytest.fixture
def emu_gru_vae(monkeypatch):
    return bind_emulator(monkeypatch)


def test_abi_stays_10_and_the_export_is_bound(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10
    assert "cvae_latent_mean" in _cabi.EXPORTS and hasattr(be.lib.lib, "cvae_latent_mean")
    assert (_cabi.STAT_MEANSTD64, _cabi.STAT_MCD64) == (6, 7)


@pytest.mark.parametrize("n", [1, 2, 300])
@pytest.mark.parametrize("L", [4, 6, 50])
def test_latent_mean_injected_eps(be, L, n):
    """1. jobs of 1, 7 and 33 frames in one launch against the oracle; rows behind a job's frames untouched."""
    S.check_latent_mean_injected(be, L, n)


def test_latent_mean_twenty_jobs(be):
    """1. twenty jobs, the most a stage-5 call issues, of 1 .. 20 frames."""
    S.check_latent_mean_injected(be, 6, 2, frames=tuple(range(1, 21)))


@pytest.mark.parametrize("L", [4, 50])
def test_latent_mean_philox_is_the_injected_form(be, L):
    """2. Philox and injected draws agree bit for bit (the draws read back through cvae_sample_cat's eps_out at B = 1)."""
    S.check_latent_mean_philox(be, L)


def test_latent_mean_more_jobs_than_one_launch_holds(be):
    """40 jobs: the entry point runs them as two launches of at most 32."""
    S.check_latent_mean_injected(be, 4, 2, frames=tuple(1 + q % 5 for q in range(40)))


def test_latent_mean_refuses_bad_arguments(be):
    lat, eps = S.latmean_inputs("bad", 3, 4, 2)
    out = np.zeros((3, 4), np.float32)
    ok = _cabi.LatMeanJob(lat.ctypes.data, eps.ctypes.data, 0, 3, 0, out.ctypes.data)
    be.lib.latent_mean([ok], 4, 2)
    for jobs, L, n in (([ok], 0, 2), ([ok], 4, 0), ([], 4, 2), ([_cabi.LatMeanJob(lat.ctypes.data, None, 0, 0, 0, out.ctypes.data)], 4, 2),
                       ([_cabi.LatMeanJob(None, None, 0, 3, 0, out.ctypes.data)], 4, 2), ([_cabi.LatMeanJob(lat.ctypes.data, None, 0, 3, 0, None)], 4, 2)):
        with pytest.raises(_cabi.CvaeError, match="cvae_latent_mean"):
            be.lib.latent_mean(jobs, L, n)


def test_new_stat_kinds_beside_the_existing_ones(be):
    """3. MEANSTD64 and MCD64 against numpy float64 at 1e-12 relative, in one launch together with every existing kind."""
    arrays, cases = S.stat_cases()
    VU.assert_stats(VU.run_stats(be, arrays, cases), cases)


def test_cvgv_pass_end_to_end(emu_gru_vae):
    """4. three pairs as 2 + 1 at H = 64 (bounds in stage5_util.run_e2e), and as one call of three: the same figures bit for bit."""
    import torch
    S.run_e2e(torch.device("cpu"))


def test_cvgv_mean_closes_the_loop_with_the_gv_postfilter(emu_gru_vae):
    """5. stage6.gv_postfilter with this pass's cvgv_mean of the same utterance yields exactly the target speaker's GV."""
    import torch
    S.run_closing_the_loop(torch.device("cpu"))


def test_library_calls_do_not_depend_on_the_number_of_pairs(emu_gru_vae, monkeypatch):
    """6."""
    import torch
    S.run_launch_count(torch.device("cpu"), monkeypatch)


@pytest.mark.skipif(not have_hdf5(), reason="no HDF5 C library on this machine")
def test_write_and_run_files(emu_gru_vae, tmp_path):
    """8."""
    import torch
    S.run_files_and_write(torch.device("cpu"), tmp_path)


def test_bad_speech_frame_index_gives_nan_for_that_pair_only(emu_gru_vae):
    """9."""
    import torch
    S.run_bad_spcidx(torch.device("cpu"))


def test_refuses_more_than_ten_pairs_and_cpu_tensors():
    """9. the real gru_vae (no emulator binding): CPU tensors are refused, as is a call of eleven pairs."""
    import torch
    P, items, eps, y, gv = S.problem()
    cp = S.make_pass(P, torch.device("cpu"), gv, 3)
    ty = S.to_dev(y, "cpu")
    with pytest.raises(RuntimeError, match="HIP device only"):
        cp.pairs([S.to_dev(items[0], "cpu")], *ty, eps=[S.to_dev(eps[0], "cpu")])
    with pytest.raises(ValueError, match="pairs per call"):
        cp.pairs([S.to_dev(items[0], "cpu")] * 11, *ty)
    with pytest.raises(ValueError, match="pairs per call"):
        cp.pairs([], *ty)
    with pytest.raises(RuntimeError, match="no pair seen"):
        cp.summary()
