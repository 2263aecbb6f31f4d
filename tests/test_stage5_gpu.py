"""Stage 5 (converted-GV statistics) on the MI355X: the cases of tests/test_stage5_cpu.py on the device (bounds and yardsticks
there and in tests/stage5_util.py; PARITY UNPINNED for the DTW and calc_mcd halves), and one CvgvPass call at H = 1024 with
n_smpl_dec = 300 Philox draws."""
import numpy as np
import pytest
from conftest import have_hdf5

import stage5_util as S
import validation_util as VU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    import gru_vae
    assert torch.cuda.is_available()
    return VU.TorchBackend(gru_vae._lib(), torch.device("cuda:0"))


@pytest.mark.parametrize("n", [1, 2, 300])
@pytest.mark.parametrize("L", [4, 6, 50])
def test_latent_mean_injected_eps(be, L, n):
    """1. jobs of 1, 7 and 33 frames in one launch against the oracle at 2e-6; rows behind a job's frames untouched."""
    S.check_latent_mean_injected(be, L, n)


def test_latent_mean_twenty_jobs(be):
    """1. twenty jobs, the most a stage-5 call issues."""
    S.check_latent_mean_injected(be, 6, 2, frames=tuple(range(1, 21)))


def test_latent_mean_more_blocks_than_the_grid_cap(be):
    """A job whose items (frames x dim quads) exceed the 1024 blocks of 256 threads a job gets: the grid-stride loop."""
    S.check_latent_mean_injected(be, 50, 1, frames=(3, 21000))


@pytest.mark.parametrize("L", [4, 50])
def test_latent_mean_philox_is_the_injected_form(be, L):
    """2. Philox and injected draws agree bit for bit (the draws read back through cvae_sample_cat's eps_out at B = 1)."""
    S.check_latent_mean_philox(be, L)


def test_new_stat_kinds_beside_the_existing_ones(be):
    """3. MEANSTD64 and MCD64 against numpy float64 at 1e-12 relative, in one launch together with every existing kind."""
    arrays, cases = S.stat_cases()
    VU.assert_stats(VU.run_stats(be, arrays, cases), cases)


def test_cvgv_pass_end_to_end(be):
    """4. three pairs as 2 + 1 at H = 64 and as one call of three (stage5_util.run_e2e)."""
    S.run_e2e(be.dev)


def test_cvgv_mean_closes_the_loop_with_the_gv_postfilter(be):
    """5."""
    S.run_closing_the_loop(be.dev)


def test_library_calls_do_not_depend_on_the_number_of_pairs(be, monkeypatch):
    """6."""
    S.run_launch_count(be.dev, monkeypatch)


def test_h1024_philox_finite_and_row_independent(be):
    """7. in 54 / out 50 / lat 32 at H = 1024, two pairs of about 60 frames, n_smpl_dec = 300, Philox.  Every figure is finite, and
    (i) the metric half on IDENTICAL trajectories for pair 0 alone gives pair 0 the figures of the two-pair call bit for bit."""
    lens = ((60, 55), (52, 58))
    P, items, _, y, gv = S.problem(tag="s5/1024", lens=lens, n_smpl=1, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05)
    cp = S.make_pass(P, be.dev, gv, 300)
    dev_items = [S.to_dev(it, be.dev) for it in items]
    got = cp.pairs(dev_items, *S.to_dev(y, be.dev), seed=20190721)
    for r in got:
        assert all(np.all(np.isfinite(v)) for v in r.values()), r
    assert all(np.all(np.isfinite(v)) for v in cp.summary().values())
    lf = cp.last_passes[0]["lat_feat"].cpu().numpy()
    assert lf.shape == (60, 32) and 0.0 < float(np.std(lf - cp.last_passes[0]["lat_src"].cpu().numpy()[:, :32])) < 1.0      # (300 draws were averaged in)
    alone = cp.metrics(dev_items[:1], cp.last_passes[:1])
    S.same_figures(got[0], alone[0], "pair 0 alone against the two-pair call")


@pytest.mark.skipif(not have_hdf5(), reason="no HDF5 C library on this machine")
def test_write_and_run_files(be, tmp_path):
    """8."""
    S.run_files_and_write(be.dev, tmp_path)


def test_bad_speech_frame_index_gives_nan_for_that_pair_only(be):
    """9."""
    S.run_bad_spcidx(be.dev)
