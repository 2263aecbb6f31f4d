"""Stage 6 (post-processing and metrics of decode_gru-cyclevae_gauss.py) on the MI355X: the cases of tests/test_decode_cpu.py on the
device (bounds and yardsticks there and in tests/decode_util.py; PARITY UNPINNED for the DTW, calc_mcd and mc2e parts), the batch
against the one-problem stage6.mc2e, and one DecodePass call at H = 1024 with n_smpl_dec = 300 Philox draws at irlen = 1024."""
import numpy as np
import pytest

import decode_util as U
import validation_util as VU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    import gru_vae
    assert torch.cuda.is_available()
    return VU.TorchBackend(gru_vae._lib(), torch.device("cuda:0"))


@pytest.mark.parametrize("D", [2, 25, 50])
@pytest.mark.parametrize("irlen", [2, 3, 63, 64, 65, 130])
def test_mc2e_batch_against_the_oracle(be, irlen, D):
    """1. jobs of 1, 7 and 33 frames in one call, fp32 and f64 mixed, ld > D; guard values behind every e_out survive."""
    U.check_mc2e_batch(be, irlen, D)


def test_mc2e_batch_at_the_recipe_irlen_and_against_stage6_mc2e(be):
    """1. irlen = 1024, D = 50, 37 frames (15 fp32 + 22 f64) against the oracle, and against the one-problem stage6.mc2e on the same
    matrices, both at 1e-11 relative."""
    import stage6
    mats, got = U.check_mc2e_batch(be, 1024, 50, frames=(15, 22))
    for m, (e, _) in zip(mats, got):
        one = stage6.mc2e(be.put(np.ascontiguousarray(m[:, :50])), U.ALPHA, 1024).cpu().numpy()
        d = float(np.max(np.abs(e / one - 1.0)))
        print("mc2e_batch against stage6.mc2e (%s): rel|d| = %.3e" % (m.dtype, d))
        assert d <= U.MC2E_REL, d


def test_mc2e_batch_24_jobs(be):
    """1. 24 jobs of different D in one call."""
    U.check_mc2e_many_jobs(be)


def test_mc2e_batch_refuses_bad_arguments(be):
    """7. irlen 1 / 4001 and bad jobs: status -1 with a message, before anything is launched."""
    U.check_mc2e_refusals(be)


@pytest.mark.parametrize("T", [1, 2, 37])
def test_decode_jobs_mod_pow_postfilter_difference(be, T):
    """2. jobs with and without the post-filter, both rounds, guard rows intact."""
    U.check_decode_jobs(be, T)


def test_decode_jobs_gather_and_refusals(be):
    U.check_decode_gather(be)
    U.check_decode_refusals(be)


def test_decode_pass_end_to_end(be):
    """3. three pairs as 2 + 1 at H = 64 and as one call of three (decode_util.run_e2e)."""
    U.run_e2e(be.dev)


def test_log_lines_are_the_scripts(be):
    """8."""
    U.run_log_lines(be.dev)


def test_library_calls_do_not_depend_on_the_number_of_pairs(be, monkeypatch):
    """4."""
    U.run_launch_count(be.dev, monkeypatch)


def test_cvgv_mean_of_stage5_closes_the_loop(be):
    """5."""
    U.run_closing_the_loop(be.dev)


def test_bad_speech_frame_index_gives_nan_for_that_pair_only(be):
    """6."""
    U.run_bad_spcidx(be.dev)


def test_argument_checks_before_anything_is_launched(be):
    """7."""
    U.run_argument_checks(be.dev)


def test_h1024_philox_finite_and_call_independent(be):
    """9. in 54 / out 50 / lat 32 at H = 1024, two pairs of about 60 frames, n_smpl_dec = 300 Philox draws, irlen = 1024.  Every
    figure is finite, and pair 0 from a one-pair call has the outputs it has in the two-pair call bit for bit."""
    lens = ((60, 55), (52, 58))
    P, items, _, y, stats = U.problem(tag="dec/1024", lens=lens, n_smpl=1, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05)
    dp = U.make_pass(P, be.dev, stats, n_smpl=300, irlen=1024)
    dev_items = [U.to_dev(it, be.dev) for it in items]
    ty = U.to_dev(y, be.dev)
    got = dp.pairs(dev_items, *ty, seed=20190721)
    for r in got:
        assert all(np.all(np.isfinite(v)) for v in U.host(r).values()), r
    assert all(np.all(np.isfinite(v)) for v in dp.summary().values())
    lf = dp.last_passes[0]["lat_feat"].cpu().numpy()
    assert lf.shape == (60, 32) and 0.0 < float(np.std(lf - dp.last_passes[0]["lat_src"].cpu().numpy()[:, :32])) < 1.0      # (300 draws were averaged in)
    assert len(dp.log_lines()) == 19
    alone = U.make_pass(P, be.dev, stats, n_smpl=300, irlen=1024, like=dp).pairs(dev_items[:1], *ty, seed=20190721)
    U.same_results(got[0], alone[0], "pair 0 alone against the two-pair call")
