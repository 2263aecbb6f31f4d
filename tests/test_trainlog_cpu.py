"""The training loop's per-window monitoring without a GPU: cvae_trainlog_window of the real library on the host-fiber emulator, and
trainlog.TrainLog end to end on it.  The emulated stage4.Stage4Step takes minutes for a handful of windows, so here the end-to-end
case feeds the monitor stand-in trajectories and a stand-in loss where the step would stand (trainlog_util.drive); the real step
drives the same body in tests/test_trainlog_gpu.py, which also holds the parameters bit-identical with and without the monitor.

Yardstick: tests/trainlog_ref.py (numpy float64 restatement of train_gru_cyclevae_gauss_batch.py:660-739, :1312-1472).  PARITY
UNPINNED for the dtw_org_to_trg / calc_mcd halves: dtw_c is not in the reference tree, the oracle's written definitions stand in.
Tolerances: the kernel against the restatement at 1e-12 relative (both float64 on the same fp32 values; the sums differ in order
only: at most 8 * 26 terms of one sign per figure, i.e. a few hundred ulp of 1.1e-16); the end-to-end figures at 1e-10 relative
(means and standard deviations of such figures, DTW means over paths both sides agree on)."""
import numpy as np
import pytest

import _cabi
import trainlog_util as U
from emu_util import bind_emulator, emu_lib


@pytest.fixture(scope="module")
def be():
    return U.NpBackend(emu_lib())


def test_abi_version_and_export(be):
    assert _cabi.ABI_VERSION == 10 and be.lib.lib.cvae_abi_version() == 10
    assert "cvae_trainlog_window" in _cabi.EXPORTS and hasattr(be.lib.lib, "cvae_trainlog_window")


def test_window_kernel_against_the_restatement(be):
    """(a) three windows that between them take every branch of the kernel; accumulators bit-equal to the concatenated windows."""
    U.check_kernel_alone(be)


def test_window_kernel_index_outside_the_window(be):
    U.check_bad_index(be)


def test_window_kernel_grid_independence(be):
    U.check_grid_independence(be)


def test_window_kernel_refuses_bad_arguments(be):
    U.check_refusals(be)


@pytest.fixture
def emu_gru_vae(monkeypatch):
    return bind_emulator(monkeypatch)


@pytest.mark.parametrize("with_sentinel", [True, False], ids=["sentinel_between_batches", "two_batches_one_pass"])
def test_trainlog_end_to_end(emu_gru_vae, with_sentinel):
    """(b) two utterance batches through before / (stand-in step) / after at H = 64; without a sentinel between them the GV rule of
    :1339-1348 fires, with one (the reference generator's flow) the epoch line prints nan for the GV figures.  The encoder pass of
    before() is the emulated library's; it is most of the case's ~25 s."""
    import torch
    U.check_e2e(torch.device("cpu"), with_sentinel)


def test_trainlog_refuses_utterance_length_batches_and_cpu_tensors():
    import torch
    import trainlog
    from validation_util import modules
    import synth
    P = synth.CycleVAEProblem(B=3, T=8, tag="tl/refuse", **U.H64)
    enc, dec = modules(P, torch.device("cpu"))
    tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, np.ones(25), np.ones(25), spk_src=U.SPK_SRC)
    with pytest.raises(NotImplementedError, match="batch_size"):
        tl.before(tuple([] for _ in range(16)), None)
    items = next(U.yields(U.e2e_batches(P, "tl/refuse")[0], 8, torch.from_numpy))
    with pytest.raises(RuntimeError, match="HIP device only"):
        tl.before(items, torch.from_numpy(P.y_in_enc))
