"""The training loop's monitoring on utterance-length mini-batches (batch_size == 0) on the MI355X: tests/test_uttlog_cpu.py's
end-to-end case with stage4.Stage4Step itself between before() and after() (H = 64, injected eps and dropout masks; the step's
arguments come from stage4.utterance_step_args).  Yardstick and tolerance as in the CPU file: tests/uttlog_ref.py on the library's own
trajectories and encoder pass, 1e-10 relative (PARITY UNPINNED for the DTW / calc_mcd halves)."""
import numpy as np
import pytest

import uttlog_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def e2e(dev):
    """The two-batch run with the monitor (checked against the restatement and against the run without a monitor), shared."""
    return U.check_e2e(dev)


def test_uttlog_end_to_end(e2e):
    """Figures within 1e-10 relative of uttlog_ref, text lines equal, parameters bit-identical with and without the monitor (all
    asserted by check_e2e); no step was repeated with the fp32 reverse recurrence."""
    print("Stage4Step.fallbacks = %d" % e2e["fallbacks"])
    assert len(e2e["records"]) == 2


def test_step_loss_is_the_sum_of_the_logged_terms(e2e):
    """The step's loss (fp32, cvae_stage4_loss with the utterance branch's lists) against the sum over cycles and utterances of the
    four logged terms (:1636-1641; the record's float64 figures from the same trajectories): 1e-5 relative, the bound
    test_stage4_step_vs_cpu_checker puts on a loss.  The window branch's list quirk (:1393) would add ~KL(lat) - KL(latcv) here."""
    assert len(e2e["losses"]) == 2
    for k, R in enumerate(e2e["ref_records"]):
        want = float(np.sum(R[:, :, [0, 1, 3, 4]]))
        print("step %d: loss %.6f, sum of the logged terms %.6f" % (k, e2e["losses"][k], want))
        assert abs(e2e["losses"][k] - want) <= 1e-5 * abs(want), (k, e2e["losses"][k], want)


def test_uttlog_lagged_step_lines_drained_late(dev, e2e):
    """Stage4Step(sync=False) and lines() called only behind the sentinel: the same lines, the same epoch figures and the same
    parameters as the synchronous run that drains every step."""
    late = U.drive(dev, sync=False, drain_every_step=False)
    assert late["lines"] == e2e["lines"]
    assert late["summary"]["line"] == e2e["summary"]["line"]
    for a, b in zip(late["params"], e2e["params"]):
        assert np.array_equal(a, b)
