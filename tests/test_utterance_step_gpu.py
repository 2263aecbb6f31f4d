"""The stage-4 step on whole padded utterances (batch_size == 0, train_gru_cyclevae_gauss_batch.py:1491-1653) on the MI355X:
stage4.Stage4Step through stage4.utterance_step_args against the stock-torch checker with dropout 0.5 and injected masks and eps, at
frame counts the train-mode kernels, tape and scratch had not seen (the largest before: T = 80).  Cases, bounds and the padding
argument: tests/utterance_step_util.py.

Measured on one MI355X (largest gradient distance device vs the fp32 checker; the checker's own fp32-vs-float64 distance for that
tensor; Stage4Step.fallbacks): profiles/utterance_mode_notes.md."""
import numpy as np
import pytest

import utterance_step_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_RUNS = {}


def run(name, dev):
    """The case's device step and the checker's, once per module."""
    if name not in _RUNS:
        P, items, masks = U.problem(name)
        _RUNS[name] = (U.device_step(P, items, masks, dev), U.reference(name, P, items, masks))
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_utterance_step_vs_cpu_checker(dev, name):
    """Loss within 1e-5 relative of the checker's; every gradient tensor within its bound (TIGHT_REL, or four times the checker's own
    fp32-vs-float64 distance where that exceeds TIGHT_REL / 4).  Stage4Step.fallbacks is printed: a status-5 repeat is legitimate."""
    (loss, grads, fallbacks), (ref_loss, ref_grads) = run(name, dev)
    print("%s: loss device %.6f checker %.6f (rel %.2e); fallbacks %d" % (name, loss, ref_loss, abs(loss - ref_loss) / abs(ref_loss), fallbacks))
    bounds = U.bounds(name)
    assert sorted(bounds) == sorted(grads) == sorted(ref_grads)
    bad = []
    for k in sorted(grads):
        assert np.all(np.isfinite(grads[k])), k
        d = U.distance(grads[k], ref_grads[k])
        print("%-16s %-28s device %.2e   checker fp32 vs f64 %.2e   bound %.2e" % (name, k, d, bounds[k][1], bounds[k][0]))
        if d > bounds[k][0]:
            bad.append((k, d, bounds[k][0]))
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_padding_content_does_not_reach_loss_or_gradients(dev, name):
    """batch_src and batch_cv_src refilled with other finite values of the features' law from frame flens[j] + 32 on (8 chained
    passes x the front-end's reach of 4: utterance_step_util): loss and every gradient bit-identical."""
    (loss, grads, _), _ = run(name, dev)
    P, items, masks = U.problem(name, refill=True)
    P0, items0, _ = U.problem(name)
    assert not np.array_equal(items[0], items0[0]) and not np.array_equal(items[4], items0[4])      # (the case has padding to refill)
    loss2, grads2, _ = U.device_step(P, items, masks, dev)
    assert loss2 == loss, (loss, loss2)
    for k in sorted(grads):
        assert np.array_equal(grads[k], grads2[k]), (k, U.distance(grads2[k], grads[k].astype(np.float64)))
