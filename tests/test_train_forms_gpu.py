"""Device stage of the training-form tests: EVERY row of the case table of tests/train_cases.py on the MI355X -- H = 64 and
H = 1024, every recurrence form plan_train_pass chooses at every row-tile class -- against the float64 references of
tests/width_ref.py.  python -m pytest tests -m gpu

Each row asserts that no option is left over from another test, sets its own, asserts the whole plan (cvae_plan_train_pass) and
only then runs, through width_util.TrainNet.run on a context of its own: every buffer exactly its queried size inside one NaN-filled device
allocation (a pass that reads or writes past a buffer, or reads a dead row nobody wrote, fails the comparison or the guard check; it
cannot fault), status sink zero, every output element written.  One train image per (H, kind) serves all rows.

What the emulator stage (tests/test_train_forms_cpu.py) cannot see: the device build of the cooperative polling kernels, and every
H = 1024 instance -- <8, 4, ..> of the exact forms, k_train_fwd_steps_x3<16>, k_train_bwd_steps_x3<32> over several launches,
k_train_fwd_steps<32>, k_train_fwd_steps_h<16> / k_train_bwd_steps<32>.

Bounds, relative to each tensor's largest entry: TIGHT_REL = 8e-6 (tests/test_gpu_train.py, the project's own) on outputs and
gradients of the exact-operand, word-exchange and per-step forms.  The fp16-pair and fp32-MFMA forms had no device bound; theirs are
twice the worst distance measured on the device at the table's rows, rounded up to one digit, and never above the emulator's
5e-5 / 1e-4 (profiles/train_forms_notes.md has the measurements):
    pair forms (train_kernel 1, both directions)       outputs PAIR_OUT, gradients PAIR_GRAD
    fp32-MFMA forward (its reverse is the exact one)   outputs FP32_OUT, gradients FP32_GRAD
Every measured distance is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to
train_forms_gpu_report.txt."""
import pytest

import train_cases as tc
import width_util as wu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_train import TIGHT_REL      # noqa: E402  (the project's device bound for training tensors)

PAIR_OUT, PAIR_GRAD = 6e-7, 7e-7          # measured 2.87e-7 / 3.37e-7
FP32_OUT, FP32_GRAD = 6e-7, 9e-7          # measured 2.71e-7 / 4.37e-7
assert PAIR_OUT <= tc.EMU_TRAIN_OUT and FP32_OUT <= tc.EMU_TRAIN_OUT and PAIR_GRAD <= tc.EMU_TRAIN_GRAD and FP32_GRAD <= tc.EMU_TRAIN_GRAD

note = wu.make_note("train_forms_gpu_report.txt")
ids = lambda cases: [c.id for c in cases]
GROUPS = tc.tiling_groups(tc.FORM_CASES)


def bounds(c):
    if c.plan[1] == tc.F_PAIR or c.plan[4] == tc.B_PAIR:
        return PAIR_OUT, PAIR_GRAD
    if c.plan[1] == tc.F_FP32:
        return FP32_OUT, FP32_GRAD
    return TIGHT_REL, TIGHT_REL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """A context of its own on the loaded library: options and the status sink set here never reach the passes of other tests."""
    import gru_vae
    ctx = gru_vae._lib().new_context()
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(scope="module")
def runner(lib, dev):
    return tc.Runner(wu.TorchMem(lib, dev), note)


@pytest.mark.parametrize("c", tc.FORM_CASES, ids=ids(tc.FORM_CASES))
def test_train_pass_in_form(runner, options, c):
    """Plan, then forward + backward of one train-mode pass with injected masks: outputs, carried state, dx and the ten gradients."""
    runner.check(c, options, *bounds(c))


@pytest.mark.parametrize("key", list(GROUPS), ids=["h%d-r%d-%s+%s" % (k[0][0], k[0][1], tc.FWD_NAMES[k[1]], tc.BWD_NAMES[k[2]]) for k in GROUPS])
def test_same_form_other_tiling_gives_identical_bits(runner, options, key):
    """One problem in the same exact-operand forms under every tiling of the table: identical bits of out, y_last, h_last and dx."""
    tc.run_tiling_group(runner, GROUPS[key], options)


@pytest.mark.parametrize("big,small", tc.PREFIX, ids=[b.id for _, b in tc.PREFIX])
def test_rows_of_a_larger_pass_equal_a_pass_of_their_own(runner, options, big, small):
    """Rows 0..15 of the 33-row pass against the same rows as a 16-row pass of the same forms, to the reference bound."""
    tc.run_prefix(runner, big, small, options, TIGHT_REL, TIGHT_REL)


PROBE = tc.PROBE_CASES + tc.PROBE_CONTROLS


@pytest.mark.parametrize("c", PROBE, ids=ids(PROBE))
def test_planned_forward_ran_and_not_its_per_step_fallback(runner, options, c):
    """The fp16-pair and fp32-MFMA forwards fall back to per-step launches at run time when their launch fails, within every bound
    here: with train_prof the persistent kernel leaves its counters in the scratch, the per-step launches (control rows) do not."""
    tc.run_fallback_probe(runner, c, options)
