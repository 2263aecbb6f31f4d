"""Emulator stage of the hidden-width tests: every row of the case table of tests/width_util.py with H <= 192, on the host-fiber
build of the real library (tests/emu), against the float64 references of tests/width_ref.py.

The library accepts any hidden width that is a positive multiple of 16, and the kernels that carry "any H" have width-dependent
code -- word and wave masks of k_gru_steps_ll, the K split over four waves of k_gru_steps<PERSIST> and k_outproj, the double-buffered
chunk loop of k_gru_step_train with its clamped tail, the partial blocks of k_gru_step_bwd, the slices of k_bwd_step_gemm -- that
the widths of the other tests (32, 64, 1024, 2048) never reach.  width_util's header lists what each width of the table reaches.

Bounds: the emulator bounds the project already uses, unchanged -- eval EMU_PASS = 5e-5 per pass (tests/stacked_util.py); training
5e-5 on outputs and carried state, 1e-4 on dx and the parameter gradients, relative to each tensor's largest entry
(tests/test_emu_train.py).  The float64 reference's own distance to its float32 form is below 5e-7 on these problems.

Rows that take much longer than 10 s here run in tests/test_width_gpu.py only, and the others run with fewer frames than there:
width_util.emu_case lists both.  The whole file takes about four minutes in one process.  Every measured distance is printed
(run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to width_cpu_report.txt."""
import pytest

import width_util as wu
from emu_util import emu_lib

note = wu.make_note("width_cpu_report.txt")
ids = lambda cases: [c.id for c in cases]
emu = lambda cases: [wu.emu_case(c) for c in cases if wu.emu_case(c) is not None]


@pytest.fixture(scope="module")
def lib():
    """A context of its own on the emulator library: options and the status sink set here never reach other tests."""
    ctx = emu_lib().new_context()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def mem(lib):
    return wu.NpMem(lib)


@pytest.fixture(scope="module")
def refs():
    """case -> float64 reference, computed once per case and module."""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = wu.train_reference(c) if isinstance(c, wu.TrainCase) else wu.eval_reference(c)
        return cache[c]
    return get


def test_the_emulator_stage_covers_every_width_up_to_192_and_every_row_class():
    for table in (wu.EVAL_CASES, wu.TRAIN_CASES, wu.PROJ_CASES, wu.DEEP_CASES):
        assert {c.H for c in emu(table)} == {c.H for c in table if c.H <= wu.EMU_MAX_H}
    assert {c.H for c in emu(wu.EVAL_CASES)} == {16, 48, 80, 128, 144, 192} and {c.H for c in emu(wu.TRAIN_CASES)} == {16, 48, 80, 144}
    for form, rows in ((wu.LL, {1, 2, 3}), (wu.GENERIC, {5, 17, 65}), (wu.PER_STEP, {5})):
        assert {c.rows for c in emu(wu.EVAL_CASES) if c.form == form} == rows
    # every (kind, carry, T = 1, option) class of the train table
    cls = lambda c: (c.H, c.kind, c.carry, c.T == 1, c.opts)
    assert {cls(c) for c in emu(wu.TRAIN_CASES)} == {cls(c) for c in wu.TRAIN_CASES if c.H <= wu.EMU_MAX_H}


@pytest.mark.parametrize("c", emu(wu.EVAL_CASES), ids=ids(emu(wu.EVAL_CASES)))
def test_eval_pass_at_width(mem, refs, c):
    """Whole pass (planned form asserted), two windows with the carried state, h_in with an off-manifold y_in, T = 1; at the
    GENERIC rows also the per-step launches, bit for bit."""
    wu.run_eval_case(mem, c, refs(c), note, wu.EMU_PASS)


@pytest.mark.parametrize("c", emu(wu.PROJ_CASES), ids=["%s-out%d" % (c.id, 2 * c.lat) for c in emu(wu.PROJ_CASES)])
def test_projection_classes_at_width(mem, refs, c):
    wu.run_proj_case(mem, c, refs(c), note, wu.EMU_PASS)


@pytest.mark.parametrize("c", emu(wu.DEEP_CASES), ids=ids(emu(wu.DEEP_CASES)))
def test_stacked_gru_at_width(mem, refs, c):
    """hidden_layers = 2 through the _deep entry points, against frontend_ref.forward."""
    wu.run_eval_case(mem, c, refs(c), note, wu.EMU_PASS)


@pytest.mark.parametrize("c", emu(wu.TRAIN_CASES), ids=ids(emu(wu.TRAIN_CASES)))
def test_train_pass_at_width(mem, refs, options, c):
    """Forward + backward of one train-mode pass with injected masks: outputs, carried state, dx and the ten gradients."""
    options(**dict(c.opts))
    wu.run_train_case(mem, c, refs(c), note, wu.EMU_TRAIN_OUT, wu.EMU_TRAIN_GRAD)
