"""Emulator stage of the training-form tests: the case table of tests/train_cases.py on the host-fiber build of the real library
(tests/emu) -- the plan of EVERY row, H = 1024 included (the plan needs no run; the emulator reports 256 CUs, as the MI355X does), and
the pass of every H = 64 row against the float64 reference of tests/width_ref.py.

Each row asserts that no option is left over from another test, sets its own, asserts the whole plan (cvae_plan_train_pass) and
only then runs, through width_util.TrainNet.run: every buffer exactly its queried size inside a NaN-filled arena, guards, status
sink and "every output element written" checked.  Bounds: the emulator's training bounds, unchanged -- EMU_TRAIN_OUT = 5e-5 on
outputs and carried state, EMU_TRAIN_GRAD = 1e-4 on dx and the parameter gradients, relative to each tensor's largest entry.

Two further checks between rows: a problem run in the same exact-operand forms under several tilings gives identical bits of out,
y_last, h_last and dx (a row's arithmetic does not depend on the block that owns it; the eval twin is in tests/test_frontend_cpu.py
and stacked_cases.TILINGS), and rows 0..15 of a 33-row pass equal the same rows run as a 16-row pass of the same forms to the
reference bound (rows are independent).

Rows of 65 rows and more run two frames here (train_cases.emu_case); the device stage runs every row at its own T.  Every measured
distance is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to train_forms_cpu_report.txt."""
import pytest

import train_cases as tc
import width_util as wu
from emu_util import emu_lib

note = wu.make_note("train_forms_cpu_report.txt")
ids = lambda cases: [c.id for c in cases]
EMU = [tc.emu_case(c) for c in tc.FORM_CASES if tc.emu_case(c) is not None]
GROUPS = tc.tiling_groups(EMU)
PREFIX = [(tc.emu_case(a), tc.emu_case(b)) for a, b in tc.PREFIX]


@pytest.fixture(scope="module")
def lib():
    """A context of its own on the emulator library: options and the status sink set here never reach other tests."""
    ctx = emu_lib().new_context()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def runner(lib):
    return tc.Runner(wu.NpMem(lib), note)


def test_the_table_reaches_every_form_and_tile_class():
    """What the header of train_cases.py promises, of the rows this stage runs and of the device-only rows."""
    for cases, fwd_tiles in ((EMU, {tc.F_X3H: {1, 2, 6, 10}, tc.F_X3: {1, 2, 3, 4}, tc.F_W3: {1, 2, 3, 6}, tc.F_PAIR: {1, 6}, tc.F_FP32: {1, 6}}),
                             (tc.H1024_CASES, {tc.F_X3H: {1, 3}, tc.F_X3: {1, 2, 4}, tc.F_W3: {1, 2, 3, 6}, tc.F_PAIR: {1, 3}, tc.F_FP32: {1, 3}})):
        assert {c.plan[1] for c in cases} == set(range(7)) and {c.plan[4] for c in cases} == set(range(5))
        for form, tiles in fwd_tiles.items():
            assert {c.plan[3] for c in cases if c.plan[1] == form} == tiles, (form, tiles)
        for form in (tc.B_W3, tc.B_X3):
            assert {c.plan[7] for c in cases if c.plan[4] == form and c.plan[6] == 0} >= {2}
            # several launches; a last launch with fewer tiles than block rows (ntile == 0 on the rest)
            multi = [c for c in cases if c.plan[4] == form and c.plan[6] > 0]
            idle = any(0 < (c.plan[0] // 16) % c.plan[6] < c.plan[5] for c in multi)
            assert multi and (idle or (cases is not EMU and form == tc.B_X3)), form      # (H = 1024, X3: two block rows, 4 + 2 tiles)
    assert {c.plan[7] for c in EMU if c.plan[4] == tc.B_PAIR} == {1, 6}
    for form in range(6):       # one carry case per forward form
        assert any(c.carry for c in EMU if c.plan[1] == form), form
    assert any(c.kind == "dec" for c in EMU)
    assert len(GROUPS) >= 8 and {k[1] for k in GROUPS} == set(tc.EXACT_FWD) and {k[2] for k in GROUPS} == set(tc.EXACT_BWD)


@pytest.mark.parametrize("c", tc.FORM_CASES, ids=ids(tc.FORM_CASES))
def test_plan_of_every_row(lib, options, c):
    """The whole plan of every row of the table, H = 1024 and the device's frame counts included."""
    tc.set_options(lib, c, options)
    tc.assert_plan(lib, c)
    e = tc.emu_case(c)
    if e is not None and e != c:
        tc.assert_plan(lib, e)


@pytest.mark.parametrize("c", EMU, ids=ids(EMU))
def test_train_pass_in_form(runner, options, c):
    """Plan, then forward + backward of one train-mode pass with injected masks: outputs, carried state, dx and the ten gradients."""
    runner.check(c, options, tc.EMU_TRAIN_OUT, tc.EMU_TRAIN_GRAD)


@pytest.mark.parametrize("key", list(GROUPS), ids=["h%d-r%d-%s+%s" % (k[0][0], k[0][1], tc.FWD_NAMES[k[1]], tc.BWD_NAMES[k[2]]) for k in GROUPS])
def test_same_form_other_tiling_gives_identical_bits(runner, options, key):
    tc.run_tiling_group(runner, GROUPS[key], options)


@pytest.mark.parametrize("big,small", PREFIX, ids=[b.id for _, b in PREFIX])
def test_rows_of_a_larger_pass_equal_a_pass_of_their_own(runner, options, big, small):
    tc.run_prefix(runner, big, small, options, tc.EMU_TRAIN_OUT, tc.EMU_TRAIN_GRAD)


PROBE = [tc.emu_case(c) for c in tc.PROBE_CASES + tc.PROBE_CONTROLS if tc.emu_case(c) is not None]


@pytest.mark.parametrize("c", PROBE, ids=ids(PROBE))
def test_planned_forward_ran_and_not_its_per_step_fallback(runner, options, c):
    """The fp16-pair and fp32-MFMA forwards fall back to per-step launches at run time when their launch fails, within every bound
    here: with train_prof the persistent kernel leaves its counters in the scratch, the per-step launches (control rows) do not."""
    tc.run_fallback_probe(runner, c, options)
