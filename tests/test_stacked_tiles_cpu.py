"""Emulator stage of the stacked-GRU tile tests: the rows of the case table of tests/stacked_cases.py up to H = 144, on the host-fiber
build of the real library (tests/emu), against the float64 references of tests/width_ref.py.

Networks with hidden_layers >= 2 run k_gru_steps_deep3 (resident, exact operands) or k_gru_steps_deep (any H); both have code that
depends on the layer count and on how many row tiles a block owns -- carried states hk0 .. hk3, ntile and the wrap of prefetch_next,
tile sets in flight, the four-tile cap of plan_deep_pass, the rt0 trips of the any-H kernel -- which the other stacked tests
(3, 4 and 64 rows at two and three layers) never reach.  stacked_cases' header lists what each row reaches.

Bound: the emulator bound the project already uses, unchanged: EMU_PASS = 5e-5 per pass (tests/stacked_util.py).  Every row asserts
the library's whole plan {path, Bp, rts, tiles} (cvae_plan_pass_deep_tiles) before it runs.  The plan itself needs no run: it is
asserted here for EVERY row, the device-only ones included.  stacked_cases.emu_case names the rows that run on the device only.
Every measured distance is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to
stacked_tiles_cpu_report.txt; profiles/stacked_tiles_notes.md keeps them."""
import pytest

import _cabi
import stacked_cases as sc
import width_util as wu
from emu_util import emu_lib

note = wu.make_note("stacked_tiles_cpu_report.txt")
EMU = [sc.emu_case(c) for c in sc.STACK_CASES if sc.emu_case(c) is not None]
ids = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def lib():
    """A context of its own on the emulator library: the max_rt set here never reaches other tests."""
    ctx = emu_lib().new_context()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def mem(lib):
    return wu.NpMem(lib)


@pytest.fixture(scope="module")
def refs():
    return sc.make_refs()


def test_table_and_library_agree_on_every_plan(lib, options):
    """Every row (device-only ones too): the table's {rts, tiles} is what the rule rts = min(256 / (L * H/8), Bp/32, max_rt) gives,
    resident exactly while a block owns at most four tiles, and cvae_plan_pass_deep_tiles reports the row's whole plan."""
    assert len({c.id for c in sc.STACK_CASES}) == len(sc.STACK_CASES)
    for c in sc.STACK_CASES:
        rts, tiles = sc.expected_rts(c)
        fits = c.H in (64, 1024) and c.layers * c.H // 8 <= sc.CUS and tiles <= 4
        if c.flags == sc.PERSISTENT:
            assert (c.form == sc.RESIDENT) == fits, c.id
        if c.form == sc.RESIDENT:
            assert (c.rts, c.tiles) == (rts, tiles), c.id
        else:
            assert (c.rts, c.tiles) == (1, c.Bp // 16), c.id
        lib.reset_options()
        sc.set_max_rt(lib, c, options)
        sc.assert_plan(lib, lib.desc(c.in_dim, 2 * c.lat, c.H, 3, 2, True, False), c, [c.T, 1])
        assert lib.plan_pass_deep(lib.desc(c.in_dim, 2 * c.lat, c.H, 3, 2, True, False), c.layers, c.rows, c.T, c.flags) == c.form
    lib.reset_options()
    for rows, tilings in sc.TILINGS.items():      # every resident tiling max_rt 0 .. 3 gives at these row counts, and no other
        c = sc.h64_case(rows)
        want = {}
        for max_rt in range(4):
            rts, tiles = sc.expected_rts(c._replace(max_rt=max_rt))
            if tiles <= 4 and (rts, tiles) not in want.values():
                want[max_rt] = (rts, tiles)
        assert want == tilings, rows
    with pytest.raises(_cabi.CvaeError):
        lib.plan_pass_deep_tiles(lib.desc(6, 8, 64, 3, 2, True, False), 1, 3, 3, sc.PERSISTENT)      # one layer: refused, as the path query


def test_the_emulator_stage_runs_every_tile_class():
    """1, 2, 3 and 4 tiles per block, uneven counts, rts > 1, the cap, L = 8 (on either kernel), a second rt0 trip, every layer count
    and every width up to 144 of the table."""
    res = [c for c in EMU if c.form == sc.RESIDENT]
    assert {c.tiles for c in res} == {1, 2, 3, 4}
    assert any(c.rts > 1 and (c.Bp // 32) % c.rts for c in res), "uneven tile counts between the blocks"
    assert {c.rts for c in res} >= {1, 2, 3}
    assert any(c.form == sc.ANY_H and c.flags == sc.PERSISTENT and c.H == 64 for c in EMU), "the four-tile cap"
    assert {c.form for c in EMU if c.layers == 8} == {sc.RESIDENT, sc.ANY_H}
    assert any(c.form == sc.ANY_H and c.tiles > 4 and c.twin for c in EMU), "a second rt0 trip, with the per-step launches as twin"
    assert {c.layers for c in EMU} >= {2, 3, 4, 8}
    assert set(sc.EMU_MOVED) <= {c.id for c in sc.STACK_CASES}
    assert {c.H for c in EMU} == {c.H for c in sc.STACK_CASES if c.H <= 144} == {48, 64, 144}
    assert all(c.T >= 2 for c in EMU)      # (a row moved down may lose a frame, never the carried-state window)


@pytest.mark.parametrize("c", EMU, ids=ids(EMU))
def test_stacked_pass_at_tiling(mem, refs, options, c):
    """The row's plan, then: whole pass, two windows with the carried (y_last, h [L,B,H]), h_in with an off-manifold y_in, T = 1; at
    the `twin` rows also the per-step launches, bit for bit."""
    sc.run_stack_case(mem, c, refs(c), note, sc.EMU_PASS, options)


@pytest.mark.parametrize("rows", sc.EMU_TILING_ROWS)
def test_resident_bits_do_not_depend_on_the_tiling(mem, refs, options, rows):
    sc.run_tilings(mem, rows, refs(sc.h64_case(rows)), note, sc.EMU_PASS, options)


def test_rows_at_tile_edges_are_independent_of_the_batch(mem):
    sc.run_row_independence(mem, note)
