"""TEST INFRASTRUCTURE of the stacked-GRU tile tests: ONE case table (eval passes of networks with hidden_layers >= 2 at every layer
count and every row-tile class the two recurrences of csrc/cvae_deep.h treat differently) and the drivers that run a case on the
host-fiber emulator (tests/test_stacked_tiles_cpu.py) or on the device (tests/test_stacked_tiles_gpu.py).

Everything a pass is held to is tests/width_util.py's, unchanged: EvalNet / run_eval_case (whole pass at T = 3, two windows with the
library's own carried (y_last, h [L,B,H]), h_in with an off-manifold y_in, T = 1), every buffer a view of exactly its queried byte
count inside a NaN-filled arena, guards, cvae_workspace_status == 0, fully written finite outputs, float64 references
(width_ref.eval_reference = frontend_ref.forward).  What a case adds: the layer count, the library option max_rt (a cap on the row-tile
sets in flight, which puts several 32-row tiles into one block at small batches), and the WHOLE plan {path, Bp, rts, tiles} asserted
with cvae_plan_pass_deep_tiles before the pass, so that a case cannot quietly run another tiling than the one it is in the table for.

T = 3 for the whole pass: frame 0 reads every tile's state from memory, frame 1 from the registers hk0 .. hk3 of k_gru_steps_deep3,
frame 2 from a register value that was itself carried.

What the rows reach (cu_count() is 256 on the MI355X and on the emulator: rts = min(256 / (L * H/8), Bp/32, max_rt or unlimited)):
  k_gru_steps_deep3  blocks (layer, octet, tile set ti of rts); block ti takes tiles ti, ti + rts, .. : ntile = ceil((nrt - ti) / rts)
                     tasks per frame, carried states hk0 .. hk3 selected by the task's index; prefetch_next's tile index wraps at
                     ntile; tile_own / tile_u slots; per-(layer, tile, octet) flags.  1, 2, 3, 4 tiles per block with a full, a partly
                     dead and a one-row last tile; uneven counts between blocks (2/1/1, 3/2, 2/1); rts 2, 3, 5 polling at once;
                     L = 3, 4, 5, 8: layer strides of hb / hx / w3, gbias[l - 1], layer 0 reading the top layer (lay_u / fl_u wrap)
  plan_deep_pass     the four-tile cap: five tiles on one block must plan the any-H kernel (H = 64 at 129 rows with max_rt 1, H = 1024
                     at 129 rows by itself)
  k_gru_steps_deep   rt0 trips of four 16-row tiles: one trip of two (Bp 32), a second of two (Bp 96), three with a last of two
                     (Bp 160); L = 3, 4, 8; the uneven K split over four waves at H = 48 and 144 above two layers
  device only        H = 1024: three and four tiles per block on the KPW = 16 instance with its RD = 8 operand ring; the any-H kernel at
                     three layers (256 resident blocks, L*T sub-steps behind the grid barrier); H = 2048: 512 blocks per launch
"""
import collections

import numpy as np

import _cabi
import gemm_util as gu
import width_util as wu
from stacked_util import EMU_PASS, PERSISTENT, TIGHT_KERNELS, TIGHT_PASS      # noqa: F401  (the project's own bounds, unchanged)
from stacked_util import GENERIC as GENERIC_FLAGS

RESIDENT, ANY_H, PER_STEP = _cabi.DEEP_RESIDENT, _cabi.DEEP_GENERIC, _cabi.DEEP_PER_STEP
PATH_NAMES = {RESIDENT: "RESIDENT", ANY_H: "GENERIC", PER_STEP: "PER_STEP"}
CUS = 256


class StackCase(collections.namedtuple("StackCase", "H rows T in_dim lat form flags layers twin max_rt rts tiles")):
    """EvalCase's fields (width_util.run_eval_case reads them) + max_rt: the library option of the case (0 = default) + what
    cvae_plan_pass_deep_tiles must report with it: form = path, rts, tiles = the most row tiles one block handles per frame."""
    __slots__ = ()

    @property
    def Bp(self):
        return gu.up(self.rows, 32)

    @property
    def plan(self):
        return [self.form, self.Bp, self.rts, self.tiles]

    @property
    def id(self):
        return "h%d-L%d-r%d-%s%s%s%s" % (self.H, self.layers, self.rows, PATH_NAMES[self.form], "-rt%d" % self.max_rt if self.max_rt else "",
                                       "-forced" if self.flags & _cabi.FLAG_GENERIC_STEP else "", "" if self.flags else "-flags0")

    @property
    def tag(self):      # the problem of a case does not depend on how it is tiled: cases that differ in max_rt / flags share inputs
        return "stack/e/%d/%d/%d" % (self.H, self.rows, self.layers)

    @property
    def problem(self):
        """What the float64 reference depends on (the key of the modules' reference caches)."""
        return (self.H, self.rows, self.T, self.in_dim, self.lat, self.layers)


def _case(L, rows, form, rts=1, tiles=None, max_rt=0, flags=PERSISTENT, H=64, T=3, twin=False):
    if tiles is None:
        assert form != RESIDENT
        tiles = gu.up(rows, 32) // 16       # the any-H kernel: every block walks all 16-row tiles
    return StackCase(H, rows, T, wu._in_dim(H), 4, form, flags, L, twin, max_rt, rts, tiles)


def _table():
    t = [_case(2, rows, RESIDENT, 1, 1) for rows in (1, 31, 32)]       # one tile with 31 dead rows, one dead row, none
    t += [_case(2, 33, RESIDENT, 2, 1),                                # ti = 1 with one live row
          _case(2, 33, RESIDENT, 1, 2, max_rt=1),                      # hk0, hk1
          _case(2, 65, RESIDENT, 1, 3, max_rt=1),                      # hk2; last tile with one live row
          _case(2, 97, RESIDENT, 1, 4, max_rt=1),                      # hk3; partly dead last tile
          _case(2, 128, RESIDENT, 1, 4, max_rt=1),                     # hk3; full last tile
          _case(2, 97, RESIDENT, 3, 2, max_rt=3),                      # 2 / 1 / 1 tiles: ntile differs between the tile sets
          _case(2, 160, RESIDENT, 2, 3, max_rt=2),                     # 3 / 2 tiles: uneven, prefetch_next wraps at 3 and at 2
          _case(2, 160, RESIDENT, 5, 1),                               # five tile sets polling at once
          _case(2, 129, ANY_H, max_rt=1),                              # five tiles exceed the cap; Bp 160: three rt0 trips, the last of two
          _case(3, 65, RESIDENT, 2, 2, max_rt=2),                      # 2 / 1 tiles with a middle layer
          _case(4, 3, RESIDENT, 1, 1), _case(5, 3, RESIDENT, 1, 1), _case(8, 3, RESIDENT, 1, 1),      # layer strides, lay_u wrap, gbias[l-1]
          _case(8, 40, RESIDENT, 1, 2, max_rt=1)]                      # the deepest net with two tiles per block
    for L in (2, 8):
        t += [_case(L, 3, ANY_H, flags=GENERIC_FLAGS),                 # one trip of two tiles
              _case(L, 70, ANY_H, flags=GENERIC_FLAGS, twin=True),     # Bp 96: a second trip of two; + the per-step launches, bit for bit
              _case(L, 70, PER_STEP, flags=0)]
    t += [_case(3, 17, ANY_H, H=48), _case(4, 17, ANY_H, H=144)]       # the uneven K split over four waves above two layers
    # each of these is milliseconds on the device and minutes on the emulator
    t += [_case(2, 96, RESIDENT, 1, 3, H=1024), _case(2, 128, RESIDENT, 1, 4, H=1024),      # KPW = 16, RD = 8 ring at three and four tiles
          _case(2, 129, ANY_H, H=1024),                                # the cap at rts = 1 without any option
          _case(3, 5, ANY_H, H=1024),                                  # 3 * 128 blocks are not resident: 256 blocks behind the grid barrier
          _case(2, 2, PER_STEP, H=2048, T=2)]                          # 512 blocks per launch
    return t


STACK_CASES = _table()

# the resident kernel's arithmetic per row does not depend on which block does it: every tiling of these row counts that max_rt
# 0 .. 3 plans on the resident kernel, as {max_rt: (rts, tiles)}
TILINGS = {33: {0: (2, 1), 1: (1, 2)}, 97: {0: (4, 1), 1: (1, 4), 2: (2, 2), 3: (3, 2)}, 160: {0: (5, 1), 2: (2, 3), 3: (3, 2)}}
# rows of the 97-row batch at the edges of its four tiles, and the last one alone
EDGE_ROWS = [0, 31, 32, 64, 96]
# resident against the any-H kernel on the same operands (device bound TIGHT_KERNELS): most tiles, most tile sets, most layers
VERSUS_CASES = [c for c in STACK_CASES if c.form == RESIDENT and (c.H, c.layers, c.rows, c.max_rt) in
                ((64, 2, 97, 1), (64, 2, 160, 0), (64, 2, 160, 2), (64, 3, 65, 2), (64, 8, 40, 1), (1024, 2, 128, 0))]


def expected_rts(c):
    """The rule of plan_deep_pass restated: rts and the resident condition of a case."""
    per_tile, nrt = c.layers * c.H // 8, c.Bp // 32
    rts = max(1, min(CUS // per_tile, nrt))
    if c.max_rt >= 1:
        rts = min(rts, c.max_rt)
    return rts, -(-nrt // rts)


# Rows that run on the device only, with the row of the emulator stage that runs the same class (case id -> reason).  The times are
# one emulator process on the machine profiles/stacked_tiles_notes.md was written on.
EMU_MOVED = {
    "h64-L2-r128-RESIDENT-rt1": "four tiles per block run here at 97 rows, a full last tile at 32",
    "h64-L2-r160-RESIDENT-rt2": "uneven tile counts run here at 97 rows with max_rt 3 (2 / 1 / 1), three tiles per block at 65 rows",
    "h64-L2-r160-RESIDENT": "80 resident blocks: the slowest row; rts > 1 runs here at 33 rows (2) and at 97 rows (3)",
    "h64-L3-r65-RESIDENT-rt2": "uneven counts run here at L = 2, a middle layer at L = 8",
    "h64-L4-r3-RESIDENT": "L = 8 at 3 rows runs here: the same strides and the same wrap with more layers",
    "h64-L5-r3-RESIDENT": "L = 8 at 3 rows runs here: the same strides and the same wrap with more layers",
    "h64-L8-r40-RESIDENT-rt1": "L = 8 runs here at 3 rows, two tiles per block at L = 2 with 33 rows",
    "h64-L8-r70-GENERIC-forced": "the second rt0 trip runs here at L = 2, the any-H kernel at L = 8 with 3 rows",
    "h64-L8-r70-PER_STEP-flags0": "the per-step launches run here at L = 2 as the twin of the 70-row GENERIC row",
    "h64-L2-r70-PER_STEP-flags0": "its whole pass runs here as the twin of the 70-row GENERIC row, bit for bit",
}
EMU_TILING_ROWS = [33]      # the tilings of 97 and 160 rows (four and three passes of 64 - 80 resident blocks) run on the device


def emu_case(c):
    """The case as the emulator stage runs it, or None where it runs on the device only.  The emulator runs every thread of every
    block as a fiber; a pass of a resident kernel costs seconds, growing with blocks x tasks.  Rules:
      * H > 144: the H = 1024 / 2048 rows are minutes per pass here (as width_util.EMU_MAX_H says of one-layer passes);
      * the rows of EMU_MOVED, each for the reason given there;
    and what stays covers every tile class at least once -- 1, 2, 3 and 4 tiles per block, uneven counts, rts > 1, the cap, L = 8, a
    second rt0 trip -- which tests/test_stacked_tiles_cpu.py asserts.  No row is shortened."""
    return None if c.H > 144 or c.id in EMU_MOVED else c


# ---------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------
def make_refs():
    """problem -> float64 reference, computed once per problem and module (cases that differ in tiling only share it)."""
    cache = {}

    def get(c):
        if c.problem not in cache:
            cache[c.problem] = wu.eval_reference(c)
        return cache[c.problem]
    return get


def set_max_rt(lib, c, options):
    """The case's max_rt through the `options` fixture, which resets the library's options after the test, failure included."""
    if c.max_rt:
        options(max_rt=c.max_rt)
    assert lib.get_option("max_rt") == c.max_rt, "a max_rt left over from another test"


def assert_plan(lib, d, c, frames):
    """Holds the library's plan to the table's {path, Bp, rts, tiles}, at every frame count the case runs."""
    for T in frames:
        got = lib.plan_pass_deep_tiles(d, c.layers, c.rows, T, c.flags)
        assert got == c.plan, "%s at T = %d: planned {path, Bp, rts, tiles} = %s, the table says %s" % (c.id, T, got, c.plan)


def run_stack_case(mem, c, ref, note, bound, options):
    """One row of the table: the plan, then the four stages of width_util.run_eval_case (which asserts the path again before the
    whole pass, and at a `twin` row the per-step launches bit for bit)."""
    lib = mem.lib
    set_max_rt(lib, c, options)
    d = lib.desc(c.in_dim, 2 * c.lat, c.H, 3, 2, True, False)
    assert_plan(lib, d, c, sorted({c.T, (c.T + 1) // 2, c.T - (c.T + 1) // 2, 1}))      # the whole pass, both windows, one frame
    note("%-9s plan  %-34s path %-8s Bp %3d rts %d tiles %d" % (mem.name, c.id, PATH_NAMES[c.form], c.Bp, c.rts, c.tiles))
    return wu.run_eval_case(mem, c, ref, note, bound)


def _whole(net, c, P, rows=None, flags=None, what=""):
    x, y = (P.x, P.y_in_enc) if rows is None else (P.x[rows], P.y_in_enc[rows])
    return net.forward(x, y, clamp_lat_dim=c.lat, flags=c.flags if flags is None else flags, what="%s %s" % (c.id, what))


def _same_bits(a, b, what):
    for name, u, v in zip(("trj_out", "y_last", "h_last"), a, b):
        assert u.shape == v.shape and u.tobytes() == v.tobytes(), "%s: %s differs (max|d| %.3e)" % (what, name, float(np.max(np.abs(u - v))))


def h64_case(rows, L=2):
    return _case(L, rows, RESIDENT, 0, 0)


def run_tilings(mem, rows, ref, note, bound, options):
    """The whole pass of `rows` rows at H = 64, L = 2 under every tiling of TILINGS[rows]: identical bits of trj_out, y_last and
    h_last, and the first one within `bound` of the reference."""
    c = h64_case(rows)
    P = wu.eval_problem(c)
    net = wu.EvalNet(mem, P.enc, c.in_dim, 2 * c.lat, c.H, c.layers)
    first = None
    for max_rt, (rts, tiles) in sorted(TILINGS[rows].items()):
        options(max_rt=max_rt)
        got = mem.lib.plan_pass_deep_tiles(net.d, c.layers, rows, c.T, c.flags)
        assert got == [RESIDENT, c.Bp, rts, tiles], (rows, max_rt, got)
        out = _whole(net, c, P, what="max_rt %d" % max_rt)
        if first is None:
            first = out
            d = wu.maxdiff(out, ref["whole"])
            note("%-9s tiling %d rows: max|d| = %.3e to the reference" % (mem.name, rows, d))
            assert d <= bound, (rows, d, bound)
        else:
            _same_bits(first, out, "%d rows, max_rt %d against max_rt %d" % (rows, max_rt, min(TILINGS[rows])))
    note("%-9s tiling %d rows: identical bits at (rts, tiles) = %s" % (mem.name, rows, sorted(TILINGS[rows].values())))


def run_row_independence(mem, note):
    """Rows at the tile edges of the 97-row batch (H = 64, L = 2, resident, four tile sets) run as a 5-row batch, and row 96 alone,
    equal the same rows of the full batch bit for bit: same kernel, per-row arithmetic."""
    c = h64_case(97)
    P = wu.eval_problem(c)
    net = wu.EvalNet(mem, P.enc, c.in_dim, 2 * c.lat, c.H, c.layers)
    lib = mem.lib
    assert lib.get_option("max_rt") == 0
    assert lib.plan_pass_deep_tiles(net.d, 2, 97, c.T, c.flags) == [RESIDENT, 128, 4, 1]
    assert lib.plan_pass_deep_tiles(net.d, 2, len(EDGE_ROWS), c.T, c.flags) == [RESIDENT, 32, 1, 1]
    full = _whole(net, c, P, what="97 rows")
    for rows in (EDGE_ROWS, [96]):
        sub = _whole(net, c, P, rows=rows, what="rows %s" % rows)
        _same_bits((full[0][rows], full[1][rows], full[2][:, rows]), sub, "rows %s of the 97-row batch against the sub-batch" % rows)
    note("%-9s rows %s and [96] of the 97-row batch: identical bits in a batch of their own" % (mem.name, EDGE_ROWS))


def run_versus(mem, c, note, bound, options):
    """The resident exact-operand kernel against the any-H kernel (CVAE_FLAG_GENERIC_STEP) on the same operands."""
    P = wu.eval_problem(c)
    net = wu.EvalNet(mem, P.enc, c.in_dim, 2 * c.lat, c.H, c.layers)
    set_max_rt(mem.lib, c, options)
    assert_plan(mem.lib, net.d, c, [c.T])
    assert mem.lib.plan_pass_deep_tiles(net.d, c.layers, c.rows, c.T, GENERIC_FLAGS) == [ANY_H, c.Bp, 1, c.Bp // 16]
    res = _whole(net, c, P, what="resident")
    gen = _whole(net, c, P, flags=GENERIC_FLAGS, what="forced any-H")
    d = wu.maxdiff(res, [g.astype(np.float64) for g in gen])
    note("%-9s %-34s resident against any-H: max|d| = %.3e" % (mem.name, c.id, d))
    assert d <= bound, (c.id, d, bound)
