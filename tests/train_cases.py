"""TEST INFRASTRUCTURE of the training-form tests: ONE case table (train-mode passes at H = 64 and H = 1024 in every recurrence form
plan_train_pass of csrc/cvae_train.inc chooses, at every row-tile class the forms treat differently) and the drivers that run a case
on the host-fiber emulator (tests/test_train_forms_cpu.py) or on the device (tests/test_train_forms_gpu.py).

Everything a pass is held to is tests/width_util.py's, unchanged: TrainNet.run (every buffer -- train image, tape, scratch, inputs,
outputs, gradients -- a view of exactly its queried byte count inside a NaN-filled arena: the library is handed NO zeroed memory, so
a dead row that the memset decisions fwd_full_writes / bwd_writes_gates leave unwritten reaches a GEMM as NaN), guards, the status
sink, fully written finite outputs, float64 references (width_ref.train_reference), inputs and masks of width_util.train_problem.
T = 3 (first, a middle, the last step); T = 4 at the word-exchange rows (both exchange slots written twice), T = 1 where stated.
What a case adds: its library options and the WHOLE plan asserted with cvae_plan_train_pass before the pass, so that a case cannot
quietly run another form or tiling than the one it is in the table for.  The table holds {Bp, fwd, fwd_rts, fwd_tiles, bwd, bwd_rts,
bwd_per_launch, bwd_tiles}; the remaining four fields of the query follow from those and the options (expected_rest) and are
asserted as well.

The rule, for deriving a row (cu_count() is 256 on the MI355X and on the emulator; fit(u, n) = min(256 / (H/u), n, max_rt or inf)):
  Bp        B for <= 3 rows on the word-exchange kernels (ll_row_pad overrides), 16 for <= 16 rows (x3_tile 32: 32), else up(B, 32)
  forward   LL <= 3 rows | W3 (16-unit blocks) from nt16 = Bp/16 >= 4 with x3_tile 0, rts fit(16, nt16) | X3 (8-unit blocks, 32-row
            tiles) when x3_tile = 32, or when a block would own >= 2 of them; at most 4 per block | X3H (16-row tiles), rts
            fit(8, nt16) | PAIR with train_kernel 1, FP32 with train_fp32_mfma 1 | STEPS with train_per_step 1 or T = 1
  reverse   LL <= 3 rows | W3 from nt16 >= 4, rts min(fit(16, nt16), nt16 / 2) | X3, rts fit(8, nt16) | PAIR | STEPS with
            train_bwd_per_step 1 or T = 1; W3 and X3 give a block at most two tiles per launch: bwd_per_launch = 2 * rts tiles when
            the pass has more
H = 64 has 8 (4) blocks per row tile, so every tile gets a block row of its own and max_rt is the knob for several tiles per block;
H = 1024 has 128 (64), i.e. 2 block rows of 8-unit blocks and 4 of 16-unit blocks.

What the rows reach:
  tiles per block    k_train_fwd_steps_x3h / _w3 / _h / k_train_fwd_steps keep the state of ntile == 1 in a register, of ntile == 2 in
                     a second one (keep1), and re-read hrow from ntile > 2 on; k_train_bwd_steps_x3 / _w3 carry dhz likewise (k1)
                     within a launch: 1, 2, 3, 6 tiles per block forward; 1 and 2 per launch in reverse; 6 in the pair reverse
  uneven counts      3/3/2 (H = 64, 97 rows, max_rt 3), 2/2/1/1 and 3/3/2/2 (H = 1024, 65 and 129 rows), 2/1 and 4/3 32-row tiles
  launches           4 + 2, 6 + 2 (the last with an idle block row: tile_n < rts), 2 + 2 + 2, 8 + 2 (two idle block rows), 4 + 4 + 2
  dead rows          13 of 16 (3 rows on the tile forms), 15 of 16 (17 rows), a wholly dead tile (33 rows: Bp 64, rows 48..63)
  word exchange      T = 4: both exchange slots of k_train_fwd_steps_ll / k_train_bwd_steps_ll written a second time within a launch
  the cap            five 32-row tiles on one block plan X3H (129 rows, x3_tile 32, max_rt 1)
  mixed directions   the tape of one geometry read by the reverse recurrence of the other
  device only        H = 1024: the instances <8, 4, ..> of the exact forms, k_train_fwd_steps_x3<16>, k_train_bwd_steps_x3<32> over
                     several launches, k_train_fwd_steps<32>
"""
import collections

import numpy as np

import _cabi
import gemm_util as gu
import width_util as wu
from width_util import EMU_TRAIN_GRAD, EMU_TRAIN_OUT      # noqa: F401  (the project's own emulator bounds, unchanged)

F_LL, F_W3, F_X3, F_X3H, F_PAIR, F_FP32, F_STEPS = range(7)
B_LL, B_W3, B_X3, B_PAIR, B_STEPS = range(5)
assert (F_LL, F_W3, F_X3, F_X3H, F_PAIR, F_FP32, F_STEPS) == (_cabi.TRAIN_FWD_LL, _cabi.TRAIN_FWD_W3, _cabi.TRAIN_FWD_X3, _cabi.TRAIN_FWD_X3H,
                                                              _cabi.TRAIN_FWD_PAIR, _cabi.TRAIN_FWD_FP32, _cabi.TRAIN_FWD_STEPS)
assert (B_LL, B_W3, B_X3, B_PAIR, B_STEPS) == (_cabi.TRAIN_BWD_LL, _cabi.TRAIN_BWD_W3, _cabi.TRAIN_BWD_X3, _cabi.TRAIN_BWD_PAIR,
                                               _cabi.TRAIN_BWD_STEPS)
FWD_NAMES = ["LL", "W3", "X3", "X3H", "PAIR", "FP32", "STEPS"]
BWD_NAMES = ["LL", "W3", "X3", "PAIR", "STEPS"]
EXACT_FWD, EXACT_BWD = (F_W3, F_X3, F_X3H), (B_W3, B_X3)
PLAN_KEYS = ("Bp", "fwd", "fwd_rts", "fwd_tiles", "bwd", "bwd_rts", "bwd_per_launch", "bwd_tiles")


class FormCase(collections.namedtuple("FormCase", "H rows T kind carry opts sub_of plan")):
    """width_util.TrainCase's fields (TrainNet and train_problem read them) + sub_of: the case is the first `rows` rows of the
    sub_of-row problem (0: a problem of its own) + plan: what cvae_plan_train_pass must report, as the values of PLAN_KEYS."""
    __slots__ = ()

    @property
    def id(self):
        o = "".join("-%s%d" % kv for kv in self.opts)
        return "h%d-r%d%s-t%d-%s%s-%s+%s%s" % (self.H, self.rows, "of%d" % self.sub_of if self.sub_of else "", self.T, self.kind,
                                                "-carry" if self.carry else "", FWD_NAMES[self.plan[1]], BWD_NAMES[self.plan[4]], o)

    @property
    def problem(self):
        """What inputs, masks and the float64 reference depend on: NOT the options, so every tiling of a shape sees the same problem."""
        return (self.H, self.sub_of or self.rows, self.T, self.kind, self.carry)

    @property
    def tag(self):
        return "forms/t/%d/%d/%d/%s/%d" % self.problem

    @property
    def wtag(self):      # one set of weights per H: the device stage keeps one train image per (H, kind)
        return "forms/w/%d" % self.H

    @property
    def expect(self):
        return dict(zip(PLAN_KEYS, self.plan))


def _case(H, rows, fwd, fwd_rts, fwd_tiles, bwd, bwd_rts, bwd_per_launch, bwd_tiles, Bp=None, T=3, kind="enc", carry=False, sub_of=0, **opts):
    if Bp is None:
        Bp = 16 if rows <= 16 and opts.get("x3_tile") != 32 else gu.up(rows, 32)
    return FormCase(H, rows, T, kind, carry, tuple(sorted(opts.items())), sub_of, (Bp, fwd, fwd_rts, fwd_tiles, bwd, bwd_rts, bwd_per_launch, bwd_tiles))


def _h64():
    c = lambda *a, **k: _case(64, *a, **k)
    t = []
    # ---- word exchange: Bp = B rows per frame (ll_row_pad: 4), no row tiles
    # (T = 4: the exchange slot of step t is (t + 1) & 1, so four frames are the first length at which a slot is written twice in a launch)
    t += [c(B, F_LL, 0, 0, B_LL, 0, 0, 0, Bp=B, T=4) for B in (1, 2, 3)]
    t += [c(2, F_LL, 0, 0, B_LL, 0, 0, 0, Bp=2, T=4, carry=True),
          c(1, F_LL, 0, 0, B_LL, 0, 0, 0, Bp=4, T=4, ll_row_pad=4),
          c(2, F_LL, 0, 0, B_STEPS, 0, 0, 0, T=4, train_bwd_per_step=1),   # LL forward on Bp = 16, per-step reverse
          c(3, F_X3H, 1, 1, B_X3, 1, 0, 1, no_ll=1)]                       # the tile forms with 13 dead rows; bwd_writes_gates = 1
    # ---- 8-unit blocks, 16-row tiles: X3H + X3
    t += [c(4, F_X3H, 1, 1, B_X3, 1, 0, 1), c(16, F_X3H, 1, 1, B_X3, 1, 0, 1),
          c(17, F_X3H, 2, 1, B_X3, 2, 0, 1),                               # second tile with one live row
          c(17, F_X3H, 1, 2, B_X3, 1, 0, 2, max_rt=1),                     # two tiles per block: keep1 / k1
          c(17, F_X3H, 2, 1, B_X3, 2, 0, 1, kind="dec"),
          c(17, F_X3H, 2, 1, B_X3, 2, 0, 1, carry=True),
          c(65, F_X3H, 1, 6, B_W3, 1, 2, 2, x3_tile=16, max_rt=1),         # ntile > 2: hrow re-read; the reverse plans W3: 2 + 2 + 2
          c(33, F_X3H, 4, 1, B_X3, 4, 0, 1, train_fwd_geom=0, train_bwd_geom=0)]      # (the prefix check's X3H + X3 pass of 33 rows)
    # ---- 8-unit blocks, 32-row tiles: X3 (its reverse from four 16-row tiles on is W3)
    t += [c(33, F_X3, 2, 1, B_W3, 2, 0, 2, x3_tile=32),
          c(33, F_X3, 2, 1, B_W3, 2, 0, 2, x3_tile=32, carry=True),
          c(33, F_X3, 1, 2, B_W3, 1, 2, 2, x3_tile=32, max_rt=1),
          c(65, F_X3, 1, 3, B_W3, 1, 2, 2, x3_tile=32, max_rt=1),
          c(97, F_X3, 1, 4, B_W3, 1, 2, 2, x3_tile=32, max_rt=1),          # the cap
          c(129, F_X3H, 1, 10, B_W3, 1, 2, 2, x3_tile=32, max_rt=1)]       # five 32-row tiles on one block: X3H
    # ---- 16-unit blocks: W3 + W3
    t += [c(33, F_W3, 4, 1, B_W3, 2, 0, 2),                                # Bp 64: rows 48..63 are a wholly dead tile
          c(33, F_W3, 4, 1, B_W3, 2, 0, 2, carry=True),
          c(64, F_W3, 4, 1, B_W3, 2, 0, 2),                                # no dead row
          c(65, F_W3, 6, 1, B_W3, 3, 0, 2),
          c(65, F_W3, 2, 3, B_W3, 2, 4, 2, max_rt=2),                      # forward 3/3; reverse launches of 4 + 2
          c(97, F_W3, 8, 1, B_W3, 4, 0, 2),
          c(97, F_W3, 3, 3, B_W3, 3, 6, 2, max_rt=3),                      # forward 3/3/2; reverse 6 + 2: one block row with ntile == 0
          c(33, F_W3, 4, 1, B_W3, 2, 0, 2, bwd_w3_l1_h64=1)]               # the <1, 2, 2> instances, both directions
    # ---- BWD_X3 from four tiles on
    t += [c(33, F_W3, 4, 1, B_X3, 4, 0, 1, train_bwd_geom=0),
          c(33, F_W3, 2, 2, B_X3, 2, 0, 2, train_bwd_geom=0, max_rt=2),    # two per block in one launch
          c(65, F_W3, 1, 6, B_X3, 1, 2, 2, train_bwd_geom=0, max_rt=1),    # 2 + 2 + 2
          c(97, F_W3, 3, 3, B_X3, 3, 6, 2, train_bwd_geom=0, max_rt=3)]    # 6 + 2, an idle block row
    # ---- mixed directions at 65 rows
    t += [c(65, F_X3H, 6, 1, B_W3, 3, 0, 2, train_fwd_geom=0),
          c(65, F_X3, 1, 3, B_W3, 1, 2, 2, train_fwd_geom=0, max_rt=1),    # the 32-row-tile tape read by W3
          c(65, F_W3, 6, 1, B_X3, 6, 0, 1, train_bwd_geom=0)]
    # ---- fp16 pairs
    t += [c(5, F_PAIR, 1, 1, B_PAIR, 1, 0, 1, train_kernel=1),
          c(5, F_PAIR, 1, 1, B_PAIR, 1, 0, 1, train_kernel=1, carry=True),
          c(33, F_PAIR, 4, 1, B_PAIR, 4, 0, 1, train_kernel=1),
          c(65, F_PAIR, 1, 6, B_PAIR, 1, 0, 6, train_kernel=1, max_rt=1)]  # six tiles per block both ways, one launch
    # ---- fp32 MFMA forward (its reverse is the exact one of the shape)
    t += [c(17, F_FP32, 2, 1, B_X3, 2, 0, 1, train_fp32_mfma=1),
          c(17, F_FP32, 2, 1, B_X3, 2, 0, 1, train_fp32_mfma=1, carry=True),
          c(65, F_FP32, 1, 6, B_W3, 1, 2, 2, train_fp32_mfma=1, max_rt=1)]
    # ---- per-step launches
    t += [c(5, F_STEPS, 0, 0, B_X3, 1, 0, 1, train_per_step=1),
          c(5, F_STEPS, 0, 0, B_X3, 1, 0, 1, train_per_step=1, carry=True),
          c(5, F_STEPS, 0, 0, B_STEPS, 0, 0, 0, train_per_step=1, train_bwd_per_step=1),
          c(5, F_STEPS, 0, 0, B_STEPS, 0, 0, 0, T=1),
          c(33, F_STEPS, 0, 0, B_STEPS, 0, 0, 0, T=1)]                     # Bp 64 with one frame
    # ---- the first 16 rows of the 33-row problem as a pass of their own, in the form of the 33-row pass (PREFIX below)
    t += [c(16, F_W3, 1, 1, B_W3, 1, 0, 1, sub_of=33, train_fwd_geom=1, train_bwd_geom=1),
          c(16, F_X3, 1, 1, B_W3, 1, 0, 2, sub_of=33, x3_tile=32, train_bwd_geom=1),
          c(16, F_X3H, 1, 1, B_X3, 1, 0, 1, sub_of=33)]
    return t


def _h1024():
    c = lambda *a, **k: _case(1024, *a, **k)
    t = [c(B, F_LL, 0, 0, B_LL, 0, 0, 0, Bp=B, T=4) for B in (1, 3)]       # (T = 4: both slot parities reused, as at H = 64)
    t += [c(4, F_X3H, 1, 1, B_X3, 1, 0, 1), c(17, F_X3H, 2, 1, B_X3, 2, 0, 1),
          c(33, F_W3, 4, 1, B_W3, 2, 0, 2),                                # one tile per block + a dead tile; reverse 2/2
          c(65, F_W3, 4, 2, B_W3, 3, 0, 2),                                # forward 2/2/1/1
          c(65, F_W3, 1, 6, B_W3, 1, 2, 2, max_rt=1),                      # six tiles on one block row of <8, 4>; reverse 2 + 2 + 2
          c(129, F_W3, 4, 3, B_W3, 4, 8, 2)]                               # forward 3/3/2/2; reverse 8 + 2 with two idle block rows
    t += [c(33, F_X3, 2, 1, B_W3, 2, 0, 2, x3_tile=32),                    # k_train_fwd_steps_x3<16>: 1/1
          c(65, F_X3, 2, 2, B_W3, 3, 0, 2, x3_tile=32),                    # 2/1
          c(200, F_X3, 2, 4, B_W3, 4, 8, 2, x3_tile=32),                   # 4/3; reverse 8 + 6
          c(65, F_X3H, 2, 3, B_W3, 3, 0, 2, x3_tile=16)]                   # 3/3
    t += [c(33, F_W3, 4, 1, B_X3, 2, 0, 2, train_bwd_geom=0),              # k_train_bwd_steps_x3<32> from four tiles on
          c(65, F_W3, 4, 2, B_X3, 2, 4, 2, train_bwd_geom=0),              # 4 + 2
          c(129, F_W3, 4, 3, B_X3, 2, 4, 2, train_bwd_geom=0)]             # 4 + 4 + 2
    t += [c(5, F_PAIR, 1, 1, B_PAIR, 1, 0, 1, train_kernel=1), c(65, F_PAIR, 2, 3, B_PAIR, 2, 0, 3, train_kernel=1),
          c(17, F_FP32, 2, 1, B_X3, 2, 0, 1, train_fp32_mfma=1), c(65, F_FP32, 2, 3, B_W3, 3, 0, 2, train_fp32_mfma=1),
          c(5, F_STEPS, 0, 0, B_X3, 1, 0, 1, train_per_step=1), c(5, F_STEPS, 0, 0, B_STEPS, 0, 0, 0, T=1)]
    return t


H64_CASES, H1024_CASES = _h64(), _h1024()
FORM_CASES = H64_CASES + H1024_CASES
assert len({c.id for c in FORM_CASES}) == len(FORM_CASES)

# the 33-row pass whose rows 0..15 a sub_of case is compared with: same forms in both directions
PREFIX = [(big, small) for small in FORM_CASES if small.sub_of for big in FORM_CASES
          if (big.H, big.rows, big.T, big.kind, big.carry, big.sub_of) == (small.H, small.sub_of, small.T, small.kind, small.carry, 0)
          and (big.plan[1], big.plan[4]) == (small.plan[1], small.plan[4]) and "max_rt" not in dict(big.opts) and "bwd_w3_l1_h64" not in dict(big.opts)]
assert len(PREFIX) == 3, PREFIX


def tiling_groups(cases):
    """Cases that run one problem in the same exact-operand forms under different tilings: {(problem, fwd, bwd): [cases]} with at
    least two members, for the bit comparison (a row's arithmetic does not depend on the block that owns it)."""
    g = collections.OrderedDict()
    for c in cases:
        if c.plan[1] in EXACT_FWD and c.plan[4] in EXACT_BWD and not c.sub_of:
            g.setdefault((c.problem, c.plan[1], c.plan[4]), []).append(c)
    return collections.OrderedDict((k, v) for k, v in g.items() if len(v) >= 2)


def emu_case(c):
    """The case as the emulator stage runs it, or None where only its plan is asserted there: H = 1024 is minutes per pass on the
    emulator; from 65 rows on a case runs two frames, as width_util.emu_case does."""
    if c.H != 64:
        return None
    return c._replace(T=2) if c.rows >= 65 and c.T > 2 else c


def expected_rest(c):
    """The four fields of the query the table does not hold, restated from plan_train_pass: they follow from the forms and options."""
    o, (Bp, fwd, _, _, bwd, _, _, _) = dict(c.opts), c.plan
    per_step, bwd_per_step, fp32, exact = o.get("train_per_step", 0), o.get("train_bwd_per_step", 0), o.get("train_fp32_mfma", 0), not o.get("train_kernel", 0)
    variants = 0
    if not (fwd == F_LL and bwd == B_LL):
        if not per_step and c.T > 1:
            variants |= 4 if fp32 else 3 if exact else 2
        if not bwd_per_step and c.T > 1:
            variants |= 1 if exact else 2
    return {"fwd_col_tiles": 1, "fwd_full_writes": int(c.T > 1 and not per_step and fwd != F_LL),
            "bwd_writes_gates": int(bwd not in (B_LL, B_STEPS) and not (c.rows <= 3 and exact and not o.get("no_ll", 0))), "variants": variants}


# ---------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------
def set_options(lib, c, options):
    """The case's options through the `options` fixture (which resets the library's after the test, failure included).  Before the
    FIRST row a test sets, every option a training pass reads (DEFAULTS and OTHER_DEFAULTS) must be at its default: anything else was
    left over from another test.  Later rows of the same test (the tiling and prefix comparisons) replace the previous row's options,
    so every option of DEFAULTS is set, and read back."""
    if not getattr(options, "forms_rows", 0):
        for name, dflt in list(DEFAULTS.items()) + list(OTHER_DEFAULTS.items()):
            assert lib.get_option(name) == dflt, "%s: option %s = %d left over from another test" % (c.id, name, lib.get_option(name))
    options.forms_rows = getattr(options, "forms_rows", 0) + 1
    want = dict(c.opts)
    assert set(want) <= set(DEFAULTS), c.id
    options(**dict(DEFAULTS, **want))
    for name, dflt in list(DEFAULTS.items()) + list(OTHER_DEFAULTS.items()):
        assert lib.get_option(name) == want.get(name, dflt), "%s: option %s is %d" % (c.id, name, lib.get_option(name))


# the options the table's rows set, with their defaults
DEFAULTS = {"max_rt": 0, "x3_tile": 0, "train_kernel": 0, "train_fp32_mfma": 0, "train_per_step": 0, "train_bwd_per_step": 0, "no_ll": 0,
            "ll_row_pad": 0, "train_fwd_geom": -1, "train_bwd_geom": -1, "bwd_w3_l1_h64": 0, "step_col_tiles": 0, "train_old_gemm": 0}
# what else a training pass reads (back-offs, block map, profiling, the exchange-range threshold, the per-step reverse's K split):
# no row sets them, and none may be left over
OTHER_DEFAULTS = {"ll_backoff": -1, "train_backoff": 32, "train_fwd_backoff": -1, "train_bwd_backoff": -1, "train_xmap": 0, "train_prof": 0,
                  "bwd_overflow_at": 60000, "bwd_ks": 8, "masks_on_side": 1}


def assert_plan(lib, c, note=None, name=""):
    """Holds the library's whole plan to the table's."""
    d = lib.desc(wu._in_dim(c.H) if c.kind == "enc" else 6, 8 if c.kind == "enc" else wu._in_dim(c.H) - 4, c.H, 3, 2, c.kind == "enc", c.kind != "enc")
    got = lib.plan_train_pass(d, c.rows, c.T)
    want = dict(c.expect, **expected_rest(c))
    assert got == want, "%s: planned %s, the table says %s" % (c.id, {k: v for k, v in got.items() if want[k] != v}, {k: v for k, v in want.items() if got[k] != v})
    if note:
        note("%-9s plan  %-58s Bp %3d  fwd %-5s rts %d tiles %2d  bwd %-5s rts %d per launch %d tiles %d" % (
            name, c.id, got["Bp"], FWD_NAMES[got["fwd"]], got["fwd_rts"], got["fwd_tiles"], BWD_NAMES[got["bwd"]], got["bwd_rts"],
            got["bwd_per_launch"], got["bwd_tiles"]))
    return got


class Runner(object):
    """Runs table rows on one backend (width_util.NpMem / TorchMem): options, plan, pass; keeps the train image of every (H, kind),
    the float64 reference of every problem and the result of every row for the comparisons between rows."""

    def __init__(self, mem, note, tape=False):
        self.mem, self.note, self.tape = mem, note, tape      # tape: results keep the pass's tape (tools/train_pass_digests.py)
        self.nets, self.refs, self.results = {}, {}, {}

    def ref(self, c):
        key = c.problem + (c.rows,)
        if key not in self.refs:
            self.refs[key] = wu.train_reference(c)
        return self.refs[key]

    def run(self, c, options):
        """The result of the row (TrainNet.run's dict); runs it once."""
        if c in self.results:
            return self.results[c]
        mem = self.mem
        set_options(mem.lib, c, options)
        assert_plan(mem.lib, c, self.note, mem.name)
        sd, i, o, x, y_in, h_in, cm, gm, cot, clamp = wu.train_problem(c)
        if (c.H, c.kind) not in self.nets:
            # (every MFMA-order image is built whatever the options are: one image serves every form)
            self.nets[(c.H, c.kind)] = wu.TrainNet(mem, sd, i, o, c.H)
        net = self.nets[(c.H, c.kind)]
        self.results[c] = got = net.run(x, y_in, h_in, cm, gm, cot, clamp, what=c.id, tape=self.tape)
        return got

    def check(self, c, options, bound_out, bound_grad):
        got = self.run(c, options)
        return wu.check_train_result(self.mem, c, got, self.ref(c), self.note, bound_out, bound_grad)


# cvae_plan_train_pass reports the plan; FWD_PAIR and FWD_FP32 fall back to the per-step launches at run time when their cooperative
# launch does not fit (or the image lacks their weights), silently and within every bound here.  With the option train_prof block 0 of
# every persistent forward kernel stores four phase cycle sums into the scratch (cvae_train_debug_counters, words 0..3: zeros on the
# emulator, whose clock reads 0); the per-step launches store nothing there, so the words keep the arena's NaN fill (two float32
# NaNs read as one int64).  The rows probed: every row whose forward has such a fall-back; the controls: a per-step forward per H.
PROBE_CASES = [c for c in FORM_CASES if c.plan[1] in (F_PAIR, F_FP32)]
PROBE_CONTROLS = [c for c in FORM_CASES if c.plan[1] == F_STEPS and c.T > 1 and not c.carry and dict(c.opts) == {"train_per_step": 1}]
assert len(PROBE_CASES) == 11 and len(PROBE_CONTROLS) == 2


def run_fallback_probe(runner, c, options):
    """The row once more with train_prof = 1: the planned persistent forward stored its counters (a control row: nothing did)."""
    mem = runner.mem
    set_options(mem.lib, c, options)
    options(train_prof=1)
    assert_plan(mem.lib, c)
    sd, i, o, x, y_in, h_in, cm, gm, cot, clamp = wu.train_problem(c)
    if (c.H, c.kind) not in runner.nets:
        runner.nets[(c.H, c.kind)] = wu.TrainNet(mem, sd, i, o, c.H)
    got = runner.nets[(c.H, c.kind)].run(x, y_in, h_in, cm, gm, cot, clamp, what=c.id + " train_prof", counters=True)
    words = got["counters"][:4]
    written = all(0 <= w < 2 ** 48 for w in words)
    runner.note("%-9s probe %-58s forward counters %s" % (mem.name, c.id, words))
    if c.plan[1] == F_STEPS:
        assert not any(0 <= w < 2 ** 48 for w in words), "%s: the per-step forward stored counters %s: the probe cannot tell the forms apart" % (c.id, words)
    else:
        assert written, "%s: no counters of the planned %s forward (%s): it fell back to the per-step launches" % (c.id, FWD_NAMES[c.plan[1]], words)
    if c in runner.results:      # profiling changes no value
        same_bits(runner.results[c], got, c.id + " with train_prof")


def same_bits(a, b, what, keys=("out", "y_last", "h_last", "dx")):
    for k in keys:
        u, v = a[k], b[k]
        assert u.shape == v.shape and u.tobytes() == v.tobytes(), "%s: %s differs (max|d| %.3e)" % (what, k, float(np.max(np.abs(u - v))))


def run_tiling_group(runner, cases, options):
    """One problem in the same exact-operand forms under every tiling of the table: identical bits of out, y_last, h_last and dx."""
    first = runner.run(cases[0], options)
    for c in cases[1:]:
        same_bits(first, runner.run(c, options), "%s against %s" % (c.id, cases[0].id))
    runner.note("%-9s tiling %s: identical bits under %d tilings" % (runner.mem.name, cases[0].id, len(cases)))


def run_prefix(runner, big, small, options, bound_out, bound_grad):
    """Rows 0..15 of the 33-row pass against the same rows as a 16-row pass of the same forms: rows are independent."""
    a, b = runner.run(big, options), runner.run(small, options)
    n = small.rows
    d = {k: wu.rel_err(a[k][:n], b[k].astype(np.float64)) for k in ("out", "h_last", "dx")}
    runner.note("%-9s prefix %s rows 0..%d against %s: %s" % (runner.mem.name, big.id, n - 1, small.id, ", ".join("%s %.3e" % kv for kv in d.items())))
    assert d["out"] <= bound_out and d["h_last"] <= bound_out and d["dx"] <= bound_grad, (big.id, small.id, d)
