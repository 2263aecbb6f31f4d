"""TEST INFRASTRUCTURE of the hidden-width tests: ONE case table (eval and train passes at every class of hidden width the kernels
treat differently) and the drivers that run a case on the host-fiber emulator (tests/test_width_cpu.py, numpy memory) or on the
device (tests/test_width_gpu.py, torch memory) through one backend.

Memory.  Every buffer the library is handed -- prepared image and prepare scratch, pass workspace, train image, tape, scratch,
every input and every output -- is a view of EXACTLY the byte count the library's own size query returns (inputs and outputs: their
shapes), inside one larger NaN-filled arena (gemm_util.NumpyArena and its torch twin, with views placed 256 bytes apart at least
and 256-byte aligned, as an allocator would).  A read past a view therefore gives NaN -- a wrong result, caught by the comparison --
and a write past it is seen in the guard floats; neither can fault, the arena is one allocation.  Work areas keep the arena's NaN
fill: the library must not count on zeroed memory (the modules hand it torch.empty).  After every pass the drivers assert: guards
intact (the pass's arena and the image's), every output element written and finite, status words zero -- eval passes run WITHOUT a
status sink and are read back with cvae_workspace_status; train passes have no such query, so they run WITH a sink (int32[4] the
host reads) that must stay zero.

Forms.  The expected recurrence of every eval case is asserted with cvae_plan_pass / cvae_plan_pass_deep before the pass runs, so a
case cannot silently move to another kernel.  The forms of a train case are asserted with cvae_plan_train_pass: off H = 64 / 1024
(persist_ok, csrc/cvae_train.inc) every pass is the per-step forward (k_gru_step_train, FWD_STEPS) and the per-step reverse
(k_gru_step_bwd + k_bwd_step_gemm, BWD_STEPS); the persistent forms of H = 64 / 1024 have a table of their own, tests/train_cases.py,
which runs through the same TrainNet.

What the widths reach, by kernel:
  k_gru_steps_ll      H % 64 == 0 up to 1024, <= 3 rows: 128 (waves 1-3 idle but voting), 192 (wave 0 with three words), 320 (wave 1
                      with one word), 960 (wave 3 with three)
  k_gru_steps<PERSIST> / k_outproj   K split over four waves as (nch * wave) >> 2: 16 (three empty shares), 48 / 80 / 144 (uneven),
                      128 (even), 1008 (252 blocks: the largest resident grid); 1040 / 2064: T launches
  k_gru_step_train    chunks per wave (of H / 8; 4 per trip, 8 per loop turn): 0-1 (16), 1-2 (48), 2-3 (80), 4-5 (144), 8-9 (272),
                      32-33 (1040), 64-65 (2064, with the default two column tiles); <2> and <2, 8> forced at 144
  k_gru_step_bwd      ceil(H / 256) blocks per row with a j < H guard: partial block after full ones at 272, 1040, 2064
  k_bwd_step_gemm     3H/16 chunks over 8 slices x 4 waves: empty slices and waves at 16 and 48, a round plus a tail at 2064
"""
import collections
import os

import numpy as np

import _cabi
import gemm_util as gu
import synth
import train_util
import width_ref
from stacked_util import EMU_PASS, TIGHT_CHAIN, TIGHT_PASS      # noqa: F401  (the project's own eval bounds, unchanged)

# the emulator's training bounds are literals in tests/test_emu_train.py (outputs and carried state 5e-5, dx and parameter gradients
# 1e-4, relative to each tensor's largest entry); the device's is test_gpu_train.TIGHT_REL, imported by tests/test_width_gpu.py
EMU_TRAIN_OUT = 5e-5
EMU_TRAIN_GRAD = 1e-4

P_, E_, S_ = _cabi.FLAG_PERSISTENT, _cabi.FLAG_EXACT3, _cabi.FLAG_SPLIT_F16
DEFAULT_FLAGS = P_ | E_ | S_
LL, GENERIC, PER_STEP = _cabi.EVAL_LL, _cabi.EVAL_GENERIC, _cabi.EVAL_PER_STEP
FORM_NAMES = {LL: "LL", GENERIC: "GENERIC", PER_STEP: "PER_STEP"}
EMU_MAX_H = 192          # the emulator stage runs every case up to this width; wider ones take > 10 s per pass there

GRAD_KEYS = {"conv0_w": "conv.conv.0.weight", "conv0_b": "conv.conv.0.bias", "conv1_w": "conv.conv.1.weight",
             "conv1_b": "conv.conv.1.bias", "w_ih": "gru.weight_ih_l0", "w_hh": "gru.weight_hh_l0", "b_ih": "gru.bias_ih_l0",
             "b_hh": "gru.bias_hh_l0", "out_w": "out_1.weight", "out_b": "out_1.bias"}


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
class EvalCase(collections.namedtuple("EvalCase", "H rows T in_dim lat form flags layers twin")):
    """One eval problem: encoder form (scale_in, clamp_vae), out_dim = 2 * lat.  form: what cvae_plan_pass (layers 1) or
    cvae_plan_pass_deep (layers 2) must report for (rows, T, flags).  twin: also run flags 0 (PER_STEP) and ask for identical bits."""
    __slots__ = ()

    @property
    def id(self):
        return "h%d-r%d-%s%s%s" % (self.H, self.rows, "deep-" if self.layers > 1 else "", FORM_NAMES.get(self.form, str(self.form)) if
                                   self.layers == 1 else "GENERIC", "" if self.flags else "-flags0")

    @property
    def tag(self):
        return "width/e/%d/%d/%d/%d/%d" % (self.H, self.rows, self.lat, self.layers, self.flags)


def _in_dim(H):
    return 10 if (H // 16) % 2 else 6


def _ecase(H, rows, T, form, flags=DEFAULT_FLAGS, lat=4, layers=1, twin=False):
    return EvalCase(H, rows, T, _in_dim(H), lat, form, flags, layers, twin)


def _eval_table():
    t = []
    for H in (128, 192, 320, 960):                  # T = 7: both slot parities of the word exchange, windows of 4 + 3 frames
        t += [_ecase(H, rows, 7, LL) for rows in (1, 2, 3)]                  # the three NR instances
    for H in (16, 48, 80, 144, 128, 1008):          # rows: one 16-row tile, two, and a second trip of the 4-tile loop
        t += [_ecase(H, rows, 6, GENERIC, twin=True) for rows in (5, 17, 65)]
    for H in (1040, 2064):                          # H/4 blocks are not resident on 256 CUs; no word exchange above 1024
        t += [_ecase(H, rows, 5, PER_STEP) for rows in (2, 17)]
    t += [_ecase(H, 5, 6, PER_STEP, flags=0) for H in (48, 144)]
    return t


EVAL_CASES = _eval_table()
# projection classes: Cop = 16 (one tile), 32 (two tiles: the GEMM projection), 64 (four tiles), at one LL and one GENERIC width;
# each with y_last requested (GEMM + epilogue) and NULL (k_outproj<1|4> at one and four tiles, whose K split is uneven here)
PROJ_CASES = [_ecase(H, rows, T, form, lat=lat) for H, rows, T, form in ((128, 2, 7, LL), (48, 5, 6, GENERIC)) for lat in (4, 10, 25)]
DEEP_CASES = [_ecase(H, 5, 6, _cabi.DEEP_GENERIC, layers=2) for H in (48, 128)]


class TrainCase(collections.namedtuple("TrainCase", "H rows T kind carry opts")):
    """One train-mode pass + backward.  kind "enc": scale_in, clamp_vae; "dec": scale_out.  carry: h_in and a non-zero y_in given.
    opts: library options of the case as sorted (name, value) pairs."""
    __slots__ = ()

    @property
    def id(self):
        o = "".join("-%s%d" % kv for kv in self.opts)
        return "h%d-r%d-t%d-%s%s%s" % (self.H, self.rows, self.T, self.kind, "-carry" if self.carry else "", o)

    @property
    def tag(self):
        return "width/t/" + self.id

    wtag = tag          # the weights are drawn with the case's own tag
    sub_of = 0          # (train_cases.FormCase: the case is the first rows of a larger problem)


def _tcase(H, rows, T, kind="enc", carry=False, **opts):
    return TrainCase(H, rows, T, kind, carry, tuple(sorted(opts.items())))


TRAIN_CASES = [
    _tcase(16, 2, 4),                                # two of four waves without chunks; empty slices of the backward GEMM
    _tcase(48, 5, 4), _tcase(48, 17, 3),             # shares of 1-2 chunks; NRTB 1 and 2
    _tcase(80, 5, 4), _tcase(80, 17, 3),             # shares of 2-3 chunks
    _tcase(144, 3, 5), _tcase(144, 65, 3),           # trip + tail; five row tiles: NRTB 4 and a ragged second group
    _tcase(144, 20, 4, step_col_tiles=2),            # k_gru_step_train<2>
    _tcase(144, 130, 3, step_col_tiles=2),           # <2, 8> at Bp = 144: nine row tiles
    _tcase(272, 5, 4),                               # 8-9 chunks per wave; partial second block of k_gru_step_bwd
    _tcase(1040, 4, 3),                              # five blocks of k_gru_step_bwd, the last partial
    _tcase(2064, 17, 4),                             # default two column tiles, 64-65 chunks per wave; round + tail in k_bwd_step_gemm
    _tcase(48, 5, 4, kind="dec"), _tcase(144, 3, 5, kind="dec"),
    _tcase(80, 5, 4, carry=True), _tcase(272, 5, 4, carry=True),
    _tcase(80, 5, 1), _tcase(272, 5, 1),
    _tcase(48, 5, 4, train_old_gemm=1),
]
assert all(c.H not in (64, 1024) for c in TRAIN_CASES), "this table is about the per-step training kernels"


def emu_case(c):
    """The case as the emulator stage runs it (fewer frames: a pass costs about a second per frame there), or None where it runs on
    the device only.  Every width up to EMU_MAX_H and every row class stays; what moves to the device stage is
      * every width above EMU_MAX_H (12 s and more per pass);
      * GENERIC at 65 rows for H = 80, 128, 144 (15-40 s per case; 65 rows run here at H = 16 and 48: the second trip of the 4-tile loop
        with empty and uneven wave shares);
      * LL at H = 192 with 1 and 3 rows (15-25 s; the three row-count instances run here at H = 128, H = 192 at 2 rows);
      * the train case of 130 rows (25 s; k_gru_step_train<2, 8> runs here at H = 64 in tests/test_emu_train.py, and the chunk shares of
        H = 144 with two column tiles in the 20-row case)."""
    if c.H > EMU_MAX_H:
        return None
    if isinstance(c, TrainCase):
        if c.rows >= 130:
            return None
        return c._replace(T=2) if c.rows >= 65 else c
    if c.layers == 1 and c.form == GENERIC and c.rows >= 65 and c.H > 48:
        return None
    if c.form == LL and c.layers == 1 and c.H == 192 and c.rows != 2:
        return None
    return c._replace(T=5 if (c.form == LL and c.layers == 1) else 4)      # LL: both slot parities, windows of 3 + 2 frames


# ---------------------------------------------------------------------------------------------------------------
# arenas and backends
# ---------------------------------------------------------------------------------------------------------------
ALIGN = 64      # floats: views start 256-byte aligned


def arena_floats(sizes):
    """Floats an arena needs for views of these sizes."""
    return gu.NumpyArena.GAP + sum(gu.up(n + gu.NumpyArena.GAP, ALIGN) for n in sizes) + ALIGN


class WidthArena(object):
    """What the drivers add to gemm_util.NumpyArena / its torch twin: views that keep the arena's NaN fill (work areas nobody
    initialises), 256-byte aligned views, and a guard check that reads the gaps only (the arenas here reach hundreds of MiB)."""

    def reserve(self, n):
        off = self.top
        assert off % ALIGN == 0 and off + n + self.GAP <= len(self.buf), (off, n, len(self.buf))
        self.top = gu.up(off + n + self.GAP, ALIGN)
        self.used.append((off, n))
        return off

    def place(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        off = self.reserve(a.size)
        self.write(off, a)
        return off

    def guards_intact(self):
        pos = 0
        for off, n in sorted(self.used) + [(self.top, 0)]:
            if not np.all(np.isnan(self.read(pos, off - pos))):
                return False
            pos = off + n
        return True


class NumpyWidthArena(WidthArena, gu.NumpyArena):
    pass


class NpMem(object):
    """ "Device" memory is numpy memory (the emulator build)."""
    name, stream = "emulator", None

    def __init__(self, lib):
        self.lib, self._pass = lib, None
        self.sink = np.zeros(4, np.int32)

    def arena(self, floats):
        return NumpyWidthArena(floats)

    def scratch(self, floats):
        """The arena of one pass: reused (and NaN-filled again) from pass to pass, grown when a pass needs more."""
        if self._pass is None or len(self._pass.buf) < floats:
            self._pass = None
            self._pass = self.arena(floats)
        self._pass.reset()
        return self._pass

    def sink_ptr(self):
        return self.sink.ctypes.data

    def sink_words(self):
        return [int(v) for v in self.sink]


class TorchMem(NpMem):
    name = "device"

    def __init__(self, lib, dev):
        import torch
        from test_gemm_gpu import TorchArena

        class TorchWidthArena(WidthArena, TorchArena):
            pass
        self._arena_cls, self.dev = TorchWidthArena, dev
        self.lib, self._pass = lib, None
        self.stream = torch.cuda.current_stream().cuda_stream
        self.sink = torch.zeros(4, dtype=torch.int32).pin_memory()       # (device-writable, host-readable: what cvae_set_status_sink asks for)

    def arena(self, floats):
        return self._arena_cls(self.dev, floats)

    def sink_ptr(self):
        return self.sink.data_ptr()

    def sink_words(self):
        return [int(v) for v in self.sink.tolist()]


def _floats(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    return nbytes // 4


# ---------------------------------------------------------------------------------------------------------------
# eval driver
# ---------------------------------------------------------------------------------------------------------------
class EvalNet(object):
    """One prepared GRU_RNN (n_layers GRU layers; 1: the one-layer entry points, >= 2: the _deep ones) inside an arena of its own."""

    def __init__(self, mem, sd, in_dim, out_dim, hidden, n_layers=1):
        lib = mem.lib
        self.mem, self.L = mem, n_layers
        self.d = d = lib.desc(in_dim, out_dim, hidden, 3, 2, "scale_in.weight" in sd, "scale_out.weight" in sd)
        deep = n_layers > 1
        self.pbytes = lib.prepared_bytes_deep(d, n_layers) if deep else lib.prepared_bytes(d)
        sbytes = lib.prepare_scratch_bytes_deep(d, n_layers) if deep else lib.prepare_scratch_bytes(d)
        fields = [(f, k) for f, k in _cabi.STATE_KEYS.items() if k in sd]
        upper = _cabi.upper_layer_keys(n_layers)
        sizes = [_floats(self.pbytes), _floats(sbytes)] + [sd[k].size for _, k in fields] + [sd[k].size for keys in upper for k in keys]
        self.A = A = mem.arena(arena_floats(sizes))
        wp = {f: A.address(A.place(sd[k])) for f, k in fields}
        up = [tuple(A.address(A.place(sd[k])) for k in keys) for keys in upper]
        self.prepared = A.reserve(_floats(self.pbytes))
        scr = A.reserve(_floats(sbytes))
        if deep:
            lib.net_prepare_deep(d, n_layers, wp, up, A.address(self.prepared), self.pbytes, A.address(scr), sbytes, mem.stream)
        else:
            lib.net_prepare(d, wp, A.address(self.prepared), self.pbytes, A.address(scr), sbytes, mem.stream)
        A.sync()
        assert A.guards_intact(), "cvae_net_prepare wrote outside the prepared image / its scratch (H = %d)" % hidden

    def plan(self, rows, T, flags):
        lib = self.mem.lib
        return lib.plan_pass_deep(self.d, self.L, rows, T, flags) if self.L > 1 else lib.plan_pass(self.d, rows, T, flags)

    def forward(self, x, y_in, h_in=None, clamp_lat_dim=-1, flags=DEFAULT_FLAGS, want_y_last=True, expect=None, what=""):
        """x [B,T,Cin], y_in [B,1,Co], h_in [L,B,H] or None -> (trj [B,T,Co], y_last [B,1,Co] or None, h [L,B,H]) float32 numpy."""
        mem, lib, d, L = self.mem, self.mem.lib, self.d, self.L
        x = np.asarray(x, np.float32)
        B, T, Cin = x.shape
        Co, H = d.out_dim, d.hidden
        if expect is not None:
            got = self.plan(B, T, flags)
            assert got == expect, "%s: planned form %d, the table says %d" % (what, got, expect)
        wsb = lib.pass_workspace_bytes_deep(d, L, B, T) if L > 1 else lib.pass_workspace_bytes(d, B, T)
        sizes = [x.size, B * Co, L * B * H, B * T * Co, B * Co, L * B * H, _floats(wsb)]
        A = mem.scratch(arena_floats(sizes))
        ox, oy = A.place(x), A.place(np.asarray(y_in, np.float32).reshape(B, Co))
        oh = None if h_in is None else A.place(np.asarray(h_in, np.float32).reshape(L, B, H))
        otrj, ohl = A.reserve(B * T * Co), A.reserve(L * B * H)
        oyl = A.reserve(B * Co) if want_y_last else None
        ows = A.reserve(_floats(wsb))
        adr = lambda o: None if o is None else A.address(o)
        pin = lib.pass_input((adr(ox), Cin, Cin))
        if L > 1:
            lib.gru_rnn_forward_deep(d, L, self.A.address(self.prepared), pin, adr(oy), adr(oh), B, T, clamp_lat_dim, adr(otrj), adr(oyl),
                                     adr(ohl), adr(ows), wsb, flags, mem.stream)
        else:
            lib.gru_rnn_forward(d, self.A.address(self.prepared), pin, adr(oy), adr(oh), B, T, clamp_lat_dim, adr(otrj), adr(oyl), adr(ohl),
                                adr(ows), wsb, flags, mem.stream)
        A.sync()
        st = lib.workspace_status(adr(ows), mem.stream)
        assert st == [0, 0, 0, 0], "%s: status words %s" % (what, st)
        assert A.guards_intact(), "%s: a write outside a buffer of the pass" % what
        assert self.A.guards_intact(), "%s: a write outside the prepared image" % what
        trj, hl = A.read(otrj, B * T * Co).reshape(B, T, Co), A.read(ohl, L * B * H).reshape(L, B, H)
        yl = A.read(oyl, B * Co).reshape(B, 1, Co) if want_y_last else None
        for name, a in (("trj_out", trj), ("y_last", yl), ("h_last", hl)):
            assert a is None or np.all(np.isfinite(a)), "%s: %s not fully written / not finite" % (what, name)
        return trj, yl, hl


def eval_problem(c):
    """(synthetic problem, encoder state dict) of an eval case; a stacked case draws the upper layers as well."""
    P = synth.CycleVAEProblem(B=c.rows, T=c.T, in_dim=c.in_dim, out_dim=c.in_dim - 4, lat_dim=c.lat, hidden=c.H, n_cyc=1,
                              bias_scale=0.1, tag=c.tag, hidden_layers=c.layers)
    return P


def maxdiff(got, ref):
    d = 0.0
    for a, b in zip(got, ref):
        if a is not None:
            assert a.shape == b.shape, (a.shape, b.shape)
            d = max(d, float(np.max(np.abs(a.astype(np.float64) - b))))
    return d


def run_eval_case(mem, c, ref, note, bound):
    """The four stages of an eval case against `ref` (width_ref.eval_reference of eval_problem(c)); returns the largest distance."""
    P = eval_problem(c)
    Co, t0 = 2 * c.lat, (c.T + 1) // 2
    net = EvalNet(mem, P.enc, c.in_dim, Co, c.H, c.layers)
    run = lambda name, *a, **k: net.forward(*a, clamp_lat_dim=c.lat, flags=c.flags, what="%s %s" % (c.id, name), **k)
    worst = {}
    whole = run("whole", P.x, P.y_in_enc, expect=c.form)
    worst["whole"] = maxdiff(whole, ref["whole"])
    if c.twin:      # the any-H kernel behind its grid barrier repeats the per-step launches bit for bit
        assert net.plan(c.rows, c.T, 0) == PER_STEP
        step = net.forward(P.x, P.y_in_enc, clamp_lat_dim=c.lat, flags=0, what=c.id + " whole, flags 0")
        for name, a, b in zip(("trj_out", "y_last", "h_last"), whole, step):
            assert a.tobytes() == b.tobytes(), "%s: %s of GENERIC differs from PER_STEP (max|d| %.3e)" % (c.id, name, float(np.max(np.abs(a - b))))
    w0 = run("window 0", P.x[:, :t0], P.y_in_enc)
    w1 = run("window 1", P.x[:, t0:], w0[1], h_in=w0[2])            # the library's own carried (y_last, h)
    worst["windows"] = max(maxdiff(w0, ref["win0"]), maxdiff(w1, ref["win1"]))
    # h_in with a y_in that is not out_1(h_in): the frame-0 correction (cvae_t0_fix) with a Co that is no multiple of 8 at lat 10 / 25
    y_odd, h_ref = (ref["win0"][1] + width_ref.Y_ODD).astype(np.float32), ref["win0"][2].astype(np.float32)
    worst["odd y_in"] = maxdiff(run("odd y_in", P.x[:, t0:], y_odd, h_in=h_ref), ref["odd"])
    worst["T=1"] = maxdiff(run("T=1", P.x[:, :1], P.y_in_enc), ref["one"])
    for k, v in worst.items():
        note("%-9s eval  %-28s %-9s max|d| = %.3e" % (mem.name, c.id, k, v))
    w = max(worst.values())
    assert w <= bound, (c.id, worst, bound)
    return w


def run_proj_case(mem, c, ref, note, bound):
    """One pass with y_last requested, one with y_last NULL through the C ABI, and one with h_in and an off-manifold y_in."""
    P = eval_problem(c)
    net = EvalNet(mem, P.enc, c.in_dim, 2 * c.lat, c.H, c.layers)
    worst = 0.0
    for want in (True, False):
        got = net.forward(P.x, P.y_in_enc, clamp_lat_dim=c.lat, flags=c.flags, want_y_last=want, expect=c.form,
                          what="%s out_dim %d y_last %s" % (c.id, 2 * c.lat, want))
        d = maxdiff(got, ref["whole"])
        note("%-9s proj  %-28s out_dim %2d y_last %-5s max|d| = %.3e" % (mem.name, c.id, 2 * c.lat, want, d))
        worst = max(worst, d)
    # the frame-0 correction (cvae_t0_fix: h_in with a y_in that is not out_1(h_in)) at this out_dim: 20 and 50 are no multiples of 8
    t0 = (c.T + 1) // 2
    y_odd, h_ref = (ref["win0"][1] + width_ref.Y_ODD).astype(np.float32), ref["win0"][2].astype(np.float32)
    got = net.forward(P.x[:, t0:], y_odd, h_in=h_ref, clamp_lat_dim=c.lat, flags=c.flags, what="%s out_dim %d odd y_in" % (c.id, 2 * c.lat))
    d = maxdiff(got, ref["odd"])
    note("%-9s proj  %-28s out_dim %2d odd y_in      max|d| = %.3e" % (mem.name, c.id, 2 * c.lat, d))
    worst = max(worst, d)
    assert worst <= bound, (c.id, worst, bound)
    return worst


def eval_reference(c):
    P = eval_problem(c)
    return width_ref.eval_reference(P.enc, P.x, P.y_in_enc, c.lat, (c.T + 1) // 2)


# ---------------------------------------------------------------------------------------------------------------
# train driver
# ---------------------------------------------------------------------------------------------------------------
class TrainNet(object):
    """One train image (cvae_net_prepare_train, every MFMA-order variant) inside an arena of its own."""

    def __init__(self, mem, sd, in_dim, out_dim, hidden):
        lib = mem.lib
        self.mem = mem
        self.sd = sd
        self.d = d = lib.desc(in_dim, out_dim, hidden, 3, 2, "scale_in.weight" in sd, "scale_out.weight" in sd)
        self.ibytes = lib.train_image_bytes(d)
        fields = [(f, k) for f, k in _cabi.STATE_KEYS.items() if k in sd]
        self.A = A = mem.arena(arena_floats([_floats(self.ibytes)] + [sd[k].size for _, k in fields]))
        wp = {f: A.address(A.place(sd[k])) for f, k in fields}
        self.image = A.reserve(_floats(self.ibytes))
        lib.net_prepare_train(d, wp, A.address(self.image), self.ibytes, mem.stream, gru_drop_p=0.5)
        A.sync()
        assert A.guards_intact(), "cvae_net_prepare_train wrote outside the train image (H = %d)" % hidden

    def run(self, x, y_in, h_in, cmask, gmask, cot, clamp_lat_dim, what="", counters=False, tape=False):
        """Forward + backward of sum(out * cot): dict(out, y_last [B,Co], h_last [B,H], dx, grads {state key: array}).  counters: also
        "counters", the eight words of cvae_train_debug_counters read from the pass's scratch (option train_prof).  tape: also "tape",
        the whole tape as the forward left it (read behind the backward, which only reads it)."""
        mem, lib, d = self.mem, self.mem.lib, self.d
        x = np.asarray(x, np.float32)
        B, T, Cin = x.shape
        Co, H = d.out_dim, d.hidden
        tb, sb = lib.train_tape_bytes(d, B, T), lib.train_scratch_bytes(d, B, T)
        gshape = {f: self.sd[k].shape for f, k in GRAD_KEYS.items()}
        sizes = [x.size, B * Co, B * H, cmask.size, gmask.size, B * T * Co, B * Co, B * H, _floats(tb), _floats(sb), B * T * Co, x.size]
        A = mem.scratch(arena_floats(sizes + [int(np.prod(s)) for s in gshape.values()]))
        ox, oy = A.place(x), A.place(np.asarray(y_in, np.float32).reshape(B, Co))
        oh = None if h_in is None else A.place(np.asarray(h_in, np.float32).reshape(B, H))
        ocm, ogm, ocot = A.place(cmask), A.place(gmask), A.place(cot)
        oout, oyl, ohl, odx = A.reserve(B * T * Co), A.reserve(B * Co), A.reserve(B * H), A.reserve(x.size)
        og = {f: A.reserve(int(np.prod(s))) for f, s in gshape.items()}
        otape, oscr = A.reserve(_floats(tb)), A.reserve(_floats(sb))
        adr = lambda o: None if o is None else A.address(o)
        mem.sink[:] = 0
        lib.set_status_sink(mem.sink_ptr())
        try:
            lib.forward_train(d, self.A.address(self.image), adr(ox), adr(oy), adr(oh), B, T, clamp_lat_dim, adr(ocm), adr(ogm), 11, 0.5,
                              adr(oout), adr(oyl), adr(ohl), adr(otape), tb, adr(oscr), sb, mem.stream)
            lib.backward(d, self.A.address(self.image), adr(ocot), B, T, clamp_lat_dim, adr(otape), adr(oscr), sb, adr(odx),
                         {f: adr(o) for f, o in og.items()}, accumulate=False, stream=mem.stream)
            A.sync()
            words = lib.train_debug_counters(d, B, T, adr(oscr), mem.stream) if counters else None
        finally:
            lib.set_status_sink(None)
        assert mem.sink_words() == [0, 0, 0, 0], "%s: status sink %s" % (what, mem.sink_words())
        assert A.guards_intact(), "%s: a write outside a buffer of the pass" % what
        assert self.A.guards_intact(), "%s: a write outside the train image" % what
        res = {"out": A.read(oout, B * T * Co).reshape(B, T, Co), "y_last": A.read(oyl, B * Co).reshape(B, Co),
               "h_last": A.read(ohl, B * H).reshape(B, H), "dx": A.read(odx, x.size).reshape(x.shape),
               "grads": {GRAD_KEYS[f]: A.read(o, int(np.prod(gshape[f]))).reshape(gshape[f]) for f, o in og.items()}}
        for name, a in list(res.items())[:4] + list(res["grads"].items()):
            assert np.all(np.isfinite(a)), "%s: %s not fully written / not finite" % (what, name)
        if counters:
            res["counters"] = words
        if tape:
            res["tape"] = A.read(otape, _floats(tb))
        return res


def train_problem(c):
    """(state dict, in_dim, out_dim, x, y_in, h_in, cmask, gmask, cot, clamp_lat_dim) of a train case: inputs of
    synth.CycleVAEProblem, masks of train_util.make_masks (every form sees the same dropout).  Weights and feature statistics are
    drawn with c.wtag, inputs and masks with c.tag (the same for a width case; train_cases.FormCase shares one set of weights per H
    and one set of inputs per problem, however the pass is tiled).  c.sub_of > 0: the first c.rows rows of the c.sub_of-row problem."""
    ind, rows = _in_dim(c.H), c.sub_of or c.rows
    assert rows >= c.rows
    P = synth.CycleVAEProblem(B=rows, T=c.T, in_dim=ind, out_dim=ind - 4, lat_dim=4, hidden=c.H, n_cyc=1, bias_scale=0.1, tag=c.wtag)
    if c.wtag != c.tag:
        P.x = synth.features(c.tag + "/x", rows, c.T, P.mu, P.sigma)
    masks = train_util.make_masks(P, 1, 1, tag=c.tag + "/masks")
    if c.kind == "enc":
        sd, i, o, x, y_in, clamp = P.enc, ind, 8, P.x, P.y_in_enc, 4
    else:
        x = np.concatenate([P.code_src, synth.normal(c.tag + "/z", (rows, c.T, 4))], 2).astype(np.float32)
        sd, i, o, y_in, clamp = P.dec, 6, ind - 4, P.y_in_dec, -1
    h_in = None
    if c.carry:
        h_in = (0.3 * synth.normal(c.tag + "/h_in", (1, rows, c.H))).astype(np.float32)
        y_in = (y_in + 0.2 * synth.normal(c.tag + "/y_in", y_in.shape)).astype(np.float32)
    cm, gm = masks[c.kind][0]
    cot = synth.normal(c.tag + "/cot", (rows, c.T, o))
    if rows != c.rows:
        n = c.rows
        x, y_in, cm, gm, cot = x[:n], y_in[:n], cm[:n], gm[:, :n], cot[:n]
        h_in = None if h_in is None else h_in[:, :n]
        x, y_in, cm, gm, cot = (np.ascontiguousarray(a) for a in (x, y_in, cm, gm, cot))
    return sd, i, o, x, y_in, h_in, cm, gm, cot, clamp


def train_reference(c):
    sd, _, _, x, y_in, h_in, cm, gm, cot, clamp = train_problem(c)
    return width_ref.train_reference(sd, x, y_in, h_in, cm, gm, cot, clamp)


def rel_err(a, ref):
    """max|d| relative to the tensor's largest entry (at least 1), as tests/test_emu_train.py and tests/test_gpu_train.py measure."""
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.max(np.abs(a.astype(np.float64) - ref))) / max(1.0, float(np.max(np.abs(ref))))


def train_distances(got, ref):
    """({output: distance}, {gradient: distance}) of TrainNet.run's result to a train_reference."""
    outs = {k: rel_err(got[k], ref[k]) for k in ("out", "y_last", "h_last")}
    grads = {"dx": rel_err(got["dx"], ref["dx"])}
    for k in GRAD_KEYS.values():
        grads["d" + k] = rel_err(got["grads"][k], ref["grads"][k])
    return outs, grads


def check_train_result(mem, c, got, ref, note, bound_out, bound_grad):
    """Prints and records the distances of a train pass to its reference, then holds them to the bounds; (worst output, worst gradient)."""
    outs, grads = train_distances(got, ref)
    wo, wg = max(outs.values()), max(grads.values())
    note("%-9s train %-36s outputs %.3e (%s)  gradients %.3e (%s)" % (mem.name, c.id, wo, max(outs, key=outs.get), wg, max(grads, key=grads.get)))
    assert wo <= bound_out, (c.id, outs, bound_out)
    assert wg <= bound_grad, (c.id, grads, bound_grad)
    return wo, wg


def run_train_case(mem, c, ref, note, bound_out, bound_grad):
    """One case of TRAIN_CASES against `ref` (train_reference(c)); the caller has set c.opts on mem.lib.  The plan must be the per-step
    launches in both directions.  Returns (worst output, worst gradient)."""
    sd, i, o, x, y_in, h_in, cm, gm, cot, clamp = train_problem(c)
    net = TrainNet(mem, sd, i, o, c.H)
    plan = mem.lib.plan_train_pass(net.d, c.rows, c.T)
    assert (plan["fwd"], plan["bwd"]) == (_cabi.TRAIN_FWD_STEPS, _cabi.TRAIN_BWD_STEPS), "%s: planned %s, the table is about the per-step kernels" % (c.id, plan)
    got = net.run(x, y_in, h_in, cm, gm, cot, clamp, what=c.id)
    return check_train_result(mem, c, got, ref, note, bound_out, bound_grad)


# ---------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------
def make_note(report_name):
    """note(msg): print, and append to <CYCLEVAE_REPORT_DIR>/<report_name> when that variable names a directory."""
    def note(msg):
        d = os.environ.get("CYCLEVAE_REPORT_DIR")
        if d:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, report_name), "a") as f:
                f.write(msg + "\n")
        print(msg)
    return note
