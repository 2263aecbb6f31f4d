"""Which recurrence an eval pass of a one-layer network takes (plan_eval_pass in csrc/cvae_lib.hip, reported by cvae_plan_pass;
the rule table is DESIGN.md 4.1).  The CPU tests ask the host-fiber build of the real library, whose device has 256 CUs like an
MI355X; cvae_plan_pass launches nothing, so the 1024- and 2048-wide rows cost nothing."""
import numpy as np
import pytest

import _cabi
import synth
from emu_util import NpNet, emu_lib, ptr

P, G, HST, S, E = _cabi.FLAG_PERSISTENT, _cabi.FLAG_GENERIC_STEP, _cabi.FLAG_HOISTED_FRONTEND, _cabi.FLAG_SPLIT_F16, _cabi.FLAG_EXACT3
PER_STEP, GENERIC, V2, V4, V5, V6, LL = (_cabi.EVAL_PER_STEP, _cabi.EVAL_GENERIC, _cabi.EVAL_V2, _cabi.EVAL_V4, _cabi.EVAL_V5,
                                         _cabi.EVAL_V6, _cabi.EVAL_LL)

# (in_dim, H, rows, flags, T, options) -> form; kernel_size 3, 256 CUs
TABLE = [
    (54, 1024, 64, P | E | S, 8, {}, V6),            # KFW 8, rows padded to 64
    (36, 1024, 64, P | E | S, 8, {}, V6),            # KFW 6
    (54, 1024, 4, P | E | S, 8, {}, V6),             # a half-empty 32-row tile rather than the pair kernel
    (54, 1024, 2, P | E | S, 8, {}, LL),
    (54, 1024, 2, P | E | S, 8, {"no_ll": 1}, V5),
    (54, 1024, 64, P | S, 8, {}, V5),
    (54, 1024, 64, P, 8, {}, V4),
    (54, 1024, 64, P | HST, 8, {}, V2),
    (54, 1024, 64, P | E | S | HST, 8, {}, V2),
    (54, 1024, 64, P | G, 8, {}, GENERIC),
    (54, 1024, 64, P | E | S | G, 8, {}, GENERIC),
    (54, 1024, 64, 0, 8, {}, PER_STEP),
    (54, 1024, 64, P | E | S, 1, {}, PER_STEP),      # one frame: nothing to keep resident for
    (20, 1024, 64, P | E | S, 8, {}, V2),            # KFW 4: no fused instance
    (6, 1024, 64, P | S, 8, {}, V2),                 # KFW 2: an instance at H = 64 only
    (54, 2048, 64, P | E | S, 8, {}, V6),            # streamed third limb
    (54, 2048, 2, P | E | S, 8, {}, PER_STEP),       # no LL above H = 1024; 512 blocks are not resident
    (54, 2048, 64, P, 8, {}, PER_STEP),
    (6, 64, 8, P | E | S, 8, {}, V6),
    (6, 64, 8, P | S, 8, {}, V5),
    (6, 64, 8, P, 8, {}, V4),
    (6, 64, 8, P | HST, 8, {}, V2),
    (6, 64, 8, P | G, 8, {}, GENERIC),
    (6, 64, 8, 0, 8, {}, PER_STEP),
    (6, 64, 2, P | E | S, 8, {}, LL),
    (10, 64, 8, P | E | S, 8, {}, V6),               # KFW 3
    (10, 64, 8, P | S, 8, {}, V2),                   # KFW 3: k_gru_steps_v5 / v4 are not built for it
    (10, 64, 20, P, 8, {}, V2),
    (6, 128, 8, P | E | S, 8, {}, GENERIC),          # no tuned kernel at H = 128
    (6, 128, 20, P | E | S, 8, {}, GENERIC),
    (6, 128, 2, P | E | S, 8, {}, LL),
    (6, 48, 2, P | E | S, 8, {}, GENERIC),           # LL wants H % 64 == 0
    (6, 1040, 2, P | E | S, 8, {}, PER_STEP),        # 260 blocks on 256 CUs
    # the width classes of tests/width_util.py
    (6, 320, 1, P | E | S, 8, {}, LL),               # wave 1 of k_gru_steps_ll with one word
    (6, 320, 3, P | E | S, 8, {}, LL),
    (6, 320, 4, P | E | S, 8, {}, GENERIC),          # a fourth row: off the word exchange, no tuned kernel at H = 320
    (10, 960, 3, P | E | S, 8, {}, LL),              # wave 3 with three words
    (10, 960, 17, P | E | S, 8, {}, GENERIC),
    (10, 1008, 2, P | E | S, 8, {}, GENERIC),        # LL wants H % 64 == 0; 252 blocks: the largest resident grid
    (10, 1008, 65, P | E | S, 8, {}, GENERIC),
    (10, 1008, 65, 0, 8, {}, PER_STEP),
    (6, 1040, 17, P | E | S, 8, {}, PER_STEP),
    (6, 1040, 17, P | G, 8, {}, PER_STEP),           # GENERIC_STEP asks for the any-H kernel: still T launches when it is not resident
]


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def test_plan_table(lib, options):
    for in_dim, H, rows, flags, T, opts, form in TABLE:
        lib.reset_options()
        options(**opts)
        got = lib.plan_pass(lib.desc(in_dim, 8, H, 3, 2, True, False), rows, T, flags)
        assert got == form, (in_dim, H, rows, flags, T, opts, got, form)
    lib.reset_options()
    with pytest.raises(_cabi.CvaeError):
        lib.plan_pass(lib.desc(6, 8, 64, 3, 2, True, False), 0, 8, P)
    with pytest.raises(_cabi.CvaeError):
        lib.plan_pass(lib.desc(6, 8, 60, 3, 2, True, False), 8, 8, P)


def test_range_word_follows_the_plan_and_retired_options_are_unknown(lib):
    """The prologue is handed the range word exactly when the planned form builds limb operands (V6: triples, V5: pairs): a
    carried-in state of 1e5 raises status 7 there and nowhere else.  The pair copies are written for every SPLIT_F16 pass off V6,
    but a pass that ends on the word-exchange kernel reads none of them."""
    Q = synth.CycleVAEProblem(B=8, T=8, in_dim=6, out_dim=4, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="evalplan")
    net = NpNet(lib, Q.enc, 6, 8, 64)
    lib.reset_options()
    h = (0.5 * synth.normal("evalplan/h_in", (8, 64))).astype(np.float32)
    h[1, 5] = 1e5
    for rows, flags, form, raised in ((8, P | E | S, V6, True), (8, P | S, V5, True), (8, P, V4, False), (8, P | HST, V2, False),
                                      (2, P | E | S, LL, False)):
        assert lib.plan_pass(net.d, rows, 8, flags) == form
        x = np.ascontiguousarray(Q.x[:rows], np.float32)
        y = np.ascontiguousarray(Q.y_in_enc.reshape(8, 8)[:rows], np.float32)
        hin = np.ascontiguousarray(h[:rows])
        trj = np.full((rows, 8, 8), np.nan, np.float32)
        ws = np.full(lib.pass_workspace_bytes(net.d, rows, 8) // 4, np.float32(7.0), np.float32)
        lib.gru_rnn_forward(net.d, ptr(net.prepared), lib.pass_input((ptr(x), 6, 6)), ptr(y), ptr(hin), rows, 8, 4, ptr(trj), None, None,
                            ptr(ws), ws.nbytes, flags)
        st = lib.workspace_status(ptr(ws))
        assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == (_cabi.STATUS_RANGE if raised else 0), (rows, flags, st)
    for name in ("old_outproj", "t0_in_kernel"):
        with pytest.raises(_cabi.CvaeError, match="unknown option"):
            lib.set_option(name, 1)
        with pytest.raises(_cabi.CvaeError, match="unknown option"):
            lib.get_option(name)


def test_form_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cyclevae_hip.h")).read()
    for name in ("PER_STEP", "GENERIC", "V2", "V4", "V5", "V6", "LL"):
        assert int(re.search(r"CVAE_EVAL_%s = (\d+)" % name, text).group(1)) == getattr(_cabi, "EVAL_" + name)


@pytest.mark.gpu
def test_headline_passes_plan_the_exact_operand_kernels_on_the_device():
    """On the MI355X itself (its CU count, not the emulator's): the passes of the headline chain."""
    import torch

    import gru_vae
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    lib = gru_vae._lib()
    lib.reset_options()
    enc, dec = lib.desc(54, 64, 1024, 3, 2, True, False), lib.desc(36, 50, 1024, 3, 2, False, True)
    assert lib.plan_pass(enc, 64, 80, P | E | S) == V6
    assert lib.plan_pass(enc, 128, 80, P | E | S) == V6
    assert lib.plan_pass(enc, 2, 80, P | E | S) == LL
    assert lib.plan_pass(dec, 128, 80, P | E | S) == V6
