#!/usr/bin/env python
"""One train-mode forward + backward per row of the training-form table (tests/train_cases.FORM_CASES) through the C ABI, and one
line per row: the plan (cvae_plan_train_pass) and the sha256 of out, y_last, h_last, dx, the ten parameter gradients and the whole
tape (read behind the backward, which only reads it: the forward's tape).  Two builds that compute alike print the same text; the
training twin of tools/eval_plan_launches.py.

The rows run through the tests' own driver (train_cases.Runner -> width_util.TrainNet.run: injected masks, NaN-filled arena, guards,
status sink), so a row that digests also passed the driver's checks.  The scratch is not digested: it holds flag and counter words
whose final values depend on the order in which blocks arrive.

Device only, after the table: two passes with Philox masks (fixed seed) at H = 64, in_dim 10, 64 rows x 256 frames -- T*B*H = 2^20, the
smallest shape at which a pass draws its feedback mask on the side stream -- accumulating into zeroed gradients, one without a side
stream and one with a side stream set (masks and weight gradients go there).

    python tools/train_pass_digests.py [--root TREE] [--emu]
        --root TREE   another checkout whose binding (_cabi.py) and built library to drive
        --emu         the host-fiber build (tests/emu/libcyclevae_emu.so, numpy memory): the H = 64 rows as the emulator tests run them

Under `rocprofv3 --kernel-trace --stats -- python tools/train_pass_digests.py` the per-kernel launch counts say which kernels the
rows took.
"""
import argparse
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT)
ap.add_argument("--emu", action="store_true")
args = ap.parse_args()
tree = os.path.abspath(args.root)
# the binding of the tree under test, under the name the drivers import
spec = importlib.util.spec_from_file_location("_cabi", os.path.join(tree, "cyclevae-vc_amd", "_cabi.py"))
cabi = sys.modules["_cabi"] = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cabi)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "cyclevae-vc_amd")]
import numpy as np

import train_cases as tc
import width_util as wu

path = os.path.join(tree, "tests", "emu", "libcyclevae_emu.so") if args.emu else os.path.join(tree, "cyclevae-vc_amd", "libcyclevae_hip.so")
assert os.path.exists(path), "%s is not built (python __graft_entry__.py in %s)" % (path, tree)
lib = cabi.CvaeLib(path)
if args.emu:
    mem = wu.NpMem(lib)
else:
    import torch
    assert torch.cuda.is_available(), "the device rows need the MI355X (--emu: the host-fiber build)"
    mem = wu.TorchMem(lib, torch.device("cuda:0"))


class Options(object):
    """What the tests' `options` fixture is to train_cases.set_options."""

    def __call__(self, **kw):
        for k, v in kw.items():
            lib.set_option(k, v)


sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def line(name, plan, got, tape):
    grads = " ".join(sha(got["grads"][k]) for k in wu.GRAD_KEYS.values())
    print("%s plan %s out %s y_last %s h_last %s dx %s grads %s tape %s" % (
        name, ",".join("%s=%d" % kv for kv in sorted(plan.items())), sha(got["out"]), sha(got["y_last"]), sha(got["h_last"]), sha(got["dx"]),
        grads, sha(tape)), flush=True)


runner, options, rows = tc.Runner(mem, lambda msg: None, tape=True), Options(), 0
for c in tc.FORM_CASES:
    c = tc.emu_case(c) if args.emu else c
    if c is None:
        continue
    assert c not in runner.results, "%s twice in the table" % c.id
    got = runner.run(c, options)       # (sets the row's options and asserts its plan first)
    d = runner.nets[(c.H, c.kind)].d
    line("row %2d %s" % (rows, c.id), lib.plan_train_pass(d, c.rows, c.T), got, got.pop("tape"))
    rows += 1
lib.reset_options()


def philox_pass(net, x, y_in, cot, side):
    """Forward with masks drawn from the seed, backward accumulating into zeroed gradients; TrainNet.run's layout and result."""
    d, (B, T, _) = net.d, x.shape
    Co, H = d.out_dim, d.hidden
    tb, sb = lib.train_tape_bytes(d, B, T), lib.train_scratch_bytes(d, B, T)
    gshape = {f: net.sd[k].shape for f, k in wu.GRAD_KEYS.items()}
    A = mem.scratch(wu.arena_floats([x.size, B * Co, cot.size, B * T * Co, B * Co, B * H, x.size, tb // 4, sb // 4] + [int(np.prod(s)) for s in gshape.values()]))
    ox, oy, ocot = A.place(x), A.place(y_in.reshape(B, Co)), A.place(cot)
    oout, oyl, ohl, odx = A.reserve(B * T * Co), A.reserve(B * Co), A.reserve(B * H), A.reserve(x.size)
    og = {f: A.place(np.zeros(s, np.float32)) for f, s in gshape.items()}
    otape, oscr = A.reserve(tb // 4), A.reserve(sb // 4)
    adr = A.address
    mem.sink[:] = 0
    lib.set_status_sink(mem.sink_ptr())
    lib.set_side_stream(side.cuda_stream if side is not None else None)
    try:
        lib.forward_train(d, net.A.address(net.image), adr(ox), adr(oy), None, B, T, 4, None, None, 20261021, 0.5, adr(oout), adr(oyl), adr(ohl),
                          adr(otape), tb, adr(oscr), sb, mem.stream)
        lib.backward(d, net.A.address(net.image), adr(ocot), B, T, 4, adr(otape), adr(oscr), sb, adr(odx), {f: adr(o) for f, o in og.items()},
                     accumulate=True, stream=mem.stream)
        lib.join_side_stream(mem.stream)
        A.sync()
    finally:
        lib.set_side_stream(None)
        lib.set_status_sink(None)
    assert mem.sink_words() == [0, 0, 0, 0], "status sink %s" % mem.sink_words()
    assert A.guards_intact() and net.A.guards_intact(), "a write outside a buffer of the pass"
    got = {"out": A.read(oout, B * T * Co), "y_last": A.read(oyl, B * Co), "h_last": A.read(ohl, B * H), "dx": A.read(odx, x.size),
           "grads": {wu.GRAD_KEYS[f]: A.read(o, int(np.prod(gshape[f]))) for f, o in og.items()}}
    assert all(np.all(np.isfinite(a)) for a in list(got.values())[:4] + list(got["grads"].values())), "an output not fully written / not finite"
    return got, A.read(otape, tb // 4)


if not args.emu:
    import synth
    P = synth.CycleVAEProblem(B=64, T=256, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=1, bias_scale=0.1, tag="digests/philox")
    net = wu.TrainNet(mem, P.enc, 10, 8, 64)
    cot = synth.normal("digests/philox/cot", (64, 256, 8))
    for name, side in (("no side stream", None), ("side stream", torch.cuda.Stream())):
        got, tape = philox_pass(net, np.asarray(P.x, np.float32), np.asarray(P.y_in_enc, np.float32), cot, side)
        line("philox h64-r64-t256 %s" % name, lib.plan_train_pass(net.d, 64, 256), got, tape)
        rows += 1
    torch.cuda.synchronize()
print("TRAIN_PASS_DIGESTS_OK %d rows" % rows)
