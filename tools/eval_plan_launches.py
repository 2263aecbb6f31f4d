#!/usr/bin/env python
"""GPU-only: one eval pass per row of the plan table (tests/test_eval_plan.py: T = 8, seeded weights and inputs) through the C ABI.

Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/eval_plan_launches.py`: the per-kernel names and launch counts
say which kernels the rows took, and two builds that select alike give the same list.  Each row also prints a digest of its output.
After the table rows: four passes of stacked networks (hidden_layers = 2) through cvae_gru_rnn_forward_deep, one per recurrence path.

    python tools/eval_plan_launches.py [--root TREE]      TREE: another checkout whose binding and built library to drive
"""
import argparse
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "cyclevae-vc_amd")]
import numpy as np
import torch

from test_eval_plan import TABLE

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT)
pkg = os.path.join(os.path.abspath(ap.parse_args().root), "cyclevae-vc_amd")
spec = importlib.util.spec_from_file_location("_cabi_of_tree", os.path.join(pkg, "_cabi.py"))
cabi = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cabi)
lib = cabi.CvaeLib(os.path.join(pkg, "libcyclevae_hip.so"))
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
Co = 8


def weights(C, H, rng):
    n = lambda sc, *s: torch.from_numpy((sc * rng.standard_normal(s)).astype(np.float32)).to(dev)
    return dict(scale_in_w=n(0.02, C, C, 1) + 0.7 * torch.eye(C, device=dev).reshape(C, C, 1), scale_in_b=n(0.1, C),
                conv0_w=n(0.5 / np.sqrt(3 * C), 3 * C, C, 3), conv0_b=n(0.05, 3 * C), conv1_w=n(0.5 / np.sqrt(9 * C), 9 * C, 3 * C, 3),
                conv1_b=n(0.05, 9 * C), w_ih=n(1 / np.sqrt(9 * C + Co), 3 * H, 9 * C + Co), w_hh=n(1 / np.sqrt(H), 3 * H, H), b_ih=n(0.05, 3 * H),
                b_hh=n(0.05, 3 * H), out_w=n(1 / np.sqrt(H), Co, H, 1), out_b=n(0.05, Co))


images = {}
for i, (C, H, rows, flags, T, opts, form) in enumerate(TABLE):
    lib.reset_options()
    for k, v in opts.items():
        lib.set_option(k, v)
    d = lib.desc(C, Co, H, 3, 2, True, False)
    if (C, H) not in images:
        w = weights(C, H, np.random.default_rng(1000 * H + C))
        prepared = torch.zeros(lib.prepared_bytes(d) // 4, device=dev)
        scratch = torch.zeros(lib.prepare_scratch_bytes(d) // 8 + 1, dtype=torch.float64, device=dev)
        lib.net_prepare(d, {k: v.contiguous().data_ptr() for k, v in w.items()}, prepared.data_ptr(), prepared.numel() * 4, scratch.data_ptr(),
                        scratch.numel() * 8, stream)
        images[(C, H)] = (prepared, w)
    prepared = images[(C, H)][0]
    rng = np.random.default_rng(i)
    x = torch.from_numpy(rng.standard_normal((rows, T, C)).astype(np.float32)).to(dev)
    y = torch.from_numpy((0.3 * rng.standard_normal((rows, Co))).astype(np.float32)).to(dev)
    trj = torch.full((rows, T, Co), float("nan"), device=dev)
    ws = torch.zeros(lib.pass_workspace_bytes(d, rows, T) // 4, device=dev)
    lib.gru_rnn_forward(d, prepared.data_ptr(), lib.pass_input((x.data_ptr(), C, C)), y.data_ptr(), None, rows, T, 4, trj.data_ptr(), None, None,
                        ws.data_ptr(), ws.numel() * 4, flags, stream)
    st = lib.workspace_status(ws.data_ptr(), stream)
    out = trj.cpu().numpy()
    assert st[0] == 0 and np.isfinite(out).all(), (i, st)
    plan = lib.plan_pass(d, rows, T, flags) if hasattr(lib, "plan_pass") else -1
    print("row %2d in=%d H=%d rows=%d flags=%d T=%d %s: table form %d, plan_pass %d, sha256(trj) %s" % (
        i, C, H, rows, flags, T, opts or "", form, plan, hashlib.sha256(out.tobytes()).hexdigest()[:16]), flush=True)

# stacked networks (L GRU layers) through the *_deep entry points: the three recurrence paths at H = 64, the resident one at H = 1024
P_, G_ = cabi.FLAG_PERSISTENT, cabi.FLAG_GENERIC_STEP
lib.reset_options()
for i, (C, H, L, rows, flags, T) in enumerate([(10, 64, 2, 3, P_, 8), (10, 64, 2, 3, P_ | G_, 8), (10, 64, 2, 3, 0, 8), (10, 1024, 2, 4, P_, 8)]):
    d = lib.desc(C, Co, H, 3, 2, True, False)
    if (C, H, L) not in images:
        rng = np.random.default_rng(1000 * H + C + 100000 * L)
        w = weights(C, H, rng)
        n = lambda sc, *s: torch.from_numpy((sc * rng.standard_normal(s)).astype(np.float32)).to(dev)
        upper = [(n(1 / np.sqrt(H), 3 * H, H), n(1 / np.sqrt(H), 3 * H, H), n(0.05, 3 * H), n(0.05, 3 * H)) for _ in range(1, L)]
        prepared = torch.zeros(lib.prepared_bytes_deep(d, L) // 4, device=dev)
        scratch = torch.zeros(lib.prepare_scratch_bytes_deep(d, L) // 8 + 1, dtype=torch.float64, device=dev)
        lib.net_prepare_deep(d, L, {k: v.contiguous().data_ptr() for k, v in w.items()}, [tuple(t.data_ptr() for t in u) for u in upper],
                             prepared.data_ptr(), prepared.numel() * 4, scratch.data_ptr(), scratch.numel() * 8, stream)
        images[(C, H, L)] = (prepared, w, upper)
    prepared = images[(C, H, L)][0]
    rng = np.random.default_rng(500 + i)
    x = torch.from_numpy(rng.standard_normal((rows, T, C)).astype(np.float32)).to(dev)
    y = torch.from_numpy((0.3 * rng.standard_normal((rows, Co))).astype(np.float32)).to(dev)
    trj = torch.full((rows, T, Co), float("nan"), device=dev)
    ws = torch.zeros(lib.pass_workspace_bytes_deep(d, L, rows, T) // 4, device=dev)
    lib.gru_rnn_forward_deep(d, L, prepared.data_ptr(), lib.pass_input((x.data_ptr(), C, C)), y.data_ptr(), None, rows, T, 4, trj.data_ptr(),
                             None, None, ws.data_ptr(), ws.numel() * 4, flags, stream)
    st = lib.workspace_status(ws.data_ptr(), stream)
    out = trj.cpu().numpy()
    assert st[0] == 0 and np.isfinite(out).all(), ("stacked", i, st)
    print("stacked row %d in=%d H=%d L=%d rows=%d flags=%d T=%d: plan_pass_deep %d, sha256(trj) %s" % (
        i, C, H, L, rows, flags, T, lib.plan_pass_deep(d, L, rows, T, flags), hashlib.sha256(out.tobytes()).hexdigest()[:16]), flush=True)
torch.cuda.synchronize()
print("EVAL_PLAN_LAUNCHES_OK")
