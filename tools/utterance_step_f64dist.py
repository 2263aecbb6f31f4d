#!/usr/bin/env python
"""Writes tests/golden/utterance_step_f64dist.json: for every case of tests/utterance_step_util.py the distance of the stock-torch
checker's fp32 step from its own float64 step, per gradient tensor (max |difference| relative to the tensor's largest entry) and for
the loss (relative).  tests/test_utterance_step_gpu.py derives its gradient bounds from these by the rule of frontend_util.bound_for.
For the two hu64 cases on 2200 frames, whose checker takes ten seconds and more, the fp32 checker's loss and gradients are recorded
as well (tests/golden/utterance_step_<case>.npz, float32 as computed), so the test does not walk them again.  Runs on a CPU; a few minutes (the float64 checker walks 2200 frames of ten passes step by step).

    python tools/utterance_step_f64dist.py [case ...]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "cyclevae-vc_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))

import utterance_step_util as U  # noqa: E402


def main(names):
    out = {}
    if os.path.exists(U.GOLDEN):
        with open(U.GOLDEN) as f:
            out = json.load(f)
    for name in names or sorted(U.CASES):
        t0 = time.time()
        P, items, masks = U.problem(name)
        l32, g32 = U.checker_step(P, items, masks, "float32")
        t1 = time.time()
        l64, g64 = U.checker_step(P, items, masks, "float64")
        out[name] = {"loss": abs(l32 - l64) / abs(l64), "grads": {k: U.distance(g32[k], g64[k]) for k in sorted(g64)}}
        if U.CASES[name]["T"] >= 1000:
            import numpy as np
            np.savez_compressed(U.recorded(name), loss=np.float64(l32), **{k.replace("/", "__"): v.astype(np.float32) for k, v in g32.items()})
        worst = max(out[name]["grads"].items(), key=lambda kv: kv[1])
        print("%-16s loss %.6f (fp32) %.6f (f64) rel %.2e; largest gradient distance %.2e (%s); checker %.1f s fp32, %.1f s f64"
              % (name, l32, l64, out[name]["loss"], worst[1], worst[0], t1 - t0, time.time() - t1), flush=True)
        with open(U.GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
