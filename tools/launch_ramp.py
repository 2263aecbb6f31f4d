#!/usr/bin/env python
"""GPU-only measuring tool: the FIXED cost of a k_gru_steps_v6 launch (profiles/v6_launch_ramp_notes.md).

    python tools/launch_ramp.py [--fits 5] [--reps 12] [--out FILE.json] [NAME=VALUE ...]      # NAME=VALUE: library options

One hu1024 encoder pass (KFW 8) and one decoder pass (KFW 6) at 64 rows, and the decoder at 128 rows (the geometry of the chain's
stacked decoder pass: two 32-row tiles per block), each at T = 20, 40, 80 and 160 frames, the recurrence launch timed by the library's
own event bracket (CVAE_FLAG_PROFILE, cvae_profile_collect_launches).  Launch time = a + b * T by least squares over the four
lengths: b is the step, a what a launch costs before and after its steps (weight and image loads, the ramp of the first frames, the
drain).  tools/step_timing.py counts inside the task loop only and cannot see a.  The fit is repeated `--fits` times on fresh
measurements (median of `--reps` launches per length each); the spread of a and b over the fits is their scatter.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cyclevae-vc_amd")]
import numpy as np
import torch

import _cabi
import gru_vae
import synth

LENGTHS = (20, 40, 80, 160)
SHAPES = (("encoder 64 rows", "enc", 64), ("decoder 64 rows", "dec", 64), ("decoder 128 rows", "dec", 128))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fits", type=int, default=5)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out")
    ap.add_argument("options", nargs="*", help="NAME=VALUE library options")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = gru_vae._lib()
    for kv in a.options:
        lib.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    P = synth.CycleVAEProblem(B=128, T=max(LENGTHS), bias_scale=0.05, tag="ramp")
    nets = {"enc": gru_vae.GRU_RNN(in_dim=54, out_dim=64, hidden_units=1024, scale_in_flag=True, scale_out_flag=False),
            "dec": gru_vae.GRU_RNN(in_dim=34, out_dim=50, hidden_units=1024, scale_in_flag=False, scale_out_flag=True)}
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(v) for n, v in getattr(P, k).items()})
        nets[k] = m.to(dev).eval()
    dec_x = np.concatenate((P.code_src, P.eps[0, 0]), axis=2).astype(np.float32)
    inp = {"enc": (torch.from_numpy(P.x).to(dev), torch.from_numpy(P.y_in_enc).to(dev), dict(clamp_vae=True, lat_dim=32)),
           "dec": (torch.from_numpy(np.ascontiguousarray(dec_x)).to(dev), torch.from_numpy(P.y_in_dec).to(dev), {})}

    def launch_ms(which, B, T, reps):
        x, y, kw = inp[which]
        x, y = x[:B, :T].contiguous(), y[:B].contiguous()
        with torch.no_grad():
            for _ in range(3):
                nets[which](x, y, **kw)
            torch.cuda.synchronize()
            lib.profile_collect_launches()
            gru_vae._flags_extra = _cabi.FLAG_PROFILE
            try:
                for _ in range(reps):
                    nets[which](x, y, **kw)
                torch.cuda.synchronize()
            finally:
                gru_vae._flags_extra = 0
        ms = [m for m, rows, cin in lib.profile_collect_launches() if rows == B]
        assert len(ms) == reps, (len(ms), reps)
        return float(np.median(ms))

    gru_vae.check_status()
    res = {"lengths": list(LENGTHS), "fits": a.fits, "reps": a.reps, "options": a.options, "shapes": {}}
    for name, which, B in SHAPES:
        fits = []
        for _ in range(a.fits):
            us = [1e3 * launch_ms(which, B, T, a.reps) for T in LENGTHS]
            b, a0 = np.polyfit(np.asarray(LENGTHS, np.float64), np.asarray(us), 1)
            fits.append({"us": us, "a_us": float(a0), "b_us": float(b)})
        aa, bb = [f["a_us"] for f in fits], [f["b_us"] for f in fits]
        res["shapes"][name] = {"fits": fits, "a_us": {"median": float(np.median(aa)), "min": min(aa), "max": max(aa)},
                               "b_us": {"median": float(np.median(bb)), "min": min(bb), "max": max(bb)}}
        print("%-17s a = %7.2f us (%.2f .. %.2f)   b = %6.3f us per frame (%.3f .. %.3f)   launch at T = %s: %s us" %
              (name, np.median(aa), min(aa), max(aa), np.median(bb), min(bb), max(bb), list(LENGTHS),
               ["%.1f" % np.median([f["us"][i] for f in fits]) for i in range(len(LENGTHS))]))
    gru_vae.check_status()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
