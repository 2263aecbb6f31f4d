"""Shared by tests/golden/make_golden_range.py (the recorder) and the range-guard tests: the out-of-range encoder cases.

A nearly constant feature dimension gives a huge 1/sigma in scale_in = diag(1/sigma) (a StandardScaler on a uv flag, on a coded-
aperiodicity band of one speaker, on another corpus's statistics).  The cases multiply ONE diagonal entry of scale_in.weight by s:
the normalised input of that channel then reaches max|x^| ~ 3e4 (s = 1e4: inside the fp16 range, beyond the 2048 up to which the
(fp16, fp16, bf8) triple is exact) or ~ 3e5 (s = 1e5: beyond the largest finite half)."""
import os

import numpy as np

import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANNEL = 2
SCALES = (("s1e4", 1e4), ("s1e5", 1e5))
# name -> (CycleVAEProblem arguments, file)
CASES = {
    "h64": (dict(B=3, T=20, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="rng64"), "range_h64.npz"),
    "h1024": (dict(B=4, T=40, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, n_cyc=2, bias_scale=0.05, tag="rng1024"), "range_h1024.npz"),
}


def problem(name):
    return synth.CycleVAEProblem(**CASES[name][0])


def scaled_encoder(P, s):
    """The encoder's state dict with scale_in.weight[CHANNEL, CHANNEL] multiplied by s (a copy)."""
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["scale_in.weight"][CHANNEL, CHANNEL, 0] *= np.float32(s)
    return sd


def golden(name):
    return np.load(os.path.join(GOLD, CASES[name][1]))


def allowance(g, key):
    """The yardstick: n = max|ref_fp32 - ref_fp64| is the reference's own rounding noise on this input (recorded as <key>_n); a
    device result must satisfy max|dev - ref_fp64| <= max(5e-6, 4 n)."""
    n = float(g[key + "_n"])
    if key + "_f32" in g.files:
        assert n == float(np.max(np.abs(g[key + "_f32"].astype(np.float64) - g[key + "_f64"])))
    return n, max(5e-6, 4.0 * n)
