"""Helpers of the front-end depth tests (dilation_size 1 / 3, kernel_size 5): the shapes the goldens were recorded at
(tests/golden/make_golden_frontend.py), one prepared net of any depth in numpy memory on the host-fiber emulator, and the bound rule.

Bounds.  The project's own (tests/stacked_util.py): 5e-6 per pass and per chain trajectory and 3e-6 kernel against kernel on the
device, 5e-5 / 3e-4 on the emulator.  A 27-tap front-end sums three times the terms of the 9-tap one, so the golden files carry,
per recorded output, the distance of the reference's fp32 pass from its own fp64 pass (`<key>_f64dist`); where that exceeds 1.25e-6
the bound of that output is four times the distance (bound_for).  On the recorded fixtures the largest distance is 5.2e-7, so every
output is held to the project's bound unchanged (profiles/frontend_depth_notes.md lists them)."""
import numpy as np

import _cabi
import synth
from emu_util import NpNet, ptr
from stacked_util import EMU_CHAIN, EMU_PASS, TIGHT_CHAIN, TIGHT_KERNELS, TIGHT_PASS, maxdiff  # noqa: F401

H64 = dict(B=5, T=12, in_dim=30, out_dim=26, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1)
DEPTHS_H64 = ((3, 1), (3, 3), (5, 2))
DEPTHS_H1024 = ((3, 1), (3, 3))
P_, G_, HST, S_, E_ = (_cabi.FLAG_PERSISTENT, _cabi.FLAG_GENERIC_STEP, _cabi.FLAG_HOISTED_FRONTEND, _cabi.FLAG_SPLIT_F16,
                       _cabi.FLAG_EXACT3)
DEFAULT = P_ | E_ | S_          # what gru_vae passes by default


def problem_h64(ks, ds):
    return synth.CycleVAEProblem(tag="fe%d%d" % (ks, ds), dilation_size=ds, kernel_size=ks, **H64)


def problem_h1024(ks, ds, B=4, T=12):
    return synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="fe1024_%d%d" % (ks, ds), dilation_size=ds, kernel_size=ks)


def bound_for(G, key, base):
    """The bound of one recorded output: `base`, or four times the reference's own fp32-vs-fp64 distance where that exceeds 1.25e-6."""
    d = float(G[key + "_f64dist"]) if key + "_f64dist" in G.files else 0.0
    return max(base, 4.0 * d) if d > 1.25e-6 else base


class NpFrontNet(NpNet):
    """NpNet (tests/emu_util.py) with the front-end's depth and kernel size in the descriptor."""

    def __init__(self, lib, sd, in_dim, out_dim, hidden, ks, ds):
        self.lib = lib
        self.sd = {k: np.ascontiguousarray(v, np.float32) for k, v in sd.items()}
        self.d = lib.desc(in_dim, out_dim, hidden, ks, ds, "scale_in.weight" in sd, "scale_out.weight" in sd)
        self.prepared = np.zeros(lib.prepared_bytes(self.d) // 4, np.float32)
        scratch = np.zeros(lib.prepare_scratch_bytes(self.d) // 8 + 1, np.float64)
        wp = {f: ptr(self.sd[k]) for f, k in _cabi.STATE_KEYS.items() if k in self.sd}
        lib.net_prepare(self.d, wp, ptr(self.prepared), self.prepared.nbytes, ptr(scratch), scratch.nbytes)
