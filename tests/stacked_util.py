"""Helpers of the stacked-GRU (hidden_layers >= 2) tests: one prepared deep net in numpy memory on the host-fiber emulator, and the
bounds the project already holds its eval passes to."""
import numpy as np

import _cabi
from emu_util import ptr

# the project's own bounds: tests/test_gpu_parity.py:27-30 (device) and the header of tests/test_emu_library.py (emulator)
TIGHT_PASS = 5e-6
TIGHT_CHAIN = 5e-6
TIGHT_KERNELS = 3e-6
EMU_PASS = 5e-5
EMU_CHAIN = 3e-4

PERSISTENT = _cabi.FLAG_PERSISTENT
GENERIC = _cabi.FLAG_PERSISTENT | _cabi.FLAG_GENERIC_STEP


class NpDeepNet(object):
    """One prepared GRU_RNN with n_layers GRU layers living in numpy memory ("device" == host under emulation)."""

    def __init__(self, lib, sd, in_dim, out_dim, hidden, n_layers, ks=3):
        self.lib, self.L = lib, n_layers
        self.sd = {k: np.ascontiguousarray(v, np.float32) for k, v in sd.items()}
        self.d = lib.desc(in_dim, out_dim, hidden, ks, 2, "scale_in.weight" in sd, "scale_out.weight" in sd)
        self.prepared = np.zeros(lib.prepared_bytes_deep(self.d, n_layers) // 4, np.float32)
        scratch = np.zeros(lib.prepare_scratch_bytes_deep(self.d, n_layers) // 8 + 1, np.float64)
        wp = {f: ptr(self.sd[k]) for f, k in _cabi.STATE_KEYS.items() if k in self.sd}
        upper = [tuple(ptr(self.sd[k]) for k in keys) for keys in _cabi.upper_layer_keys(n_layers)]
        lib.net_prepare_deep(self.d, n_layers, wp, upper, ptr(self.prepared), self.prepared.nbytes, ptr(scratch), scratch.nbytes)

    def forward(self, x, y_in, h_in=None, clamp_lat_dim=-1, flags=PERSISTENT, lat=None, lat_dim=0, eps=None, seg1=None, n_draws=0):
        """x: [B,T,w0] seg0; optional seg1 [B,T,w1] or (lat, eps) sampling.  Returns (trj, y_last [B,1,Co], h [L,B,H])."""
        x = np.ascontiguousarray(x, np.float32)
        B, T = x.shape[:2]
        Co, H, L = self.d.out_dim, self.d.hidden, self.L
        keep = [x]
        s1 = None
        if seg1 is not None:
            seg1 = np.ascontiguousarray(seg1, np.float32)
            keep.append(seg1)
            s1 = (ptr(seg1), seg1.shape[2], seg1.shape[2])
        pin = self.lib.pass_input((ptr(x), x.shape[2], x.shape[2]), s1, ptr(lat), lat_dim, ptr(eps), n_draws=n_draws)
        y_in = np.ascontiguousarray(np.asarray(y_in).reshape(B, Co), np.float32)
        h_in = None if h_in is None else np.ascontiguousarray(np.asarray(h_in).reshape(L, B, H), np.float32)
        trj, yl = np.full((B, T, Co), np.nan, np.float32), np.full((B, Co), np.nan, np.float32)
        hl = np.full((L, B, H), np.nan, np.float32)
        ws = np.zeros(self.lib.pass_workspace_bytes_deep(self.d, L, B, T) // 4, np.float32)
        self.lib.gru_rnn_forward_deep(self.d, L, ptr(self.prepared), pin, ptr(y_in), ptr(h_in), B, T, clamp_lat_dim, ptr(trj),
                                      ptr(yl), ptr(hl), ptr(ws), ws.nbytes, flags)
        assert self.lib.workspace_status(ptr(ws))[0] == 0, "a hand-off spin or grid barrier timed out"
        return trj, yl[:, None, :], hl


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))
