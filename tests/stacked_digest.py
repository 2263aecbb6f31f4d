"""SHA-256 digests of what the library makes of STACKED networks (hidden_layers 2 and 3) on the host-fiber emulator: prepared images
and eval-pass outputs of the H64 problem of tests/test_stacked_cpu.py on each of the three recurrence paths.
tests/golden/stacked_pass_digests.json holds them as recorded from the commit BEFORE the stacked pass was rebuilt from the stages of
the one-layer pass (e75f5a1); tests/test_stacked_cpu.py asks the current library for the same bits.  To record (only ever from that
parent commit):

    cd PARENT_CHECKOUT && python -c "import __graft_entry__ as g; g.build()"
    cp tests/stacked_digest.py /tmp/d.py      # (python puts a script's own directory in front of PYTHONPATH)
    PYTHONPATH=PARENT_CHECKOUT/tests:PARENT_CHECKOUT/cyclevae-vc_amd python /tmp/d.py > tests/golden/stacked_pass_digests.json

Imports nothing newer than that commit (stacked_util.NpDeepNet, synth)."""
import hashlib
import json

import numpy as np

import _cabi
import synth
from emu_util import emu_lib, ptr
from stacked_util import GENERIC, PERSISTENT, NpDeepNet

H64 = dict(B=3, T=20, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1)
PATHS = (("resident", PERSISTENT), ("generic", GENERIC), ("per_step", 0))
N_DRAWS = 3


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def trj_only(lib, net, x, y_in, clamp_lat_dim, flags):
    """A pass with y_last and h_last null (NpDeepNet.forward always asks for both): the fused projection at Cop = 16."""
    x = np.ascontiguousarray(x, np.float32)
    B, T = x.shape[:2]
    y_in = np.ascontiguousarray(np.asarray(y_in).reshape(B, net.d.out_dim), np.float32)
    trj = np.full((B, T, net.d.out_dim), np.nan, np.float32)
    ws = np.zeros(lib.pass_workspace_bytes_deep(net.d, net.L, B, T) // 4, np.float32)
    lib.gru_rnn_forward_deep(net.d, net.L, ptr(net.prepared), lib.pass_input((ptr(x), x.shape[2], x.shape[2])), ptr(y_in), None, B, T,
                             clamp_lat_dim, ptr(trj), None, None, ptr(ws), ws.nbytes, flags)
    assert lib.workspace_status(ptr(ws))[0] == 0, "a hand-off spin or grid barrier timed out"
    return trj


def digests(lib):
    out = {}
    for L in (2, 3):
        P = synth.CycleVAEProblem(tag="stk%d" % L, hidden_layers=L, **H64)
        enc, dec = NpDeepNet(lib, P.enc, 10, 8, 64, L), NpDeepNet(lib, P.dec, 6, 6, 64, L)
        eps1 = synth.normal("stk%d/eps_draws" % L, (N_DRAWS, 20, 4))
        for path, fl in PATHS:
            k = "L%d/%s/" % (L, path)
            out[k + "image_enc"], out[k + "image_dec"] = sha(enc.prepared), sha(dec.prepared)
            lat = enc.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=fl)
            out[k + "enc"] = sha(*lat)
            _, ay, ah = enc.forward(P.x[:, :10], P.y_in_enc, clamp_lat_dim=4, flags=fl)
            out[k + "enc_carried"] = sha(*enc.forward(P.x[:, 10:], ay, h_in=ah, clamp_lat_dim=4, flags=fl))
            out[k + "dec_eps"] = sha(*dec.forward(P.code_src, P.y_in_dec, lat=lat[0], lat_dim=4, eps=np.ascontiguousarray(P.eps[0, 0]),
                                                  flags=fl))
            out[k + "dec_row_draws"] = sha(*dec.forward(P.code_src[:1], P.y_in_dec[:1], lat=np.ascontiguousarray(lat[0][:1]), lat_dim=4,
                                                        eps=eps1, n_draws=N_DRAWS, flags=fl))
            out[k + "enc_trj_only"] = sha(trj_only(lib, enc, P.x, P.y_in_enc, 4, fl))
    return out


if __name__ == "__main__":
    print(json.dumps(digests(emu_lib()), indent=1, sort_keys=True))
