"""SHA-256 digests of what the library makes of the DEFAULT front-end depth (dilation_size 2) on the host-fiber emulator: prepared
images and eval-pass outputs at the shapes of tests/test_emu_library.py.  tests/golden/frontend_layers2_digests.json holds them as
recorded from the commit BEFORE the front-end fold became an iteration over layers; tests/test_frontend_cpu.py asks the current
library for the same bits.  To record (only ever from that parent commit):

    cd PARENT_CHECKOUT && python -c "import __graft_entry__ as g; g.build()"
    cp tests/frontend_digest.py /tmp/d.py      # (python puts a script's own directory in front of PYTHONPATH)
    PYTHONPATH=PARENT_CHECKOUT/tests:PARENT_CHECKOUT/cyclevae-vc_amd python /tmp/d.py > tests/golden/frontend_layers2_digests.json

Imports nothing newer than that commit (emu_util.NpNet, synth with its default arguments)."""
import hashlib
import json

import numpy as np

import _cabi
import synth
from emu_util import NpNet, emu_lib

CASES = (("tiny", 2, 12, 32), ("stack", 20, 6, 64), ("v6", 8, 8, 64))      # tag, B, T, hidden; in_dim 6, out_dim 4, lat 4
FLAGS = (0, _cabi.FLAG_PERSISTENT, _cabi.FLAG_PERSISTENT | _cabi.FLAG_SPLIT_F16,
         _cabi.FLAG_PERSISTENT | _cabi.FLAG_SPLIT_F16 | _cabi.FLAG_EXACT3)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(lib):
    out = {}
    for tag, B, T, hidden in CASES:
        P = synth.CycleVAEProblem(B=B, T=T, in_dim=6, out_dim=4, lat_dim=4, hidden=hidden, n_cyc=2, bias_scale=0.1, tag=tag)
        enc, dec = NpNet(lib, P.enc, 6, 8, hidden), NpNet(lib, P.dec, 6, 4, hidden)
        out["%s/image_enc" % tag], out["%s/image_dec" % tag] = sha(enc.prepared), sha(dec.prepared)
        for fl in FLAGS:
            lat = enc.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=fl)
            rec = dec.forward(P.code_src, P.y_in_dec, lat=lat[0], lat_dim=4, eps=np.ascontiguousarray(P.eps[0, 0]), flags=fl)
            out["%s/pass_enc/flags%d" % (tag, fl)], out["%s/pass_dec/flags%d" % (tag, fl)] = sha(*lat), sha(*rec)
    return out


if __name__ == "__main__":
    print(json.dumps(digests(emu_lib()), indent=1, sort_keys=True))
