"""What every leg of bench.py shares: the algorithmic work figures of SURVEY.md 8(d), the roofline peak, logging, the ONE JSON line and
the output dump (--dump-outputs)."""
import json
import os
import sys

# algorithmic MACs per frame per pass
MAC_ENC, MAC_DEC = 5166220, 4397100
# what the dominant kernel (k_gru_steps_v5 / v4: front-end + recurrence of one pass) computes, in the reference's terms:
# conv0 + conv1 + W_ih[:, :9C].x_conv + W_ih[:, 9C:].y + W_hh.h  (everything of a pass but scale_in, out_1, scale_out)
MAC_KERN_ENC = 26244 + 236196 + 1492992 + 196608 + 3145728
MAC_KERN_DEC = 10404 + 93636 + 940032 + 153600 + 3145728
PEAK_F32_MFMA_TFLOPS = 157.3                                      # MI355X_MICROARCH.md chip table



def log(msg):
    sys.stderr.write("[bench] %s\n" % msg)
    sys.stderr.flush()


def flush_c_stdio():
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()


def emit(res):
    """The ONE JSON line, as the last line of stdout (whatever C libraries still hold in their stdio buffers goes out first)."""
    flush_c_stdio()
    print(json.dumps(res), flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, suffix=""):
    """--dump-outputs: every array of `arrays` ({name: tensor [n_cyc, B, T, C]}) as out_dir/<name><suffix>.npy in float32.  Above 64 MB in
    all, the same fixed, seeded sample of batch rows (axis 1) is written for every array."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    rows = None
    if total > DUMP_LIMIT_BYTES:
        nb = next(iter(host.values())).shape[1]
        keep = max(1, int(nb * DUMP_LIMIT_BYTES // total))
        rows = np.sort(np.random.default_rng(20240).choice(nb, keep, replace=False))
        host = {k: np.ascontiguousarray(a[:, rows]) for k, a in host.items()}
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), a)
    log("outputs of the last timed step -> %s: %s%s" % (out_dir, ", ".join("%s%s" % (k, list(a.shape)) for k, a in host.items()),
                                                          "" if rows is None else " (batch rows %s)" % rows.tolist()))
