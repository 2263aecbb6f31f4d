"""TEST INFRASTRUCTURE: the Python side of the range guard (gru_vae.check_status -> CvaeRangeError, set_range_policy, the image
query of _Prepared, stage6 under "retry") on the host-fiber build of the library, with a status sink in host memory.  Run as a
process of its own by tests/test_range_guard_cpu.py (emu_bench_backend.install() rebinds the module to the emulator for the whole
process); prints RANGE_POLICY_OK."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import emu_bench_backend  # noqa: E402

dev = emu_bench_backend.install()

import torch  # noqa: E402

import _cabi  # noqa: E402
import gru_vae  # noqa: E402
import range_util  # noqa: E402
import stage6  # noqa: E402

sink = torch.zeros(4, dtype=torch.int32)
gru_vae._lib().set_status_sink(sink.data_ptr())
gru_vae._sink = lambda: sink
stage6.gru_vae = gru_vae


def module(sd, i, o, enc):
    m = gru_vae.GRU_RNN(in_dim=i, out_dim=o, hidden_units=64, kernel_size=3, dilation_size=2, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.eval()


P = range_util.problem("h64")
g = range_util.golden("h64")
x = torch.from_numpy(np.concatenate([P.x, P.x]))
y0 = torch.from_numpy(np.concatenate([P.y_in_enc, P.y_in_enc]))
bad, ok = module(range_util.scaled_encoder(P, 1e5), 10, 8, True), module(P.enc, 10, 8, True)
n, tol = range_util.allowance(g, "s1e5")

with torch.no_grad():
    # "raise": the call returns, the check raises the dedicated error once, naming the remedy
    bad(x, y0, clamp_vae=True, lat_dim=4)
    assert list(sink) == [0, 0, 0, _cabi.STATUS_RANGE], list(sink)
    try:
        gru_vae.check_status(sync=True)
        raise SystemExit("no CvaeRangeError")
    except _cabi.CvaeRangeError as e:
        assert "set_kernel" in str(e) and "set_range_policy" in str(e), str(e)
    gru_vae.check_status(sync=True)
    lat_ok = ok(x, y0, clamp_vae=True, lat_dim=4)[0]
    gru_vae.check_status(sync=True)
    assert int(sink[3]) == 0 and bool(torch.isfinite(lat_ok).all())
    # the lagged contract: the next entry point refuses to enqueue
    bad(x, y0, clamp_vae=True, lat_dim=4)
    try:
        ok(x, y0, clamp_vae=True, lat_dim=4)
        raise SystemExit("no CvaeRangeError at the next entry point")
    except _cabi.CvaeRangeError:
        pass
    # a time-out code in word 0 is neither masked by the range word nor masks it
    bad(x, y0, clamp_vae=True, lat_dim=4)
    sink[0] = 2
    try:
        gru_vae.check_status()
        raise SystemExit("no CvaeError")
    except _cabi.CvaeRangeError:
        raise SystemExit("the time-out was masked by the range word")
    except _cabi.CvaeError:
        pass
    try:
        gru_vae.check_status()
        raise SystemExit("the range word was lost with the time-out")
    except _cabi.CvaeRangeError:
        pass
    # "retry": the fp32-operand result, finite, the reference's within its own noise, bit for bit what set_kernel("fp32") gives
    assert gru_vae.set_range_policy("retry") == "raise"
    lat = bad(x, y0, clamp_vae=True, lat_dim=4)[0]
    gru_vae.check_status(sync=True)
    d = float(np.max(np.abs(lat.numpy()[:3].astype(np.float64) - g["s1e5_f64"])))
    assert bool(torch.isfinite(lat).all()) and d <= tol, (d, tol)
    assert torch.equal(ok(x, y0, clamp_vae=True, lat_dim=4)[0], lat_ok)          # in-range calls are what they were
    # stage 6 with that encoder: two pairs = four encoder rows (the exact-operand kernel)
    dec = module(P.dec, 6, 6, False)
    ypp, yd = y0[:1], torch.from_numpy(P.y_in_dec[:1])
    pairs = [(x[0], x[1]), (x[2], x[0])]
    res = stage6.convert_pairs(bad, dec, pairs, ypp, yd, yd, 4, n_smpl_dec=3, seed=11)
    gru_vae.check_status(sync=True)
    assert gru_vae.set_range_policy("raise") == "retry"
    gru_vae.set_kernel("fp32")
    lat32 = bad(x, y0, clamp_vae=True, lat_dim=4)[0]
    res32 = stage6.convert_pairs(bad, dec, pairs, ypp, yd, yd, 4, n_smpl_dec=3, seed=11)
    gru_vae.check_status(sync=True)
    gru_vae.set_kernel("exact3")
    assert torch.equal(lat, lat32)
    for a, b in zip(res, res32):
        for u, v in zip(a, b):
            assert torch.equal(u, v) and bool(torch.isfinite(u).all())
    assert float(np.max(np.abs(res[0][3].numpy().astype(np.float64) - g["s1e5_f64"][0]))) <= tol
    stage6.convert_pairs(bad, dec, pairs, ypp, yd, yd, 4, n_smpl_dec=3, seed=11)
    try:
        gru_vae.check_status(sync=True)
        raise SystemExit("stage 6 under the raise policy: no CvaeRangeError")
    except _cabi.CvaeRangeError:
        pass
    # weights beyond the fp16 range: asked once per image build, fp32-operand kernels from the start, no status under either policy
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["gru.weight_hh_l0"][64 + 7, 3] = 1e5
    heavy = module(sd, 10, 8, True)
    a = heavy(x, y0, clamp_vae=True, lat_dim=4)[0]
    gru_vae.check_status(sync=True)
    assert heavy._prep.in_range is False and ok._prep.in_range is True
    gru_vae.set_kernel("fp32")
    b = heavy(x, y0, clamp_vae=True, lat_dim=4)[0]
    gru_vae.set_kernel("exact3")
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
try:
    gru_vae.set_range_policy("ignore")
    raise SystemExit("a policy that does not exist was accepted")
except ValueError:
    pass
print("RANGE_POLICY_OK")
