"""The range guard of the exact-operand eval kernels on the device, through gru_vae -> ctypes -> libcyclevae_hip.so: status 7
(CvaeRangeError), the "raise" and "retry" policies, images whose weights leave the fp16 range, the stacked path, and that in-range
work is untouched.  python -m pytest tests -m gpu

Ordinary inputs only.  A pass of the limb kernels on an inf operand runs to its end like any other: the flags, tags and spin bounds
of the hand-off do not depend on the data.  The out-of-range fixtures come from the reference itself
(tests/golden/make_golden_range.py); a device result must satisfy max|dev - ref_fp64| <= max(5e-6, 4 n), n = the reference's own
fp32-vs-fp64 distance on that input (range_util.allowance).  Every measured figure is printed (-s) and, when CYCLEVAE_REPORT_DIR
names a directory, appended to range_gpu_report.txt there."""
import os

import numpy as np
import pytest

import _cabi
import range_util
import stacked_ref
import synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("CYCLEVAE_REPORT_DIR")


def note(msg):
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "range_gpu_report.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


def dist(a, b, name, tol, n=None):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    assert a.shape == np.asarray(b).shape, (name, a.shape, np.asarray(b).shape)
    assert np.all(np.isfinite(a)), name + ": non-finite output"
    d = float(np.max(np.abs(a.astype(np.float64) - np.asarray(b, np.float64))))
    note("%-58s max|dev - ref64| = %.3e  (allowed %.3e%s)" % (name, d, tol, "" if n is None else ", n = %.3e" % n))
    assert d <= tol, (name, d, tol)
    return d


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def gv():
    """gru_vae with the default kernel, policy and flags, whatever the test leaves behind."""
    import gru_vae
    yield gru_vae
    gru_vae.set_range_policy("raise")
    gru_vae.set_kernel("exact3")
    gru_vae._flags_extra = 0
    gru_vae._lib().reset_options()
    torch.cuda.synchronize()
    sink = gru_vae._sink()
    if sink is not None:
        sink.zero_()


def module(gv, sd, i, o, h, enc, dev, layers=1):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, hidden_layers=layers, kernel_size=3, dilation_size=2, scale_in_flag=enc,
                   scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def encoder_case(gv, dev, s):
    P = range_util.problem("h1024")
    g = range_util.golden("h1024")
    assert synth.sha256_state(P.enc) == str(g["sha_enc"])
    enc = module(gv, range_util.scaled_encoder(P, s), 54, 64, 1024, True, dev)
    return P, g, enc, T_(P.x, dev), T_(P.y_in_enc, dev)


def test_out_of_range_input_raises_at_the_next_check(gv, dev):
    """hu1024 encoder, scale_in[2,2] x 1e5 (max|x^| = 3.4e5), policy "raise": the forward returns, the check raises CvaeRangeError,
    the next in-range call is clean.  Fails without the guard (NaN / inf with a clean status)."""
    P, g, enc, x, y0 = encoder_case(gv, dev, 1e5)
    with torch.no_grad():
        lat = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    with pytest.raises(_cabi.CvaeRangeError) as e:
        gv.check_status(sync=True)
    assert "set_kernel" in str(e.value) and "retry" in str(e.value)
    note("hu1024 s1e5 on the limb kernels: %d of %d outputs finite (status 7 raised)" % (int(torch.isfinite(lat).sum()), lat.numel()))
    gv.check_status(sync=True)                       # cleared by the raise
    ok = module(gv, P.enc, 54, 64, 1024, True, dev)
    with torch.no_grad():
        lat = ok(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)
    r64 = stacked_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)[0]
    dist(lat, r64, "hu1024 s = 1 exact kernels (stock-torch fp64)", 5e-6)
    # the lagged form: nobody checks, the NEXT entry point refuses to enqueue on top of invalid results
    with torch.no_grad():
        enc(x, y0, clamp_vae=True, lat_dim=32)
        torch.cuda.synchronize()
        with pytest.raises(_cabi.CvaeRangeError):
            ok(x, y0, clamp_vae=True, lat_dim=32)


def test_retry_policy_returns_the_fp32_result(gv, dev):
    P, g, enc, x, y0 = encoder_case(gv, dev, 1e5)
    assert gv.set_range_policy("retry") == "raise"
    with torch.no_grad():
        lat = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)
    n, tol = range_util.allowance(g, "s1e5")
    dist(lat, g["s1e5_f64"], "hu1024 s1e5 retry (fp32 kernels)", tol, n)
    assert gv.set_range_policy("raise") == "retry"
    gv.set_kernel("fp32")
    with torch.no_grad():
        lat32 = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)
    gv.set_kernel("exact3")
    assert torch.equal(lat, lat32)


def test_retry_policy_in_stage6_conversion(gv, dev):
    """Two utterance pairs (four encoder rows: the exact-operand kernel) with the out-of-range encoder: "retry" hands back what
    set_kernel("fp32") computes, and the latents are the reference's.  One pair alone (two rows: k_gru_steps_ll, no limb operand)
    needs no retry and raises nothing."""
    import stage6
    P, g, enc, x, y0 = encoder_case(gv, dev, 1e5)
    dec = module(gv, P.dec, 34, 50, 1024, False, dev)
    ypp, yd = y0[:1], T_(P.y_in_dec[:1], dev)
    pairs = [(x[0], x[1]), (x[2], x[3])]
    n, tol = range_util.allowance(g, "s1e5")
    with torch.no_grad():
        gv.set_range_policy("retry")
        res = stage6.convert_pairs(enc, dec, pairs, ypp, yd, yd, 32, n_smpl_dec=3, seed=11)
        gv.check_status(sync=True)
        gv.set_range_policy("raise")
        gv.set_kernel("fp32")
        res32 = stage6.convert_pairs(enc, dec, pairs, ypp, yd, yd, 32, n_smpl_dec=3, seed=11)
        gv.check_status(sync=True)
        gv.set_kernel("exact3")
        for q, (a, b) in enumerate(zip(res, res32)):
            for u, v in zip(a, b):
                assert torch.equal(u, v) and bool(torch.isfinite(u).all())
            dist(a[3], g["s1e5_f64"][2 * q], "stage6 pair %d lat_src (retry)" % q, tol, n)
            dist(a[4], g["s1e5_f64"][2 * q + 1], "stage6 pair %d lat_trg (retry)" % q, tol, n)
        one = stage6.convert_pair(enc, dec, x[0], x[1], ypp, yd, yd, 32, n_smpl_dec=3, seed=11)
        gv.check_status(sync=True)
        dist(one[3], g["s1e5_f64"][0], "stage6 one pair lat_src (k_gru_steps_ll)", tol, n)
        # and under "raise" the two-pair call is reported
        stage6.convert_pairs(enc, dec, pairs, ypp, yd, yd, 32, n_smpl_dec=3, seed=11)
        with pytest.raises(_cabi.CvaeRangeError):
            gv.check_status(sync=True)


def test_band_below_the_bound_is_carried(gv, dev):
    """scale_in[2,2] x 1e4 (max|x^| = 3.4e4, between 2048 and the largest half) at the default bound: no status, and the limb
    kernels meet the reference within its own noise; exact_range_at = 2048 reports the same pass."""
    P, g, enc, x, y0 = encoder_case(gv, dev, 1e4)
    with torch.no_grad():
        lat = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)
    n, tol = range_util.allowance(g, "s1e4")
    dist(lat, g["s1e4_f64"], "hu1024 s1e4 exact kernels (default bound)", tol, n)
    gv._lib().set_option("exact_range_at", 2048)
    with torch.no_grad():
        lat2 = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    with pytest.raises(_cabi.CvaeRangeError):
        gv.check_status(sync=True)
    assert torch.equal(lat, lat2)


def test_weight_beyond_the_fp16_range_runs_the_fp32_kernels(gv, dev):
    P = range_util.problem("h1024")
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["gru.weight_hh_l0"][1024 + 7, 3] = 1e5
    enc = module(gv, sd, 54, 64, 1024, True, dev)
    x, y0 = T_(P.x, dev), T_(P.y_in_enc, dev)
    with torch.no_grad():
        lat = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)                       # no status under the default policy: the image was asked once, at its build
    assert enc._prep.in_range is False
    gv.set_kernel("fp32")
    with torch.no_grad():
        lat32 = enc(x, y0, clamp_vae=True, lat_dim=32)[0]
    gv.check_status(sync=True)
    gv.set_kernel("exact3")
    assert torch.equal(lat, lat32)
    r64 = stacked_ref.forward(sd, P.x, P.y_in_enc, clamp_lat_dim=32)[0]
    r32 = stacked_ref.forward(sd, P.x, P.y_in_enc, clamp_lat_dim=32, dtype=torch.float32)[0]
    n = float(np.max(np.abs(r32.astype(np.float64) - r64)))
    dist(lat, r64, "hu1024 W_hh entry 1e5 (fp32 kernels by themselves)", max(5e-6, 4 * n), n)


@pytest.mark.parametrize("H,B,T", [(64, 3, 12), (1024, 4, 10)])
def test_stacked_network_carried_in_state(gv, dev, H, B, T):
    """hidden_layers = 2 with an h_in entry beyond the bound: raised by the slot-0 fill of the resident kernel; "retry" hands back
    the any-H kernel's result (k_gru_steps_deep, fp32 operands)."""
    dims = dict(in_dim=10, out_dim=6, lat_dim=4) if H == 64 else dict(in_dim=54, out_dim=50, lat_dim=32)
    P = synth.CycleVAEProblem(B=B, T=T, hidden=H, n_cyc=2, bias_scale=0.05, tag="rngstk%d" % H, hidden_layers=2, **dims)
    L = P.lat_dim
    enc = module(gv, P.enc, P.in_dim, 2 * L, H, True, dev, layers=2)
    x, y0 = T_(P.x, dev), T_(P.y_in_enc, dev)
    h = (0.5 * synth.normal("rngstk%d/h_in" % H, (2, B, H))).astype(np.float32)
    h[0, 1, 9] = -1e5
    hd = T_(h, dev)
    with torch.no_grad():
        enc(x, y0, h_in=hd, clamp_vae=True, lat_dim=L)
        with pytest.raises(_cabi.CvaeRangeError):
            gv.check_status(sync=True)
        gv.set_range_policy("retry")
        lat = enc(x, y0, h_in=hd, clamp_vae=True, lat_dim=L)[0]
        gv.check_status(sync=True)
        gv.set_range_policy("raise")
        gv._flags_extra = _cabi.FLAG_GENERIC_STEP
        lat_g = enc(x, y0, h_in=hd, clamp_vae=True, lat_dim=L)[0]
        gv.check_status(sync=True)
        gv._flags_extra = 0
    assert torch.equal(lat, lat_g)
    r64 = stacked_ref.forward(P.enc, P.x, P.y_in_enc, h, clamp_lat_dim=L)[0]
    r32 = stacked_ref.forward(P.enc, P.x, P.y_in_enc, h, clamp_lat_dim=L, dtype=torch.float32)[0]
    n = float(np.max(np.abs(r32.astype(np.float64) - r64)))
    dist(lat, r64, "stacked H=%d h_in = -1e5 (retry, any-H kernel)" % H, max(5e-6, 4 * n), n)


def test_headline_chain_is_untouched_by_either_policy(gv, dev):
    """In-range headline geometry (B = 64, T = 80, cyc2): no status under either policy and the same bits."""
    P = synth.CycleVAEProblem(B=64, T=80, bias_scale=0.05, tag="rnghead")
    enc, dec = module(gv, P.enc, 54, 64, 1024, True, dev), module(gv, P.dec, 34, 50, 1024, False, dev)
    chain = gv.CycleChain(enc, dec, lat_dim=32, n_cyc=2)
    args = [T_(getattr(P, k), dev) for k in ("x", "cvx", "code_src", "code_trg", "y_in_enc", "y_in_dec")]
    eps = T_(P.eps, dev)
    outs = {}
    for policy in ("raise", "retry"):
        gv.set_range_policy(policy)
        with torch.no_grad():
            outs[policy] = chain(*args, eps=eps)
        st = chain.status()
        assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == 0, (policy, st)
        gv.check_status()
    for k in outs["raise"]:
        assert torch.equal(outs["raise"][k], outs["retry"][k]), k
        assert bool(torch.isfinite(outs["raise"][k]).all()), k


def test_limb_window_on_the_device(gv, dev):
    """cvae_selftest_limbs over binades on the device: bit for bit the host build's answer (tests/test_range_guard_cpu.py holds
    that to the figures of DESIGN.md 4.1), exact below 2048, at most 2^-23 relative in [2048, 65504), non-finite from 65520."""
    from emu_util import emu_lib, ptr
    rng = np.random.default_rng(20190721)
    xs = []
    for b in range(-14, 16):
        x = rng.uniform(2.0 ** b, 2.0 ** (b + 1), 40000).astype(np.float32)
        xs.append(x * rng.choice(np.float32([-1, 1]), x.size))
    xs.append(np.float32([65504, 65519.99, 65520, 65536, 1e5, -65520, np.inf, 3e38]))
    x = np.concatenate(xs)
    y_host = np.zeros_like(x)
    emu_lib().selftest_limbs(ptr(x), ptr(y_host), x.size)
    xd = T_(x, dev)
    yd = torch.empty_like(xd)
    gv._lib().selftest_limbs(xd.data_ptr(), yd.data_ptr(), x.size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert np.array_equal(y.view(np.uint32)[np.isfinite(y)], y_host.view(np.uint32)[np.isfinite(y)])
    assert np.array_equal(np.isfinite(y), np.isfinite(y_host))
    a = np.abs(x)
    assert np.array_equal(y[a < 2048], x[a < 2048])
    band = (a >= 2048) & (a < 65504)
    rel = np.abs((y[band].astype(np.float64) - x[band]) / x[band])
    note("device limb self-test: worst relative error in [2048, 65504) = %.4g, inexact fraction %.3f; exact below 2048: True"
         % (rel.max(), float((rel > 0).mean())))
    assert 0.0 < rel.max() <= 2.0 ** -23
    assert not np.isfinite(y[a >= 65520]).any() and np.isfinite(y[a < 65520]).all()
