"""Stacked GRU networks (hidden_layers >= 2) on the device, through gru_vae -> ctypes -> libcyclevae_hip.so: the goldens recorded from
the reference (tests/golden/make_golden_stacked.py), the 64-row hu1024 pass against the stock-torch fp64 restatement
(tests/stacked_ref.py), row independence, the resident kernel against the any-H path, launch counts.  python -m pytest tests -m gpu

Bounds are the project's own (tests/test_gpu_parity.py:27-30): TIGHT_PASS = TIGHT_CHAIN = 5e-6, TIGHT_KERNELS = 3e-6.
Every measured difference is printed (run with -s to see it) and, when CYCLEVAE_REPORT_DIR names a directory, appended to
stacked_gpu_report.txt there."""
import os

import numpy as np
import pytest

import _cabi
import stacked_ref
import synth
from stacked_util import TIGHT_CHAIN, TIGHT_KERNELS, TIGHT_PASS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("CYCLEVAE_REPORT_DIR")
H64 = dict(B=3, T=20, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1)


def note(msg):
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "stacked_gpu_report.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


def maxabs(a, b, name):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.all(np.isfinite(a)), name + ": non-finite output"
    d = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
    note("%-52s max|d| = %.3e" % (name, d))
    return d


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gv():
    import gru_vae
    return gru_vae


@pytest.fixture
def kernel_path(gv):
    """kernel_path("generic") forces the any-H kernel for the test (the C ABI's CVAE_FLAG_GENERIC_STEP), restored afterwards."""
    def setter(which):
        gv._flags_extra = _cabi.FLAG_GENERIC_STEP if which == "generic" else 0
    yield setter
    gv._flags_extra = 0


def module(gv, sd, i, o, h, layers, enc, dev):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, hidden_layers=layers, kernel_size=3, dilation_size=2, scale_in_flag=enc,
                   scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def finish(gv):
    torch.cuda.synchronize()
    gv.check_status()


@pytest.mark.parametrize("path", ["resident", "generic"])
@pytest.mark.parametrize("L", [2, 3])
def test_h64_passes_vs_golden(gv, dev, golden, kernel_path, L, path):
    """H = 64, L = 2 and 3: 3-D pass with clamp_vae, 2-D pass, two windows with carried (y, h [L,B,H]), on either kernel."""
    kernel_path(path)
    G = golden("stacked_h64")
    P = synth.CycleVAEProblem(tag="stk%d" % L, hidden_layers=L, **H64)
    assert synth.sha256_state(P.enc) == str(G["L%d_sha_enc" % L])
    enc = module(gv, P.enc, 10, 8, 64, L, True, dev)
    x, y0 = T_(P.x, dev), T_(P.y_in_enc, dev)
    with torch.no_grad():
        lat, y, h = enc(x, y0, clamp_vae=True, lat_dim=4)
        lat2d = enc(x[0], y0[:1], clamp_vae=True, lat_dim=4)[0]
        a, ay, ah = enc(x[:, :10], y0, clamp_vae=True, lat_dim=4)
        b, by, bh = enc(x[:, 10:], ay, h_in=ah, clamp_vae=True, lat_dim=4)
    finish(gv)
    assert h.shape == (L, 3, 64) and ah.shape == (L, 3, 64) and lat2d.shape == (20, 8) and y.shape == (3, 1, 8)
    tag = "h64 L%d %s " % (L, path)
    for name, got in (("lat", lat), ("lat_y", y), ("lat_h", h), ("lat2d", lat2d), ("carry_a", a), ("carry_ah", ah), ("carry_b", b),
                      ("carry_by", by), ("carry_bh", bh)):
        assert maxabs(got, G["L%d_%s" % (L, name)], tag + name) <= TIGHT_PASS


def test_h64_chain_vs_golden(gv, dev, golden):
    """cyc2 eval chain with L = 2 encoder and decoder; the carry form is refused."""
    G = golden("stacked_chain")
    P = synth.CycleVAEProblem(tag="stkchain", hidden_layers=2, **H64)
    assert synth.sha256_state(P.enc) == str(G["sha_enc"]) and synth.sha256_state(P.dec) == str(G["sha_dec"])
    enc, dec = module(gv, P.enc, 10, 8, 64, 2, True, dev), module(gv, P.dec, 6, 6, 64, 2, False, dev)
    chain = gv.CycleChain(enc, dec, lat_dim=4, n_cyc=2)
    args = [T_(getattr(P, n), dev) for n in ("x", "cvx", "code_src", "code_trg", "y_in_enc", "y_in_dec")]
    with torch.no_grad():
        out = chain(*args, eps=T_(P.eps, dev))
    finish(gv)
    assert sorted(out) == ["cv", "lat", "latcv", "rec", "reccyc"]
    for k in out:
        assert maxabs(out[k], G[k], "h64 L2 chain " + k) <= TIGHT_CHAIN
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        chain(*args, eps=T_(P.eps, dev), return_state=True)


def stage6_problem(tag, G):
    hidden, in_dim, out_dim, lat_dim, Ts, Tt, nd = [int(v) for v in G["dims"]]
    stdim = in_dim - out_dim
    mu, sg = synth.feature_stats(tag + "/stats", in_dim)
    enc = synth.gru_rnn_state(tag + "/enc", in_dim, 2 * lat_dim, hidden, scale_in=(mu, sg), bias_scale=0.05, hidden_layers=2)
    dec = synth.gru_rnn_state(tag + "/dec", lat_dim + 2, out_dim, hidden, scale_out=(mu[stdim:], sg[stdim:]), bias_scale=0.05,
                              hidden_layers=2)
    assert synth.sha256_state(enc) == str(G["sha_enc"]) and synth.sha256_state(dec) == str(G["sha_dec"])
    fs, ft = synth.features(tag + "/src", 1, Ts, mu, sg)[0], synth.features(tag + "/trg", 1, Tt, mu, sg)[0]
    es, et = synth.normal(tag + "/eps_src", (nd, Ts, lat_dim)), synth.normal(tag + "/eps_trg", (nd, Tt, lat_dim))
    y_pp = np.zeros((1, 1, 2 * lat_dim), np.float32)
    y_dec = ((0.0 - mu[stdim:]) / sg[stdim:]).astype(np.float32)[None, None, :]
    return dict(hidden=hidden, in_dim=in_dim, out_dim=out_dim, lat_dim=lat_dim, nd=nd, enc=enc, dec=dec, fs=fs, ft=ft, es=es, et=et,
                y_pp=y_pp, y_dec=y_dec)


@pytest.mark.parametrize("name,tag", [("stacked_stage6_h64", "stk6"), ("stacked_stage6_h1024", "stk6k")])
def test_stage6_vs_golden(gv, dev, golden, name, tag):
    """A reference-layout hidden_layers = 2 checkpoint converts: the reference's decode statements (decode_gru-cyclevae_gauss.py:
    302-319) on the drop-in modules, and stage6.convert_pair, both against the reference's recorded outputs."""
    import stage6
    G = golden(name)
    Q = stage6_problem(tag, G)
    L, nd = Q["lat_dim"], Q["nd"]
    enc = module(gv, Q["enc"], Q["in_dim"], 2 * L, Q["hidden"], 2, True, dev)
    dec = module(gv, Q["dec"], L + 2, Q["out_dim"], Q["hidden"], 2, False, dev)
    fs, ypp, yd, es = T_(Q["fs"], dev), T_(Q["y_pp"], dev), T_(Q["y_dec"], dev), T_(Q["es"], dev)
    with torch.no_grad():
        lat_src = enc(fs, ypp, clamp_vae=True, lat_dim=L)[0]
        z = torch.mean(gv.sampling_with_eps(lat_src.unsqueeze(0).repeat(nd, 1, 1), es, lat_dim=L), 0)
        trg_code = torch.zeros(fs.shape[0], 2, device=dev)
        trg_code[:, 1] = 1
        cv = dec(torch.cat((trg_code, z), 1), yd)[0]
        res = stage6.convert_pair(enc, dec, fs, T_(Q["ft"], dev), ypp, yd, yd, L, n_smpl_dec=nd, eps_src=es, eps_trg=T_(Q["et"], dev))
    finish(gv)
    assert maxabs(lat_src, G["lat_src"], name + " statements lat_src") <= TIGHT_PASS
    assert maxabs(z, G["z_src"], name + " statements z_src") <= TIGHT_PASS
    assert maxabs(cv, G["cvmcep"], name + " statements cvmcep") <= TIGHT_PASS
    for got, key in zip(res, ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg")):
        assert maxabs(got, G[key], name + " convert_pair " + key) <= TIGHT_PASS
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        stage6.convert_pair(enc, dec, fs, T_(Q["ft"], dev), ypp, yd, yd, L, n_smpl_dec=nd, window=16)


def test_h1024_four_rows_vs_golden(gv, dev, golden):
    """hu1024, L = 2, B = 4, T = 80: encoder and decoder pass on the resident kernel against the reference's outputs."""
    G = golden("stacked_h1024")
    P = synth.CycleVAEProblem(B=4, T=80, bias_scale=0.05, tag="stk1024", hidden_layers=2)
    assert synth.sha256_state(P.enc) == str(G["sha_enc"]) and synth.sha256_state(P.dec) == str(G["sha_dec"])
    enc, dec = module(gv, P.enc, 54, 64, 1024, 2, True, dev), module(gv, P.dec, 34, 50, 1024, 2, False, dev)
    d, _ = enc.prepared(dev)
    assert gv._lib().plan_pass_deep(d, 2, 4, 80, gv._flags()) == _cabi.DEEP_RESIDENT
    with torch.no_grad():
        lat, lat_y, lat_h = enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=32)
        z = gv.sampling_with_eps(lat, T_(P.eps[0, 0], dev), lat_dim=32)
        rec, rec_y, rec_h = dec(torch.cat((T_(P.code_src, dev), z), 2), T_(P.y_in_dec, dev))
    finish(gv)
    assert lat_h.shape == (2, 4, 1024)
    for name, got in (("lat", lat), ("lat_y", lat_y), ("lat_h", lat_h), ("rec", rec), ("rec_y", rec_y), ("rec_h", rec_h)):
        assert maxabs(got, G[name], "h1024 L2 B4 " + name) <= TIGHT_PASS


@pytest.fixture(scope="module")
def headline(gv, dev):
    """hu1024, L = 2 encoder at 64 rows x 80 frames: the module, its inputs and the pass on the resident kernel."""
    P = synth.CycleVAEProblem(B=64, T=80, bias_scale=0.05, tag="stk1024h", hidden_layers=2)
    enc = module(gv, P.enc, 54, 64, 1024, 2, True, dev)
    x, y0 = T_(P.x, dev), T_(P.y_in_enc, dev)
    gv._lib().profile_collect()
    gv._flags_extra = _cabi.FLAG_PROFILE
    try:
        with torch.no_grad():
            out = enc(x, y0, clamp_vae=True, lat_dim=32)
        finish(gv)
        ms, launches = gv._lib().profile_collect()
    finally:
        gv._flags_extra = 0
    return dict(P=P, enc=enc, x=x, y0=y0, out=out, ms=ms, launches=launches)


def test_h1024_64_rows_vs_restatement(gv, dev, headline):
    """All 64 rows (both 32-row tiles) x 80 frames against the stock-torch fp64 restatement; outputs, y_last and h of both layers."""
    P = headline["P"]
    ref = stacked_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)
    for name, got, want in zip(("lat", "y_last", "h"), headline["out"], ref):
        assert maxabs(got, want, "h1024 L2 B64 resident " + name) <= TIGHT_PASS


def test_h1024_resident_is_one_launch(gv, dev, headline):
    d, _ = headline["enc"].prepared(dev)
    assert gv._lib().plan_pass_deep(d, 2, 64, 80, gv._flags()) == _cabi.DEEP_RESIDENT
    note("h1024 L2 B64 T80 resident recurrence: %d launch(es), %.3f ms" % (headline["launches"], headline["ms"]))
    assert headline["launches"] == 1


def test_h1024_rows_independent_of_batch(gv, dev, headline):
    """A row run alone, and a sub-batch, equal the same rows inside the 64-row batch (same kernel, per-row arithmetic)."""
    enc, x, y0, full = headline["enc"], headline["x"], headline["y0"], headline["out"]
    rows = list(range(5, 24)) + [41, 63]
    with torch.no_grad():
        sub = enc(x[rows], y0[rows], clamp_vae=True, lat_dim=32)
        one = enc(x[37:38], y0[37:38], clamp_vae=True, lat_dim=32)
    finish(gv)
    assert torch.equal(full[0][rows], sub[0]) and torch.equal(full[1][rows], sub[1]) and torch.equal(full[2][:, rows], sub[2])
    assert torch.equal(full[0][37:38], one[0]) and torch.equal(full[2][:, 37:38], one[2])


def test_h1024_resident_vs_generic(gv, dev, headline, kernel_path):
    """The resident exact-operand kernel and the any-H path (fp32-input MFMA) on the same operands; the generic path is one
    persistent launch as well at this size (H/4 = 256 blocks)."""
    enc, x, y0, full = headline["enc"], headline["x"], headline["y0"], headline["out"]
    d, _ = enc.prepared(dev)
    kernel_path("generic")
    assert gv._lib().plan_pass_deep(d, 2, 64, 80, gv._flags()) == _cabi.DEEP_GENERIC
    gv._lib().profile_collect()
    gv._flags_extra |= _cabi.FLAG_PROFILE
    with torch.no_grad():
        gen = enc(x, y0, clamp_vae=True, lat_dim=32)
    finish(gv)
    ms, launches = gv._lib().profile_collect()
    note("h1024 L2 B64 T80 generic recurrence: %d launch(es), %.3f ms" % (launches, ms))
    assert launches == 1
    for name, a, b in zip(("lat", "y_last", "h"), full, gen):
        assert maxabs(a, b.cpu().numpy(), "h1024 L2 B64 resident vs generic " + name) <= TIGHT_KERNELS


def test_train_mode_refused(gv, dev):
    """Autograd / dropout passes of a stacked network raise, naming hidden_layers."""
    P = synth.CycleVAEProblem(tag="stk2", hidden_layers=2, **H64)
    enc = module(gv, P.enc, 10, 8, 64, 2, True, dev)
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=4)       # grad enabled, parameters require grad
    import stage4
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        stage4.Stage4Step(enc, module(gv, P.dec, 6, 6, 64, 2, False, dev), lat_dim=4)
