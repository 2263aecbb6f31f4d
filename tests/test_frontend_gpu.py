"""Conv front-ends of depth 1 and 3 (reference dilation_size) on the device, through gru_vae -> ctypes -> libcyclevae_hip.so: the
goldens recorded from the reference (tests/golden/make_golden_frontend.py), the hoisted exact-operand kernel (form V6H) at hu1024
against the stock-torch fp64 restatement (tests/frontend_ref.py) at three row counts, row independence, launch counts, V6H against
V2, the fused instances of the one-layer front-end, chain and stage-6 conversion.  python -m pytest tests -m gpu

Bounds are the project's own (tests/stacked_util.py): 5e-6 per pass and per chain trajectory, 3e-6 kernel against kernel; per
recorded output through frontend_util.bound_for (the reference's own fp32-vs-fp64 distance stays below 1.25e-6 on every fixture, so
the bounds are the project's unchanged).  Every measured difference is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a
directory, appended to frontend_gpu_report.txt there."""
import os

import numpy as np
import pytest

import _cabi
import frontend_ref
import synth
from frontend_util import (DEFAULT, DEPTHS_H1024, H64, HST, TIGHT_CHAIN, TIGHT_KERNELS, TIGHT_PASS, bound_for, problem_h64,
                           problem_h1024)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("CYCLEVAE_REPORT_DIR")
V2, V6, V6H = _cabi.EVAL_V2, _cabi.EVAL_V6, _cabi.EVAL_V6H


def note(msg):
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "frontend_gpu_report.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


def maxabs(a, b, name):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.all(np.isfinite(a)), name + ": non-finite output"
    d = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
    note("%-60s max|d| = %.3e" % (name, d))
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
def extra_flags(gv):
    """extra_flags(bits): OR flags of the C ABI into every pass of the test (HOISTED_FRONTEND, PROFILE), restored afterwards."""
    def setter(bits):
        gv._flags_extra = bits
    yield setter
    gv._flags_extra = 0


def module(gv, sd, i, o, h, ks, ds, enc, dev):
    m = gv.GRU_RNN(in_dim=i, out_dim=o, hidden_units=h, kernel_size=ks, dilation_size=ds, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def finish(gv):
    torch.cuda.synchronize()
    gv.check_status()


def plan(gv, mod, dev, rows, T):
    return gv._lib().plan_pass(mod.prepared(dev)[0], rows, T, gv._flags())


@pytest.mark.parametrize("ks,ds", DEPTHS_H1024)
def test_h1024_passes_vs_golden(gv, dev, golden, ks, ds):
    """hu1024, B = 4, T = 12: encoder 54 -> 64 and decoder 34 -> 50 against the reference's outputs; (3, 1) on the fused instances
    k_gru_steps_v6<16, 3> / <16, 2>, (3, 3) on the hoisted kernel."""
    G, pre = golden("frontend_h1024"), "k%dd%d_" % (ks, ds)
    P = problem_h1024(ks, ds)
    assert synth.sha256_state(P.enc) == str(G[pre + "sha_enc"]) and synth.sha256_state(P.dec) == str(G[pre + "sha_dec"])
    enc, dec = module(gv, P.enc, 54, 64, 1024, ks, ds, True, dev), module(gv, P.dec, 34, 50, 1024, ks, ds, False, dev)
    want = V6 if ds == 1 else V6H
    assert plan(gv, enc, dev, 4, 12) == want and plan(gv, dec, dev, 4, 12) == want
    with torch.no_grad():
        lat, lat_y, lat_h = enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=32)
        z = gv.sampling_with_eps(T_(G[pre + "lat"], dev), T_(P.eps[0, 0], dev), lat_dim=32)
        rec, rec_y, rec_h = dec(torch.cat((T_(P.code_src, dev), z), 2), T_(P.y_in_dec, dev))
    finish(gv)
    for name, got in (("lat", lat), ("lat_y", lat_y), ("lat_h", lat_h), ("rec", rec), ("rec_y", rec_y), ("rec_h", rec_h)):
        assert maxabs(got, G[pre + name], "h1024 ks%d ds%d B4 %s" % (ks, ds, name)) <= bound_for(G, pre + name, TIGHT_PASS)


@pytest.fixture(scope="module")
def wide(gv, dev):
    """hu1024, dilation_size 3, encoder: the module, 160 rows of input and the fp64 restatement of the rows the tests compare
    (computed once: the 27-tap conv stack of 160 rows is the slow part on a CPU)."""
    P = problem_h1024(3, 3, B=160, T=12)
    enc = module(gv, P.enc, 54, 64, 1024, 3, 3, True, dev)
    h0 = (0.5 * synth.normal("fe1024_33/h_in", (160, 1024))).astype(np.float32)
    # rows are independent recurrences: the restatement runs a sample of rows from every 32-row tile, edges included
    r12 = sorted(set(range(0, 64, 3)) | {31, 32, 63})
    r6 = sorted(set(range(0, 160, 11)) | {31, 32, 63, 64, 95, 96, 127, 128, 159})
    ref12 = frontend_ref.forward(P.enc, P.x[r12], P.y_in_enc[r12], h_in=h0[None, r12], clamp_lat_dim=32)
    ref6 = frontend_ref.forward(P.enc, P.x[r6, :6], P.y_in_enc[r6], clamp_lat_dim=32)
    return dict(P=P, enc=enc, x=T_(P.x, dev), y0=T_(P.y_in_enc, dev), h0=T_(h0[None], dev), r12=r12, ref12=ref12, r6=r6, ref6=ref6)


def run_profiled(gv, extra_flags, fn, more=0):
    gv._lib().profile_collect()
    extra_flags(_cabi.FLAG_PROFILE | more)
    with torch.no_grad():
        out = fn()
    finish(gv)
    ms, launches = gv._lib().profile_collect()
    extra_flags(0)
    return out, ms, launches


@pytest.mark.parametrize("rows,T", [(33, 12), (64, 12)])
def test_v6h_h1024_vs_restatement(gv, dev, wide, extra_flags, rows, T):
    """33 rows (two tiles, the second ragged) and 64 rows, T = 12, with a carried-in state: outputs, y_last and h against the fp64
    restatement; one launch of the recurrence."""
    enc = wide["enc"]
    assert plan(gv, enc, dev, rows, T) == V6H
    out, ms, launches = run_profiled(gv, extra_flags, lambda: enc(wide["x"][:rows], wide["y0"][:rows], h_in=wide["h0"][:, :rows],
                                                                   clamp_vae=True, lat_dim=32))
    note("h1024 ds3 V6H %d rows T%d: %d launch(es), %.3f ms" % (rows, T, launches, ms))
    assert launches == 1
    keep = [i for i, r in enumerate(wide["r12"]) if r < rows]
    sel = [wide["r12"][i] for i in keep]
    for name, got, want in zip(("lat", "y_last", "h"), out, wide["ref12"]):
        got, want = (got[:, sel], want[:, keep]) if name == "h" else (got[sel], want[keep])
        assert maxabs(got, want, "h1024 ds3 V6H %d rows %s" % (rows, name)) <= TIGHT_PASS


def test_v6h_h1024_160_rows_three_tiles_per_block(gv, dev, wide, extra_flags):
    """160 rows = five 32-row tiles on 256 CUs: two sets of 128 octet blocks, three tiles per block in one set (the path that
    re-reads its own state from the exchange buffer) and two in the other.  T = 6, fresh state, against the fp64 restatement; row independence
    across tiles."""
    enc, x, y0 = wide["enc"], wide["x"][:, :6].contiguous(), wide["y0"]
    assert plan(gv, enc, dev, 160, 6) == V6H
    out, ms, launches = run_profiled(gv, extra_flags, lambda: enc(x, y0, clamp_vae=True, lat_dim=32))
    note("h1024 ds3 V6H 160 rows T6: %d launch(es), %.3f ms" % (launches, ms))
    assert launches == 1
    for name, got, want in zip(("lat", "y_last", "h"), out, wide["ref6"]):
        got = got[:, wide["r6"]] if name == "h" else got[wide["r6"]]
        assert maxabs(got, want, "h1024 ds3 V6H 160 rows %s" % name) <= TIGHT_PASS
    # Row independence.  Tiles 1 and 3 share their blocks two by two: the state stays in a register, as in a pass of one tile --
    # the same bits.  Tiles 0, 2, 4 (three per block) re-read their state from the limb triples, which carry |h| < 2^-16 to an
    # absolute 2^-40: such a difference can move a rounding of a later value by an ulp, so those rows are held to
    # the kernel-against-kernel bound, not to equal bits.
    same, near = [32, 40, 63, 96, 127], [0, 31, 64, 70, 95, 128, 159]
    with torch.no_grad():
        sub = enc(x[same], y0[same], clamp_vae=True, lat_dim=32)
        sub3 = enc(x[near], y0[near], clamp_vae=True, lat_dim=32)
        one = enc(x[37:38], y0[37:38], clamp_vae=True, lat_dim=32)          # (one row: the word-exchange kernel, another arithmetic)
    finish(gv)
    assert torch.equal(out[0][same], sub[0]) and torch.equal(out[1][same], sub[1]) and torch.equal(out[2][:, same], sub[2])
    assert maxabs(sub3[0], out[0][near], "h1024 ds3 rows of three-tile blocks alone vs in the 160-row pass") <= TIGHT_KERNELS
    assert maxabs(one[0], out[0][37:38], "h1024 ds3 one row (LL) vs the 160-row pass") <= TIGHT_KERNELS


def test_v6h_vs_v2_h1024(gv, dev, wide, extra_flags):
    """The same 64-row pass forced onto k_gru_steps_v2 by CVAE_FLAG_HOISTED_FRONTEND: kernel against kernel."""
    enc = wide["enc"]
    f = lambda: enc(wide["x"][:64], wide["y0"][:64], h_in=wide["h0"][:, :64], clamp_vae=True, lat_dim=32)
    a, ms_a, la = run_profiled(gv, extra_flags, f)
    extra_flags(HST)
    assert plan(gv, enc, dev, 64, 12) == V2
    b, ms_b, lb = run_profiled(gv, extra_flags, f, more=HST)
    note("h1024 ds3 64 rows T12 recurrence + GEMM bracket: V6H %.3f ms, V2 %.3f ms" % (ms_a, ms_b))
    assert la == 1 and lb == 1
    for name, u, v in zip(("lat", "y_last", "h"), a, b):
        assert maxabs(u, v, "h1024 ds3 V6H vs V2 " + name) <= TIGHT_KERNELS


def test_v6h_h2048_vs_restatement(gv, dev):
    """k_gru_steps_v6<32, 0, 3, true> (third weight limb streamed): 33 rows, T = 6 at H = 2048 against the fp64 restatement."""
    P = synth.CycleVAEProblem(B=33, T=6, hidden=2048, bias_scale=0.05, tag="fe2048_33", dilation_size=3)
    enc = module(gv, P.enc, 54, 64, 2048, 3, 3, True, dev)
    assert plan(gv, enc, dev, 33, 6) == V6H
    with torch.no_grad():
        out = enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=32)
    finish(gv)
    ref = frontend_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)
    for name, got, want in zip(("lat", "y_last", "h"), out, ref):
        assert maxabs(got, want, "h2048 ds3 V6H 33 rows " + name) <= TIGHT_PASS


@pytest.mark.parametrize("rows", [4, 64])
def test_fused_instances_of_the_one_layer_front_end(gv, dev, rows):
    """k_gru_steps_v6<16, 3> (encoder, in_dim 54) and <16, 2> (decoder, in_dim 34) at dilation_size 1: 4 rows (a half-empty tile)
    and 64 rows, T = 12, against the fp64 restatement."""
    P = problem_h1024(3, 1, B=rows, T=12)
    enc, dec = module(gv, P.enc, 54, 64, 1024, 3, 1, True, dev), module(gv, P.dec, 34, 50, 1024, 3, 1, False, dev)
    assert plan(gv, enc, dev, rows, 12) == V6 and plan(gv, dec, dev, rows, 12) == V6
    xd = np.concatenate([P.code_src, synth.normal("fe1024_31/z", (rows, 12, 32))], 2)
    with torch.no_grad():
        lat = enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=32)
        rec = dec(T_(xd, dev), T_(P.y_in_dec, dev))
    finish(gv)
    for tag, got, ref in (("enc <16,3>", lat, frontend_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)),
                          ("dec <16,2>", rec, frontend_ref.forward(P.dec, xd, P.y_in_dec))):
        for name, u, v in zip(("trj", "y_last", "h"), got, ref):
            assert maxabs(u, v, "h1024 ds1 %s %d rows %s" % (tag, rows, name)) <= TIGHT_PASS


@pytest.mark.parametrize("ks,ds", [(3, 1), (3, 3), (5, 2)])
def test_h64_passes_vs_golden(gv, dev, golden, ks, ds):
    """H = 64: 3-D pass with clamp_vae, 2-D pass, two windows with carried (y, h), decoder pass, against frontend_h64.npz."""
    G, pre = golden("frontend_h64"), "k%dd%d_" % (ks, ds)
    P = problem_h64(ks, ds)
    enc, dec = module(gv, P.enc, 30, 8, 64, ks, ds, True, dev), module(gv, P.dec, 6, 26, 64, ks, ds, False, dev)
    assert plan(gv, enc, dev, 5, 12) == (V6 if ds == 1 else V6H)
    x, y0 = T_(P.x, dev), T_(P.y_in_enc, dev)
    with torch.no_grad():
        lat, y, h = enc(x, y0, clamp_vae=True, lat_dim=4)
        lat2d = enc(x[0], y0[:1], clamp_vae=True, lat_dim=4)[0]
        a, ay, ah = enc(x[:, :6], y0, clamp_vae=True, lat_dim=4)
        b, by, bh = enc(x[:, 6:], ay, h_in=ah, clamp_vae=True, lat_dim=4)
        z = gv.sampling_with_eps(T_(G[pre + "lat"], dev), T_(P.eps[0, 0], dev), lat_dim=4)
        rec, ry, rh = dec(torch.cat((T_(P.code_src, dev), z), 2), T_(P.y_in_dec, dev))
    finish(gv)
    assert lat2d.shape == (12, 8) and h.shape == (1, 5, 64)
    for name, got in (("lat", lat), ("lat_y", y), ("lat_h", h), ("lat2d", lat2d), ("carry_a", a), ("carry_ay", ay), ("carry_ah", ah),
                      ("carry_b", b), ("carry_by", by), ("carry_bh", bh), ("rec", rec), ("rec_y", ry), ("rec_h", rh)):
        assert maxabs(got, G[pre + name], "h64 ks%d ds%d %s" % (ks, ds, name)) <= bound_for(G, pre + name, TIGHT_PASS)


def test_h64_chain_vs_golden(gv, dev, golden):
    """cyc2 CycleChain at (3, 3), fresh and carry form: two 6-frame halves with carried state equal the whole chain's goldens."""
    G = golden("frontend_h64")
    P = synth.CycleVAEProblem(tag="fechain", dilation_size=3, **H64)
    assert synth.sha256_state(P.enc) == str(G["chain_sha_enc"]) and synth.sha256_state(P.dec) == str(G["chain_sha_dec"])
    enc, dec = module(gv, P.enc, 30, 8, 64, 3, 3, True, dev), module(gv, P.dec, 6, 26, 64, 3, 3, False, dev)
    chain = gv.CycleChain(enc, dec, lat_dim=4, n_cyc=2)
    args = [T_(getattr(P, n), dev) for n in ("x", "cvx", "code_src", "code_trg", "y_in_enc", "y_in_dec")]
    with torch.no_grad():
        out = chain(*args, eps=T_(P.eps, dev))
        out2, state = chain(*args, eps=T_(P.eps, dev), return_state=True)
    finish(gv)
    assert sorted(out) == ["cv", "lat", "latcv", "rec", "reccyc"] and state is not None
    for k in out:
        assert maxabs(out[k], G["chain_" + k], "h64 ks3 ds3 chain " + k) <= TIGHT_CHAIN
        assert maxabs(out2[k], G["chain_" + k], "h64 ks3 ds3 chain (carry form) " + k) <= TIGHT_CHAIN


def test_h64_stage6_vs_golden(gv, dev, golden):
    """stage6.convert_pair at (3, 3), without and with window= (context frames from pad = 13: windows of 30 > 2 x 13 frames),
    against the reference's recorded statements; a window no longer than twice the reach is refused."""
    import stage6
    G = golden("frontend_h64")
    hidden, in_dim, out_dim, L, Ts, Tt, nd = [int(v) for v in G["s6_dims"]]
    tag, stdim = "fe6", in_dim - out_dim
    mu, sg = synth.feature_stats(tag + "/stats", in_dim)
    esd = synth.gru_rnn_state(tag + "/enc", in_dim, 2 * L, hidden, scale_in=(mu, sg), bias_scale=0.05, dilation_size=3)
    dsd = synth.gru_rnn_state(tag + "/dec", L + 2, out_dim, hidden, scale_out=(mu[stdim:], sg[stdim:]), bias_scale=0.05, dilation_size=3)
    assert synth.sha256_state(esd) == str(G["s6_sha_enc"]) and synth.sha256_state(dsd) == str(G["s6_sha_dec"])
    fs, ft = T_(synth.features(tag + "/src", 1, Ts, mu, sg)[0], dev), T_(synth.features(tag + "/trg", 1, Tt, mu, sg)[0], dev)
    es, et = T_(synth.normal(tag + "/eps_src", (nd, Ts, L)), dev), T_(synth.normal(tag + "/eps_trg", (nd, Tt, L)), dev)
    ypp = T_(np.zeros((1, 1, 2 * L), np.float32), dev)
    yd = T_(((0.0 - mu[stdim:]) / sg[stdim:]).astype(np.float32)[None, None, :], dev)
    enc, dec = module(gv, esd, in_dim, 2 * L, hidden, 3, 3, True, dev), module(gv, dsd, L + 2, out_dim, hidden, 3, 3, False, dev)
    with torch.no_grad():
        res = stage6.convert_pair(enc, dec, fs, ft, ypp, yd, yd, L, n_smpl_dec=nd, eps_src=es, eps_trg=et)
        win = stage6.convert_pair(enc, dec, fs, ft, ypp, yd, yd, L, n_smpl_dec=nd, eps_src=es, eps_trg=et, window=30)
        with pytest.raises(ValueError, match="reach"):
            stage6.convert_pair(enc, dec, fs, ft, ypp, yd, yd, L, n_smpl_dec=nd, eps_src=es, eps_trg=et, window=26)
    finish(gv)
    for got, w, key in zip(res, win, ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg")):
        assert maxabs(got, G["s6_" + key], "h64 ks3 ds3 convert_pair " + key) <= TIGHT_PASS
        assert maxabs(w, G["s6_" + key], "h64 ks3 ds3 convert_pair window=30 " + key) <= TIGHT_PASS


def test_train_mode_refused(gv, dev):
    """Autograd / dropout passes and Stage4Step of a network of another depth raise, naming dilation_size."""
    import stage4
    P = problem_h64(3, 3)
    enc = module(gv, P.enc, 30, 8, 64, 3, 3, True, dev)
    with pytest.raises(NotImplementedError, match="dilation_size"):
        enc(T_(P.x, dev), T_(P.y_in_enc, dev), clamp_vae=True, lat_dim=4)       # grad enabled, parameters require grad
    with pytest.raises(NotImplementedError, match="dilation_size"):
        stage4.Stage4Step(enc, module(gv, P.dec, 6, 26, 64, 3, 3, False, dev), lat_dim=4)
