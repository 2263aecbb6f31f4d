"""Stacked GRU networks (hidden_layers >= 2) without a GPU: the real library on the host-fiber emulator through the C ABI (*_deep
entry points) against the goldens recorded from the reference (tests/golden/make_golden_stacked.py), the drop-in module's
constructor / state_dict, the refusals of what is not covered, and the helper tests/stacked_ref.py pinned to the same goldens.

Bounds: the emulator's own (header of tests/test_emu_library.py): 5e-5 per pass, 3e-4 per chain.  stacked_ref (fp64) is held to
1e-6 of the reference's fp32 outputs: ten times the 1e-7 the reference's fp32 result sits from its fp64 result on these networks."""
import json
import os
import re

import numpy as np
import pytest

import _cabi
import stacked_digest
import stacked_ref
import synth
from emu_util import NpNet, emu_lib, ptr
from stacked_util import EMU_CHAIN, EMU_PASS, GENERIC, PERSISTENT, NpDeepNet, maxdiff

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H64 = dict(B=3, T=20, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1)
PATHS = {"resident": (PERSISTENT, _cabi.DEEP_RESIDENT), "generic": (GENERIC, _cabi.DEEP_GENERIC), "per_step": (0, _cabi.DEEP_PER_STEP)}
REF_PIN = 1e-6


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def problem(L):
    return synth.CycleVAEProblem(tag="stk%d" % L, hidden_layers=L, **H64)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("L", [2, 3])
def test_h64_passes_vs_golden(lib, golden, L, path):
    """3-D pass with clamp_vae, 2-D pass (B = 1), two windows with carried (y, h [L,B,H]) on each of the three recurrence forms."""
    flags, plan = PATHS[path]
    G = golden("stacked_h64")
    P = problem(L)
    assert synth.sha256_state(P.enc) == str(G["L%d_sha_enc" % L])
    net = NpDeepNet(lib, P.enc, 10, 8, 64, L)
    assert lib.plan_pass_deep(net.d, L, 3, 20, flags) == plan
    lat, y, h = net.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=flags)
    lat2d = net.forward(P.x[:1], P.y_in_enc[:1], clamp_lat_dim=4, flags=flags)[0][0]
    a, ay, ah = net.forward(P.x[:, :10], P.y_in_enc, clamp_lat_dim=4, flags=flags)
    b, by, bh = net.forward(P.x[:, 10:], ay, h_in=ah, clamp_lat_dim=4, flags=flags)
    assert h.shape == (L, 3, 64) and ah.shape == (L, 3, 64)
    got = dict(lat=lat, lat_y=y, lat_h=h, lat2d=lat2d, carry_a=a, carry_ah=ah, carry_b=b, carry_by=by, carry_bh=bh)
    for k, v in got.items():
        d = maxdiff(v, G["L%d_%s" % (L, k)])
        print("emu h64 L%d %-9s %-9s max|d| = %.3e" % (L, path, k, d))
        assert d <= EMU_PASS, (k, d)
    assert np.any(lat[:, :, 4:] == np.float32(stacked_ref.CLAMP_GAUSS)) or np.all(lat[:, :, 4:] > stacked_ref.CLAMP_GAUSS)


def test_h64_chain_vs_golden(lib, golden):
    """cyc2 eval chain, L = 2 encoder and decoder, pass by pass through cvae_gru_rnn_forward_deep with the draw inside each decoder
    pass's prologue (what CycleChain does for stacked modules on the device)."""
    G = golden("stacked_chain")
    P = synth.CycleVAEProblem(tag="stkchain", hidden_layers=2, **H64)
    assert synth.sha256_state(P.enc) == str(G["sha_enc"]) and synth.sha256_state(P.dec) == str(G["sha_dec"])
    enc, dec = NpDeepNet(lib, P.enc, 10, 8, 64, 2), NpDeepNet(lib, P.dec, 6, 6, 64, 2)
    L, prev = 4, None
    for i in range(2):
        if i == 0:
            lat = enc.forward(P.x, P.y_in_enc, clamp_lat_dim=L)[0]
        else:
            lat = enc.forward(P.x[:, :, :P.stdim], P.y_in_enc, clamp_lat_dim=L, seg1=prev)[0]
        rec = dec.forward(P.code_src, P.y_in_dec, lat=lat, lat_dim=L, eps=np.ascontiguousarray(P.eps[i, 0]))[0]
        cv = dec.forward(P.code_trg, P.y_in_dec, lat=lat, lat_dim=L, eps=np.ascontiguousarray(P.eps[i, 1]))[0]
        latcv = enc.forward(P.cvx, P.y_in_enc, clamp_lat_dim=L, seg1=cv)[0]
        reccyc = dec.forward(P.code_src, P.y_in_dec, lat=latcv, lat_dim=L, eps=np.ascontiguousarray(P.eps[i, 2]))[0]
        prev = reccyc
        for k, v in (("lat", lat), ("rec", rec), ("cv", cv), ("latcv", latcv), ("reccyc", reccyc)):
            d = maxdiff(v, G[k][i])
            print("emu h64 L2 chain cycle %d %-7s max|d| = %.3e" % (i, k, d))
            assert d <= EMU_CHAIN, (i, k, d)


def test_h64_stage6_sequence_vs_golden(lib, golden):
    """The stage-6 decode sequence at L = 2 as stage6.convert_pair issues it for stacked modules: one single-row cell per pass,
    constant code rows (row stride 0), the n-draw latent mean inside the decoder prologue."""
    G = golden("stacked_stage6_h64")
    hidden, in_dim, out_dim, L, Ts, Tt, nd = [int(v) for v in G["dims"]]
    tag, stdim = "stk6", in_dim - out_dim
    mu, sg = synth.feature_stats(tag + "/stats", in_dim)
    esd = synth.gru_rnn_state(tag + "/enc", in_dim, 2 * L, hidden, scale_in=(mu, sg), bias_scale=0.05, hidden_layers=2)
    dsd = synth.gru_rnn_state(tag + "/dec", L + 2, out_dim, hidden, scale_out=(mu[stdim:], sg[stdim:]), bias_scale=0.05, hidden_layers=2)
    assert synth.sha256_state(esd) == str(G["sha_enc"]) and synth.sha256_state(dsd) == str(G["sha_dec"])
    fs, ft = synth.features(tag + "/src", 1, Ts, mu, sg), synth.features(tag + "/trg", 1, Tt, mu, sg)
    es, et = synth.normal(tag + "/eps_src", (nd, Ts, L)), synth.normal(tag + "/eps_trg", (nd, Tt, L))
    y_pp = np.zeros((1, 1, 2 * L), np.float32)
    y_dec = ((0.0 - mu[stdim:]) / sg[stdim:]).astype(np.float32)[None, None, :]
    enc, dec = NpDeepNet(lib, esd, in_dim, 2 * L, hidden, 2), NpDeepNet(lib, dsd, L + 2, out_dim, hidden, 2)
    lat_src = enc.forward(fs, y_pp, clamp_lat_dim=L)[0]
    lat_trg = enc.forward(ft, y_pp, clamp_lat_dim=L)[0]
    src_code = lambda T: np.tile(np.array([1.0, 0.0], np.float32), (1, T, 1))
    trg_code = lambda T: np.tile(np.array([0.0, 1.0], np.float32), (1, T, 1))
    cv = dec.forward(trg_code(Ts), y_dec, lat=lat_src, lat_dim=L, eps=es, n_draws=nd)[0]
    cv_src = dec.forward(src_code(Ts), y_dec, lat=lat_src, lat_dim=L, eps=es, n_draws=nd)[0]
    cv_trg = dec.forward(trg_code(Tt), y_dec, lat=lat_trg, lat_dim=L, eps=et, n_draws=nd)[0]
    for k, v in (("lat_src", lat_src), ("lat_trg", lat_trg), ("cvmcep", cv), ("cvmcep_src", cv_src), ("cvmcep_trg", cv_trg)):
        d = maxdiff(v[0], G[k])
        print("emu h64 L2 stage6 %-10s max|d| = %.3e" % (k, d))
        assert d <= EMU_PASS, (k, d)


def test_stacked_pass_bits_are_the_parents(lib):
    """L = 2, 3 on each recurrence path: prepared images and pass outputs (carried state, injected eps, the n_draws prologue shape,
    the fused projection) are bit-identical to what the commit before the stacked pass was rebuilt from the one-layer pass's stages
    produced (tests/stacked_digest.py)."""
    lib.reset_options()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "stacked_pass_digests.json")))
    got = stacked_digest.digests(lib)
    assert sorted(got) == sorted(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


def test_one_layer_through_deep_entry_points_is_bit_identical(lib):
    """n_layers = 1: the *_deep entry points are the one-layer ones (same image, workspace and kernels): same bits."""
    P = synth.CycleVAEProblem(tag="stk1", **H64)
    a, b = NpNet(lib, P.enc, 10, 8, 64), NpDeepNet(lib, P.enc, 10, 8, 64, 1)
    assert lib.prepared_bytes_deep(a.d, 1) == lib.prepared_bytes(a.d)
    assert lib.pass_workspace_bytes_deep(a.d, 1, 3, 20) == lib.pass_workspace_bytes(a.d, 3, 20)
    assert np.array_equal(a.prepared, b.prepared)
    fl = _cabi.FLAG_PERSISTENT | _cabi.FLAG_EXACT3 | _cabi.FLAG_SPLIT_F16
    for flags in (fl, 0):
        ra = a.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=flags)
        rb = b.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=flags)
        for u, v in zip(ra, rb):
            assert np.array_equal(u, v)


def test_deep_entry_points_refuse_bad_arguments(lib):
    d = lib.desc(10, 8, 64, 3, 2, True, False)
    with pytest.raises(_cabi.CvaeError):
        lib.prepared_bytes_deep(d, 0)
    with pytest.raises(_cabi.CvaeError):
        lib.prepared_bytes_deep(d, _cabi.MAX_LAYERS + 1)
    with pytest.raises(_cabi.CvaeError):
        lib.plan_pass_deep(d, 1, 3, 20, 0)
    assert lib.prepared_bytes_deep(d, 3) > lib.prepared_bytes_deep(d, 2) > lib.prepared_bytes(d)
    # the resident kernel needs n_layers * H/8 resident blocks: four layers of H = 1024 do not fit 256 CUs, the any-H kernel takes them
    big = lib.desc(54, 64, 1024, 3, 2, True, False)
    assert lib.plan_pass_deep(big, 2, 64, 80, PERSISTENT) == _cabi.DEEP_RESIDENT
    assert lib.plan_pass_deep(big, 3, 64, 80, PERSISTENT) == _cabi.DEEP_GENERIC
    assert lib.plan_pass_deep(big, 2, 64, 80, GENERIC) == _cabi.DEEP_GENERIC
    assert lib.plan_pass_deep(lib.desc(54, 128, 2048, 3, 2, True, False), 2, 4, 16, PERSISTENT) == _cabi.DEEP_PER_STEP


def test_stacked_ref_is_pinned_to_the_goldens(golden):
    """tests/stacked_ref.py (fp64, stock torch) reproduces what the reference recorded, at H = 64 (L = 2, 3) and at hu1024 (L = 2)."""
    G = golden("stacked_h64")
    for L in (2, 3):
        P = problem(L)
        lat, y, h = stacked_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=4)
        a, ay, ah = stacked_ref.forward(P.enc, P.x[:, :10], P.y_in_enc, clamp_lat_dim=4)
        b, by, bh = stacked_ref.forward(P.enc, P.x[:, 10:], ay, h_in=ah, clamp_lat_dim=4)
        lat2d = stacked_ref.forward(P.enc, P.x[0], P.y_in_enc[:1], clamp_lat_dim=4)[0]
        for k, v in (("lat", lat), ("lat_y", y), ("lat_h", h), ("lat2d", lat2d), ("carry_b", b), ("carry_by", by), ("carry_bh", bh)):
            assert maxdiff(v, G["L%d_%s" % (L, k)]) <= REF_PIN, (L, k)
    G = golden("stacked_h1024")
    P = synth.CycleVAEProblem(B=4, T=80, bias_scale=0.05, tag="stk1024", hidden_layers=2)
    lat, y, h = stacked_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)
    for k, v in (("lat", lat), ("lat_y", y), ("lat_h", h)):
        d = maxdiff(v, G[k])
        print("stacked_ref vs reference, hu1024 L2 %-6s max|d| = %.3e" % (k, d))
        assert d <= REF_PIN, (k, d)


def test_module_has_the_reference_layout(golden):
    """Constructor, state_dict keys / shapes and load_state_dict of a reference-layout hidden_layers = 2 / 3 checkpoint."""
    import gru_vae
    G = golden("stacked_h64")
    for L in (2, 3):
        P = problem(L)
        m = gru_vae.GRU_RNN(in_dim=10, out_dim=8, hidden_units=64, hidden_layers=L, kernel_size=3, dilation_size=2, scale_in_flag=True,
                            scale_out_flag=False)
        assert list(m.state_dict().keys()) == [str(k) for k in G["L%d_keys" % L]]
        assert m.gru.num_layers == L and m.hidden_layers == L
        m.load_state_dict({k: torch.from_numpy(v) for k, v in P.enc.items()})            # strict: every key, every shape
        assert m.state_dict()["gru.weight_ih_l%d" % (L - 1)].shape == (192, 64)
    C = golden("stacked_chain")
    dec = gru_vae.GRU_RNN(in_dim=6, out_dim=6, hidden_units=64, hidden_layers=2, scale_in_flag=False, scale_out_flag=True)
    assert list(dec.state_dict().keys()) == [str(k) for k in C["keys_dec"]]
    drop = gru_vae.GRU_RNN(in_dim=6, out_dim=6, hidden_units=64, hidden_layers=2, do_prob=0.5)
    assert drop.gru.dropout == 0.5 and gru_vae.GRU_RNN(in_dim=6, out_dim=6, hidden_units=64, do_prob=0.5).gru.dropout == 0
    with pytest.raises(ValueError):
        gru_vae.GRU_RNN(hidden_layers=0)


def test_uncovered_paths_are_refused():
    """Train-mode / autograd passes, Stage4Step, the carry form of the chain and the windowed stage-6 form raise NotImplementedError
    naming hidden_layers (before anything touches a device)."""
    import gru_vae
    import stage4
    import stage6
    P = synth.CycleVAEProblem(tag="stkchain", hidden_layers=2, **H64)
    enc = gru_vae.GRU_RNN(in_dim=10, out_dim=8, hidden_units=64, hidden_layers=2, do_prob=0.5, scale_in_flag=True, scale_out_flag=False)
    dec = gru_vae.GRU_RNN(in_dim=6, out_dim=6, hidden_units=64, hidden_layers=2, scale_in_flag=False, scale_out_flag=True)
    x, y0 = torch.from_numpy(P.x), torch.from_numpy(P.y_in_enc)
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        enc(x, y0, do=True)                                       # train mode with dropout
    enc.eval()
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        enc(x, y0)                                                # autograd: parameters require grad
    with pytest.raises(NotImplementedError, match="hidden_layers"):
        stage4.Stage4Step(enc, dec, lat_dim=4)
    chain = gru_vae.CycleChain(enc, dec, lat_dim=4, n_cyc=2)
    args = [torch.from_numpy(getattr(P, n)) for n in ("x", "cvx", "code_src", "code_trg", "y_in_enc", "y_in_dec")]
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="hidden_layers"):
            chain(*args, return_state=True)
        with pytest.raises(NotImplementedError, match="hidden_layers"):
            stage6.convert_pair(enc, dec, x[0], x[1], y0[:1], args[5][:1], args[5][:1], 4, n_smpl_dec=2, window=8)
    assert stage6._net_config(enc)[0]["hidden_layers"] == 2       # the per-GPU workers of convert_files rebuild the same network


def test_synth_extra_layers_leave_the_one_layer_state_alone():
    one = synth.gru_rnn_state("stk/x", 10, 8, 64, bias_scale=0.1)
    two = synth.gru_rnn_state("stk/x", 10, 8, 64, bias_scale=0.1, hidden_layers=2)
    assert sorted(set(two) - set(one)) == ["gru.bias_hh_l1", "gru.bias_ih_l1", "gru.weight_hh_l1", "gru.weight_ih_l1"]
    assert synth.sha256_state({k: two[k] for k in one}) == synth.sha256_state(one)
    assert two["gru.weight_ih_l1"].shape == (192, 64) and not np.array_equal(two["gru.weight_hh_l1"], two["gru.weight_hh_l0"])


def test_deep_kernels_do_not_spill():
    """Resource remarks of the shipped gfx950 build: the recurrent kernels of stacked networks use no scratch, the resident one runs
    at one wave per SIMD inside the 512-register budget."""
    import __graft_entry__
    lib_path = os.path.join(ROOT, "cyclevae-vc_amd", "libcyclevae_hip.so")
    if not os.path.exists(__graft_entry__.RESOURCES) or not os.path.exists(lib_path) or \
            os.path.getmtime(__graft_entry__.RESOURCES) < os.path.getmtime(lib_path):
        __graft_entry__.build(force=True)
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(__graft_entry__.RESOURCES).read())[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        if "k_gru_steps_deep" not in name:
            continue
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert num(r"ScratchSize \[bytes/lane\]") == 0, name
        seen[name] = (num("    VGPRs"), num("AGPRs"), num(r"Occupancy \[waves/SIMD\]"))
    big = [v for k, v in seen.items() if "deep3ILi16E" in k]
    assert len(seen) == 4 and len(big) == 1, sorted(seen)
    assert big[0][0] + big[0][1] <= 512 and big[0][2] == 1
