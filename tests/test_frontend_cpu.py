"""Conv front-ends of depth 1 and 3 (reference dilation_size) and kernel_size 5 without a GPU: the real library on the host-fiber
emulator through the C ABI against the goldens recorded from the reference (tests/golden/make_golden_frontend.py), the plan rows of
the new forms, the default depth's bits against the commit before (tests/frontend_digest.py), the refusals, the drop-in module's
layout, and the helper tests/frontend_ref.py pinned to the same goldens.

Bounds: the emulator's own (tests/stacked_util.py: 5e-5 per pass, 3e-4 per chain), through frontend_util.bound_for; 3e-6 kernel
against kernel; frontend_ref (fp64) is held to 1e-6 of the reference's fp32 outputs, as stacked_ref is."""
import json
import os
import re

import numpy as np
import pytest

import _cabi
import frontend_digest
import frontend_ref
import synth
from emu_util import emu_lib, ptr
from frontend_util import (DEFAULT, DEPTHS_H64, E_, EMU_CHAIN, EMU_PASS, G_, H64, HST, P_, S_, TIGHT_KERNELS, NpFrontNet, bound_for,
                           maxdiff, problem_h64)
from stacked_util import NpDeepNet

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V2, V6, V6H, LL, GENERIC, PER_STEP = _cabi.EVAL_V2, _cabi.EVAL_V6, _cabi.EVAL_V6H, _cabi.EVAL_LL, _cabi.EVAL_GENERIC, _cabi.EVAL_PER_STEP
REF_PIN = 1e-6
# flags -> the form the ENCODER (in_dim 30) takes per (ks, ds); the decoder (in_dim 6) has KFW 1 at (3, 1) and KFW 4 else
PATHS = {"default": DEFAULT, "generic": P_ | G_, "per_step": 0}
ENC_FORM = {"default": {(3, 1): V6, (3, 3): V6H, (5, 2): V6H}, "generic": GENERIC, "per_step": PER_STEP}


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


_NETS = {}


def nets(lib, ks, ds):
    """The prepared encoder / decoder of one golden depth, built once per process: folding a 27-tap front-end is the emulator's
    slowest step (one fiber per element of the fold)."""
    if (ks, ds) not in _NETS:
        P = problem_h64(ks, ds)
        _NETS[(ks, ds)] = (P, NpFrontNet(lib, P.enc, 30, 8, 64, ks, ds), NpFrontNet(lib, P.dec, 6, 26, 64, ks, ds))
    return _NETS[(ks, ds)]


def test_default_depth_bits_are_the_parents(lib):
    """layers == 2: prepared images and pass outputs (every recurrence form) are bit-identical to what the commit before the fold
    became an iteration over layers produced, at the shapes of tests/test_emu_library.py."""
    lib.reset_options()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "frontend_layers2_digests.json")))
    got = frontend_digest.digests(lib)
    assert sorted(got) == sorted(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


# (in_dim, H, ks, ds, rows, flags, T) -> form; 256 CUs
TABLE = [
    (30, 64, 3, 3, 5, DEFAULT, 12, V6H),            # KFW 14
    (30, 64, 5, 2, 5, DEFAULT, 12, V6H),            # KFW 13
    (54, 1024, 3, 3, 64, DEFAULT, 12, V6H),         # the encoder: 27 x 56 = 1512 k, KFW 24
    (34, 1024, 3, 3, 64, DEFAULT, 12, V6H),         # the decoder: KFW 17
    (54, 1024, 3, 3, 4, DEFAULT, 12, V6H),          # a half-empty 32-row tile, as on V6
    (54, 1024, 3, 3, 160, DEFAULT, 6, V6H),
    (54, 1024, 3, 1, 64, DEFAULT, 12, V6),          # KFW 3: k_gru_steps_v6<16, 3>
    (34, 1024, 3, 1, 64, DEFAULT, 12, V6),          # KFW 2: k_gru_steps_v6<16, 2>
    (30, 64, 3, 1, 5, DEFAULT, 12, V6),             # KFW 2 at H = 64
    (54, 1024, 3, 3, 2, DEFAULT, 12, LL),
    (30, 64, 3, 3, 2, DEFAULT, 12, LL),
    (54, 1024, 3, 3, 64, DEFAULT | G_, 12, GENERIC),
    (30, 64, 3, 3, 5, DEFAULT | G_, 12, GENERIC),
    (54, 1024, 3, 3, 64, DEFAULT | HST, 12, V2),    # HOISTED_FRONTEND keeps its meaning: the 16-row kernel behind the GEMM
    (30, 64, 3, 3, 5, DEFAULT | HST, 12, V2),
    (54, 1024, 3, 3, 64, P_ | S_, 12, V2),          # without EXACT3: no fused pair / fp32 instance of that width
    (54, 1024, 3, 3, 64, 0, 12, PER_STEP),
    (54, 1024, 3, 3, 64, DEFAULT, 1, PER_STEP),
    (20, 1024, 3, 2, 64, DEFAULT, 8, V2),           # KFW 4 stays where tests/test_eval_plan.py pins it
    (6, 64, 3, 3, 5, DEFAULT, 12, V2),              # KFW 4 at H = 64 (the decoder of the goldens)
    (54, 2048, 3, 3, 64, DEFAULT, 12, V6H),         # k_gru_steps_v6<32, 0, 3, true>
    (54, 2048, 3, 3, 2, DEFAULT, 12, PER_STEP),     # no LL above H = 1024
    (54, 128, 3, 3, 8, DEFAULT, 12, GENERIC),       # no hoisted instance at H = 128
]


def test_plan_table_of_the_new_rows(lib, options):
    lib.reset_options()
    for in_dim, H, ks, ds, rows, flags, T, form in TABLE:
        got = lib.plan_pass(lib.desc(in_dim, 8, H, ks, ds, True, False), rows, T, flags)
        assert got == form, (in_dim, H, ks, ds, rows, flags, T, got, form)
    options(v6_limbs_h2048=2)       # no pair form of the hoisted kernel at H = 2048
    assert lib.plan_pass(lib.desc(54, 8, 2048, 3, 3, True, False), 64, 12, DEFAULT) == PER_STEP
    options(v6_limbs_h2048=3, v6_limbs_h64=2)
    assert lib.plan_pass(lib.desc(30, 8, 64, 3, 3, True, False), 5, 12, DEFAULT) == V6H
    text = open(os.path.join(ROOT, "include", "cyclevae_hip.h")).read()
    assert int(re.search(r"CVAE_EVAL_V6H = (\d+)", text).group(1)) == V6H
    assert int(re.search(r"#define CVAE_ABI_VERSION (\d+)", text).group(1)) == _cabi.ABI_VERSION == 10


def _passes(enc, dec, P, G, pre, flags, rows=slice(None)):
    """The recorded passes of one (ks, ds) on the given flags: {golden key: output}."""
    x, y0 = P.x[rows], P.y_in_enc[rows]
    lat, y, h = enc.forward(x, y0, clamp_lat_dim=4, flags=flags)
    lat2d = enc.forward(x[:1], y0[:1], clamp_lat_dim=4, flags=flags)[0][0]
    a, ay, ah = enc.forward(x[:, :6], y0, clamp_lat_dim=4, flags=flags)
    b, by, bh = enc.forward(x[:, 6:], ay, h_in=ah, clamp_lat_dim=4, flags=flags)
    rec, ry, rh = dec.forward(P.code_src[rows], P.y_in_dec[rows], lat=np.ascontiguousarray(G[pre + "lat"][rows]), lat_dim=4,
                              eps=np.ascontiguousarray(P.eps[0, 0][rows]), flags=flags)
    return dict(lat=lat, lat_y=y, lat_h=h, lat2d=lat2d, carry_a=a, carry_ay=ay, carry_ah=ah, carry_b=b, carry_by=by, carry_bh=bh,
                rec=rec, rec_y=ry, rec_h=rh)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("ks,ds", DEPTHS_H64)
def test_h64_passes_vs_golden(lib, golden, ks, ds, path):
    """Every golden of frontend_h64.npz -- 3-D pass with clamp_vae, 2-D pass, two windows with carried (y, h), decoder pass with the
    draw in its prologue -- on V6H / the fused V6 instances (default), GENERIC and PER_STEP (V2: test_v6h_against_v2 below)."""
    lib.reset_options()
    G = golden("frontend_h64")
    (P, enc, dec), pre = nets(lib, ks, ds), "k%dd%d_" % (ks, ds)
    assert synth.sha256_state(P.enc) == str(G[pre + "sha_enc"]) and synth.sha256_state(P.dec) == str(G[pre + "sha_dec"])
    form = ENC_FORM[path]
    assert lib.plan_pass(enc.d, 5, 12, PATHS[path]) == (form[(ks, ds)] if isinstance(form, dict) else form)
    for k, v in _passes(enc, dec, P, G, pre, PATHS[path]).items():
        d = maxdiff(v, G[pre + k])
        print("emu h64 ks%d ds%d %-8s %-9s max|d| = %.3e" % (ks, ds, path, k, d))
        assert d <= bound_for(G, pre + k, EMU_PASS), (k, d)


@pytest.mark.parametrize("ks,ds", DEPTHS_H64)
def test_h64_two_rows_on_the_word_exchange_kernel(lib, golden, ks, ds):
    """Rows are independent recurrences: the first two rows of every recorded pass on k_gru_steps_ll (at most three rows)."""
    lib.reset_options()
    G = golden("frontend_h64")
    (P, enc, dec), pre = nets(lib, ks, ds), "k%dd%d_" % (ks, ds)
    assert lib.plan_pass(enc.d, 2, 12, DEFAULT) == LL and lib.plan_pass(dec.d, 2, 12, DEFAULT) == LL
    rows = slice(0, 2)
    for k, v in _passes(enc, dec, P, G, pre, DEFAULT, rows).items():
        want = G[pre + k]
        want = want if k == "lat2d" else (want[:, rows] if k in ("lat_h", "carry_ah", "carry_bh", "rec_h") else want[rows])
        d = maxdiff(v, want)
        print("emu h64 ks%d ds%d LL       %-9s max|d| = %.3e" % (ks, ds, k, d))
        assert d <= bound_for(G, pre + k, EMU_PASS), (k, d)


@pytest.mark.parametrize("opts", [{}, {"v6_limbs_h64": 2}, {"v6_w2s_h64": 1}])
def test_v6h_against_v2(lib, options, opts):
    """The hoisted exact-operand kernel -- three limbs, the two-limb form, the streamed-third-limb form -- against the 16-row
    fp32-MFMA kernel behind the same GEMM, on the recorded (3, 3) pass with a carried-in state.  The two-limb form carries 22-bit
    operands: the pair kernels' bound of tests/test_emu_library.py (2e-5)."""
    lib.reset_options()
    P, enc, _ = nets(lib, 3, 3)
    h0 = (0.5 * synth.normal("fe33/h_in", (5, 64))).astype(np.float32)
    if "v2" not in _NETS:
        assert lib.plan_pass(enc.d, 5, 12, DEFAULT | HST) == V2
        _NETS["v2"] = enc.forward(P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, flags=DEFAULT | HST)
    options(**opts)
    assert lib.plan_pass(enc.d, 5, 12, DEFAULT) == V6H
    a = enc.forward(P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, flags=DEFAULT)
    tol = 2e-5 if opts.get("v6_limbs_h64") == 2 else TIGHT_KERNELS
    for name, u, v in zip(("trj", "y_last", "h"), a, _NETS["v2"]):
        d = maxdiff(u, v)
        print("emu V6H vs V2 %-22s %-7s max|d| = %.3e" % (opts, name, d))
        assert np.isfinite(u).all() and d <= tol, (name, d)


def test_v6h_tiles_per_block(lib, options):
    """70 rows = three 32-row tiles, the last ragged, T = 2, carried-in state: one tile per block (24 blocks) and all three in
    one block (max_rt = 1: the path that re-reads its own state from the exchange buffer, exact with three limbs) give the same bits
    (two tiles per block: the 160-row device test); rows picked from all three tiles, run alone in one tile, too; 33 rows against V2."""
    lib.reset_options()
    _, enc, _ = nets(lib, 3, 3)
    P = synth.CycleVAEProblem(B=70, T=2, in_dim=30, out_dim=26, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1, tag="fe33v", dilation_size=3)
    h0 = (0.5 * synth.normal("fe33v/h_in", (70, 64))).astype(np.float32)
    assert lib.plan_pass(enc.d, 70, 2, DEFAULT) == V6H
    a = enc.forward(P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, flags=DEFAULT)
    options(max_rt=1)
    b = enc.forward(P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, flags=DEFAULT)
    assert all(np.array_equal(u, v) and np.isfinite(u).all() for u, v in zip(a, b))
    lib.reset_options()
    rows = [0, 31, 32, 40, 63, 64, 69]
    sub = enc.forward(P.x[rows], P.y_in_enc[rows], h_in=h0[rows], clamp_lat_dim=4, flags=DEFAULT)
    assert np.array_equal(sub[0], a[0][rows]) and np.array_equal(sub[2], a[2][:, rows])
    v2 = enc.forward(P.x[:33], P.y_in_enc[:33], h_in=h0[:33], clamp_lat_dim=4, flags=DEFAULT | HST)
    for name, u, v in zip(("trj", "y_last", "h"), a, v2):
        u = u[:, :33] if name == "h" else u[:33]
        d = maxdiff(u, v)
        print("emu V6H (70 rows) vs V2 (rows 0..32) %-7s max|d| = %.3e" % (name, d))
        assert d <= TIGHT_KERNELS, (name, d)


def test_range_word_on_v6h_covers_the_state_only(lib):
    """A carried-in state of 1e5 raises status 7 on V6H (its slot-0 limb triples cannot carry it); a normalised input of 1e5 does
    not: it goes through the fp32 GEMM, as in the stacked path."""
    lib.reset_options()
    P, enc, _ = nets(lib, 3, 3)
    assert lib.plan_pass(enc.d, 5, 12, DEFAULT) == V6H

    def status(x, h):
        y = np.ascontiguousarray(P.y_in_enc.reshape(5, 8))
        trj = np.full((5, 12, 8), np.nan, np.float32)
        ws = np.full(lib.pass_workspace_bytes(enc.d, 5, 12) // 4, np.float32(7.0), np.float32)
        lib.gru_rnn_forward(enc.d, ptr(enc.prepared), lib.pass_input((ptr(x), 30, 30)), ptr(y), ptr(h), 5, 12, 4, ptr(trj), None, None,
                            ptr(ws), ws.nbytes, DEFAULT)
        return lib.workspace_status(ptr(ws)), trj
    h = (0.5 * synth.normal("fe33/h_in", (5, 64))).astype(np.float32)
    x = np.ascontiguousarray(P.x)
    st, _ = status(x, h)
    assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == 0, st
    h[1, 5] = 1e5
    st, _ = status(x, h)
    assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == _cabi.STATUS_RANGE, st
    h[1, 5] = 0.25
    big = x.copy()
    big[2, 3, 7] = 1e5 * P.sigma[7] + P.mu[7]       # x^ = scale_in(x) = 1e5 there
    st, trj = status(big, h)
    assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == 0 and np.isfinite(trj).all(), st


def test_unfit_image_leaves_v6h(lib):
    """An image with a recurrent weight beyond the fp16 range: once the context knows, its passes run the fp32-operand kernels
    whatever flags they are given -- the bits of the pass without EXACT3 / SPLIT_F16 -- and raise nothing."""
    lib.reset_options()
    P = problem_h64(3, 3)
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["gru.weight_hh_l0"][64 + 7, 3] = 1e5
    enc = NpFrontNet(lib, sd, 30, 8, 64, 3, 3)
    assert lib.net_prepared_in_range(enc.d, 1, ptr(enc.prepared)) is False
    a = enc.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=DEFAULT)
    b = enc.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=P_)
    assert lib.plan_pass(enc.d, 5, 12, P_) == V2
    assert all(np.array_equal(u, v) and np.isfinite(u).all() for u, v in zip(a, b))
    ref = frontend_ref.forward(sd, P.x, P.y_in_enc, clamp_lat_dim=4)
    r32 = frontend_ref.forward(sd, P.x, P.y_in_enc, clamp_lat_dim=4, dtype=torch.float32)
    n = maxdiff(r32[0], ref[0])
    assert maxdiff(a[0], ref[0]) <= max(EMU_PASS, 4.0 * n)
    # (a fit image at the same address is asked about again: the context forgets the old answer)
    enc.prepared[:] = nets(lib, 3, 3)[1].prepared
    assert lib.net_prepared_in_range(enc.d, 1, ptr(enc.prepared)) is True


def test_h64_chain_vs_golden(lib, golden):
    """cyc2 eval chain at (3, 3) through cvae_cycle_forward: encoder passes on V6H, decoder passes on V2 (KFW 4), the stacked rec ||
    cv pass included."""
    lib.reset_options()
    G = golden("frontend_h64")
    P = synth.CycleVAEProblem(tag="fechain", dilation_size=3, **H64)
    assert synth.sha256_state(P.enc) == str(G["chain_sha_enc"]) and synth.sha256_state(P.dec) == str(G["chain_sha_dec"])
    enc, dec = NpFrontNet(lib, P.enc, 30, 8, 64, 3, 3), NpFrontNet(lib, P.dec, 6, 26, 64, 3, 3)
    assert lib.plan_pass(enc.d, 5, 12, DEFAULT) == V6H and lib.plan_pass(dec.d, 10, 12, DEFAULT) == V2
    B, T = P.B, P.T
    outs = {k: np.full((2, B, T, c), np.nan, np.float32) for k, c in (("lat", 8), ("rec", 26), ("cv", 26), ("latcv", 8), ("reccyc", 26))}
    ws = np.zeros(lib.cycle_workspace_bytes(enc.d, dec.d, B, T, 2) // 4, np.float32)
    ye, yd = np.ascontiguousarray(P.y_in_enc.reshape(B, 8)), np.ascontiguousarray(P.y_in_dec.reshape(B, 26))
    eps = np.ascontiguousarray(P.eps)
    lib.cycle_forward(enc.d, ptr(enc.prepared), dec.d, ptr(dec.prepared), ptr(P.x), ptr(P.cvx), P.stdim, ptr(P.code_src),
                      ptr(P.code_trg), 2, ptr(ye), ptr(yd), B, T, 2, 4, ptr(eps), 0, ptr(outs["lat"]), ptr(outs["rec"]),
                      ptr(outs["cv"]), ptr(outs["latcv"]), ptr(outs["reccyc"]), ptr(ws), ws.nbytes, DEFAULT)
    st = lib.workspace_status(ptr(ws))
    assert st[0] == 0 and st[_cabi.STATUS_RANGE_WORD] == 0, st
    for k, v in outs.items():
        d = maxdiff(v, G["chain_" + k])
        print("emu h64 ks3 ds3 chain %-7s max|d| = %.3e" % (k, d))
        assert d <= EMU_CHAIN, (k, d)


def test_h64_stage6_sequence_vs_golden(lib, golden):
    """The stage-6 statement sequence at (3, 3): single-row passes (k_gru_steps_ll), the n-draw latent mean in the decoder prologue."""
    lib.reset_options()
    G = golden("frontend_h64")
    hidden, in_dim, out_dim, L, Ts, Tt, nd = [int(v) for v in G["s6_dims"]]
    tag, stdim = "fe6", in_dim - out_dim
    mu, sg = synth.feature_stats(tag + "/stats", in_dim)
    esd = synth.gru_rnn_state(tag + "/enc", in_dim, 2 * L, hidden, scale_in=(mu, sg), bias_scale=0.05, dilation_size=3)
    dsd = synth.gru_rnn_state(tag + "/dec", L + 2, out_dim, hidden, scale_out=(mu[stdim:], sg[stdim:]), bias_scale=0.05, dilation_size=3)
    assert synth.sha256_state(esd) == str(G["s6_sha_enc"]) and synth.sha256_state(dsd) == str(G["s6_sha_dec"])
    fs, ft = synth.features(tag + "/src", 1, Ts, mu, sg), synth.features(tag + "/trg", 1, Tt, mu, sg)
    es, et = synth.normal(tag + "/eps_src", (nd, Ts, L)), synth.normal(tag + "/eps_trg", (nd, Tt, L))
    y_pp = np.zeros((1, 1, 2 * L), np.float32)
    y_dec = ((0.0 - mu[stdim:]) / sg[stdim:]).astype(np.float32)[None, None, :]
    enc, dec = NpDeepLike(lib, esd, in_dim, 2 * L, hidden), NpDeepLike(lib, dsd, L + 2, out_dim, hidden)
    lat_src = enc.forward(fs, y_pp, clamp_lat_dim=L)[0]
    lat_trg = enc.forward(ft, y_pp, clamp_lat_dim=L)[0]
    code = lambda T, i: np.tile(np.eye(2, dtype=np.float32)[i], (1, T, 1))
    cv = dec.forward(code(Ts, 1), y_dec, lat=lat_src, lat_dim=L, eps=es, n_draws=nd)[0]
    cv_src = dec.forward(code(Ts, 0), y_dec, lat=lat_src, lat_dim=L, eps=es, n_draws=nd)[0]
    cv_trg = dec.forward(code(Tt, 1), y_dec, lat=lat_trg, lat_dim=L, eps=et, n_draws=nd)[0]
    for k, v in (("lat_src", lat_src), ("lat_trg", lat_trg), ("cvmcep", cv), ("cvmcep_src", cv_src), ("cvmcep_trg", cv_trg)):
        d = maxdiff(v[0], G["s6_" + k])
        print("emu h64 ks3 ds3 stage6 %-10s max|d| = %.3e" % (k, d))
        assert d <= EMU_PASS, (k, d)


class NpDeepLike(NpDeepNet):
    """A ONE-GRU-layer net of depth-3 front-end driven through the *_deep entry points (n_layers = 1 is the one-layer path), whose
    numpy wrapper takes n_draws."""

    def __init__(self, lib, sd, in_dim, out_dim, hidden, n_layers=1, ks=3, ds=3):
        self.lib, self.L = lib, n_layers
        self.sd = {k: np.ascontiguousarray(v, np.float32) for k, v in sd.items()}
        self.d = lib.desc(in_dim, out_dim, hidden, ks, ds, "scale_in.weight" in sd, "scale_out.weight" in sd)
        self.prepared = np.zeros(lib.prepared_bytes_deep(self.d, n_layers) // 4, np.float32)
        scratch = np.zeros(lib.prepare_scratch_bytes_deep(self.d, n_layers) // 8 + 1, np.float64)
        wp = {f: ptr(self.sd[k]) for f, k in _cabi.STATE_KEYS.items() if k in self.sd}
        upper = [tuple(ptr(self.sd[k]) for k in keys) for keys in _cabi.upper_layer_keys(n_layers)]
        lib.net_prepare_deep(self.d, n_layers, wp, upper, ptr(self.prepared), self.prepared.nbytes, ptr(scratch), scratch.nbytes)


@pytest.mark.parametrize("flags", [P_, P_ | G_])
def test_stacked_network_with_a_depth_3_front_end(lib, flags):
    """hidden_layers = 2 behind dilation_size = 3 (resident and any-H recurrence of cvae_gru_rnn_forward_deep): layer 0's input
    side is the same GEMM over the folded 27-tap matrix.  Against the fp64 restatement, allowance as in tests/test_range_guard_cpu.py:
    the emulator's bound or four times the restatement's own fp32 distance."""
    lib.reset_options()
    P = synth.CycleVAEProblem(tag="fe33L2", hidden_layers=2, dilation_size=3, **H64)
    net = NpDeepLike(lib, P.enc, 30, 8, 64, n_layers=2)
    h0 = (0.5 * synth.normal("fe33L2/h_in", (2, 5, 64))).astype(np.float32)
    got = net.forward(P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, flags=flags)
    ref = frontend_ref.forward(P.enc, P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4)
    r32 = frontend_ref.forward(P.enc, P.x, P.y_in_enc, h_in=h0, clamp_lat_dim=4, dtype=torch.float32)
    assert got[2].shape == (2, 5, 64)
    for name, u, v, w in zip(("trj", "y_last", "h"), got, ref, r32):
        d, n = maxdiff(u, v), maxdiff(w, v)
        print("emu h64 L2 ds3 flags %d %-6s max|d| = %.3e (restatement fp32 vs fp64 %.3e)" % (flags, name, d, n))
        assert d <= max(EMU_PASS, 4.0 * n), (name, d)


def test_frontend_ref_is_pinned_to_the_goldens(golden):
    """tests/frontend_ref.py (fp64, stock torch) reproduces what the reference recorded, at H = 64 (every depth) and at hu1024."""
    import frontend_util
    G = golden("frontend_h64")
    for ks, ds in DEPTHS_H64:
        P, pre = problem_h64(ks, ds), "k%dd%d_" % (ks, ds)
        lat, y, h = frontend_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=4)
        lat2d = frontend_ref.forward(P.enc, P.x[0], P.y_in_enc[:1], clamp_lat_dim=4)[0]
        a, ay, ah = frontend_ref.forward(P.enc, P.x[:, :6], P.y_in_enc, clamp_lat_dim=4)
        b, by, bh = frontend_ref.forward(P.enc, P.x[:, 6:], ay, h_in=ah, clamp_lat_dim=4)
        for k, v in (("lat", lat), ("lat_y", y), ("lat_h", h), ("lat2d", lat2d), ("carry_b", b), ("carry_by", by), ("carry_bh", bh)):
            assert maxdiff(v, G[pre + k]) <= REF_PIN, (ks, ds, k)
    G = golden("frontend_h1024")
    for ks, ds in frontend_util.DEPTHS_H1024:
        P, pre = frontend_util.problem_h1024(ks, ds), "k%dd%d_" % (ks, ds)
        assert synth.sha256_state(P.enc) == str(G[pre + "sha_enc"]) and synth.sha256_state(P.dec) == str(G[pre + "sha_dec"])
        for k, v in zip(("lat", "lat_y", "lat_h"), frontend_ref.forward(P.enc, P.x, P.y_in_enc, clamp_lat_dim=32)):
            d = maxdiff(v, G[pre + k])
            print("frontend_ref vs reference, hu1024 ks%d ds%d %-6s max|d| = %.3e" % (ks, ds, k, d))
            assert d <= REF_PIN, (k, d)


def test_module_has_the_reference_layout(golden):
    """Constructor, state_dict keys / shapes and strict load_state_dict per depth; TwoSidedDilConv1d on its own is the conv stack."""
    import gru_vae
    G = golden("frontend_h64")
    for ks, ds in DEPTHS_H64:
        P, pre = problem_h64(ks, ds), "k%dd%d_" % (ks, ds)
        enc = gru_vae.GRU_RNN(in_dim=30, out_dim=8, hidden_units=64, kernel_size=ks, dilation_size=ds, scale_in_flag=True, scale_out_flag=False)
        dec = gru_vae.GRU_RNN(in_dim=6, out_dim=26, hidden_units=64, kernel_size=ks, dilation_size=ds, scale_in_flag=False, scale_out_flag=True)
        assert list(enc.state_dict().keys()) == [str(k) for k in G[pre + "keys_enc"]]
        assert list(dec.state_dict().keys()) == [str(k) for k in G[pre + "keys_dec"]]
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in P.enc.items()})
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in P.dec.items()})
        assert enc.receptive_field == ks ** ds and enc.tot_in_dim == 30 * ks ** ds + 8 and enc.conv.padding == (ks ** ds - 1) // 2
        with torch.no_grad():
            alone = enc.conv(torch.from_numpy(P.x).transpose(1, 2)).transpose(1, 2).numpy()
        sd = {k: v for k, v in P.enc.items() if k.startswith("conv.")}
        assert alone.shape == (5, 12, 30 * ks ** ds)
        assert maxdiff(alone, frontend_ref.front_end(sd, P.x).numpy()) <= REF_PIN


def test_synth_depth_arguments_leave_the_default_state_alone():
    two = synth.gru_rnn_state("fe/x", 10, 8, 64, bias_scale=0.1)
    assert synth.sha256_state(synth.gru_rnn_state("fe/x", 10, 8, 64, bias_scale=0.1, dilation_size=2, kernel_size=3)) == synth.sha256_state(two)
    one = synth.gru_rnn_state("fe/x", 10, 8, 64, bias_scale=0.1, dilation_size=1)
    three = synth.gru_rnn_state("fe/x", 10, 8, 64, bias_scale=0.1, dilation_size=3)
    assert sorted(set(three) - set(two)) == ["conv.conv.2.bias", "conv.conv.2.weight"]
    assert sorted(set(two) - set(one)) == ["conv.conv.1.bias", "conv.conv.1.weight"]
    assert three["conv.conv.2.weight"].shape == (270, 90, 3) and three["gru.weight_ih_l0"].shape == (192, 278)
    assert one["gru.weight_ih_l0"].shape == (192, 38)
    for k in ("conv.conv.0.weight", "conv.conv.0.bias", "gru.weight_hh_l0", "out_1.weight"):
        assert np.array_equal(one[k], two[k]) and np.array_equal(three[k], two[k])
    assert np.array_equal(three["conv.conv.1.weight"], two["conv.conv.1.weight"])
    five = synth.gru_rnn_state("fe/x", 10, 8, 64, kernel_size=5)
    assert five["conv.conv.1.weight"].shape == (250, 50, 5)


def test_uncovered_paths_are_refused(lib):
    """Training a network of another depth raises NotImplementedError naming dilation_size, before anything touches a device; the
    train / backward entry points of the library return an error; depths 0 and 4, and kernel_size 5 at depth 3, are refused."""
    import gru_vae
    import stage4
    P = problem_h64(3, 3)
    enc = gru_vae.GRU_RNN(in_dim=30, out_dim=8, hidden_units=64, dilation_size=3, do_prob=0.5, scale_in_flag=True, scale_out_flag=False)
    dec = gru_vae.GRU_RNN(in_dim=6, out_dim=26, hidden_units=64, dilation_size=1, scale_in_flag=False, scale_out_flag=True)
    x, y0 = torch.from_numpy(P.x), torch.from_numpy(P.y_in_enc)
    with pytest.raises(NotImplementedError, match="dilation_size"):
        enc(x, y0, do=True)                                       # train mode with dropout
    enc.eval()
    with pytest.raises(NotImplementedError, match="dilation_size"):
        enc(x, y0)                                                # autograd: parameters require grad
    with pytest.raises(NotImplementedError, match="dilation_size"):
        stage4.Stage4Step(enc, dec, lat_dim=4)
    with pytest.raises(NotImplementedError, match="dilation_size"):
        stage4.Stage4Step(gru_vae.GRU_RNN(in_dim=30, out_dim=8, hidden_units=64), dec, lat_dim=4)
    for ks, ds in ((5, 3), (3, 0), (3, 4)):
        with pytest.raises(ValueError, match="dilation_size"):
            gru_vae.GRU_RNN(in_dim=30, out_dim=8, hidden_units=64, kernel_size=ks, dilation_size=ds)
        with pytest.raises(_cabi.CvaeError, match="kernel_size" if ds == 3 else "layers"):
            lib.prepared_bytes(lib.desc(30, 8, 64, ks, ds, True, False))
    assert lib.prepared_bytes(lib.desc(30, 8, 64, 7, 2, True, False)) > 0          # whatever layers == 2 accepted stays accepted
    # depth 3 wants H % 64 == 0 (tests/test_emu_library.py pins the refusal of hidden 32); depths 1 and 2 take any H % 16 == 0
    with pytest.raises(_cabi.CvaeError, match="multiple of 64"):
        lib.prepared_bytes(lib.desc(30, 8, 48, 3, 3, True, False))
    with pytest.raises(ValueError, match="multiple of 64"):
        gru_vae.GRU_RNN(in_dim=30, out_dim=8, hidden_units=48, dilation_size=3)
    assert lib.prepared_bytes(lib.desc(30, 8, 48, 3, 1, True, False)) > 0 and lib.prepared_bytes(lib.desc(30, 8, 128, 3, 3, True, False)) > 0
    buf = np.zeros(64, np.float32)
    grads = {f: ptr(buf) for f in _cabi.GRAD_FIELDS}
    for ds in (1, 3):
        d = lib.desc(30, 8, 64, 3, ds, True, False)
        assert lib.train_image_bytes(d) == 0 and "dilation_size" in lib.lib.cvae_last_error_string().decode()
        assert lib.train_tape_bytes(d, 5, 12) == 0 and lib.train_scratch_bytes(d, 5, 12) == 0
        with pytest.raises(_cabi.CvaeError, match="dilation_size"):
            lib.net_prepare_train(d, {}, ptr(buf), buf.nbytes)
        with pytest.raises(_cabi.CvaeError, match="dilation_size"):
            lib.forward_train(d, ptr(buf), ptr(buf), ptr(buf), None, 5, 12, -1, None, None, 0, 0.0, ptr(buf), ptr(buf), ptr(buf), ptr(buf),
                              buf.nbytes, ptr(buf), buf.nbytes)
        with pytest.raises(_cabi.CvaeError, match="dilation_size"):
            lib.backward(d, ptr(buf), ptr(buf), 5, 12, -1, ptr(buf), ptr(buf), buf.nbytes, None, grads)


def test_new_kernels_do_not_spill():
    """Resource remarks of the shipped gfx950 build: the hoisted instances and the two fused instances of the one-layer front-end
    use no scratch; the H = 1024 and H = 2048 ones run at one wave per SIMD inside the 512-register budget."""
    import __graft_entry__
    lib_path = os.path.join(ROOT, "cyclevae-vc_amd", "libcyclevae_hip.so")
    if not os.path.exists(__graft_entry__.RESOURCES) or not os.path.exists(lib_path) or \
            os.path.getmtime(__graft_entry__.RESOURCES) < os.path.getmtime(lib_path):
        __graft_entry__.build(force=True)
    blocks = re.split(r"remark: [^\n]*Function Name: ", open(__graft_entry__.RESOURCES).read())[1:]
    want = {"v6ILi16ELi0ELi3ELb0E": True, "v6ILi32ELi0ELi3ELb1E": True, "v6ILi16ELi3ELi3ELb0E": True, "v6ILi16ELi2ELi3ELb0E": True,
            "v6ILi1ELi0ELi3ELb0E": False, "v6ILi1ELi0ELi3ELb1E": False, "v6ILi1ELi0ELi2ELb0E": False}
    seen = set()
    for b in blocks:
        name = b.split()[0]
        hit = [k for k in want if "k_gru_steps_" + k in name]
        if not hit:
            continue
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        assert num(r"ScratchSize \[bytes/lane\]") == 0, name
        if want[hit[0]]:
            assert num("    VGPRs") + num("AGPRs") <= 512 and num(r"Occupancy \[waves/SIMD\]") == 1, name
        seen.add(hit[0])
    assert seen == set(want), sorted(set(want) - seen)
