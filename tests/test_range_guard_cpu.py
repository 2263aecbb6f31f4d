"""The range guard of the exact-operand eval kernels (status 7, ABI 8) on the host-fiber build of the real library.

An fp32 operand travels as fp16 limbs; a value of 65504 or more (NaN and inf included) turns its first limb into inf, and the pass
returns NaN / inf where the reference -- which simply computes -- is finite.  The kernels that BUILD limb operands raise status word
3 = 7 for it; passes that build none never do.  The out-of-range fixtures come from the reference itself
(tests/golden/make_golden_range.py); their allowance is the reference's own rounding noise on such input (range_util.allowance)."""
import os
import re

import numpy as np
import pytest
import torch

import _cabi
import range_util
import stacked_ref
import synth
from emu_util import NpNet, emu_lib, ptr
from stacked_util import GENERIC, NpDeepNet

EXACT = _cabi.FLAG_PERSISTENT | _cabi.FLAG_EXACT3
FP32 = _cabi.FLAG_PERSISTENT
RANGE, WORD = _cabi.STATUS_RANGE, _cabi.STATUS_RANGE_WORD


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def maxabs(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def forward(net, x, y_in, flags, h_in=None, clamp=-1):
    """One pass through the C ABI; returns (trj, the four status words of the pass's workspace)."""
    lib, d = net.lib, net.d
    x = np.ascontiguousarray(x, np.float32)
    B, T = x.shape[:2]
    y_in = np.ascontiguousarray(np.asarray(y_in).reshape(B, d.out_dim), np.float32)
    h_in = None if h_in is None else np.ascontiguousarray(np.asarray(h_in).reshape(B, d.hidden), np.float32)
    trj = np.full((B, T, d.out_dim), np.nan, np.float32)
    # garbage in the workspace, as a caller's torch.empty would hand over: the status must not depend on it
    ws = np.full(lib.pass_workspace_bytes(d, B, T) // 4, np.float32(7.0), np.float32)
    lib.gru_rnn_forward(d, ptr(net.prepared), lib.pass_input((ptr(x), x.shape[2], x.shape[2])), ptr(y_in), ptr(h_in), B, T, clamp,
                        ptr(trj), None, None, ptr(ws), ws.nbytes, flags)
    return trj, lib.workspace_status(ptr(ws))


def six_rows(P):
    """The fixture's three rows twice: rows are independent recurrences, and the exact-operand kernel takes passes of >= 4 rows
    (<= 3 rows run k_gru_steps_ll, which builds no limb operand)."""
    return np.concatenate([P.x, P.x]), np.concatenate([P.y_in_enc, P.y_in_enc])


def test_in_range_pass_and_chain_raise_nothing(lib):
    P = range_util.problem("h64")
    g = range_util.golden("h64")
    assert synth.sha256_state(P.enc) == str(g["sha_enc"])
    x, y = six_rows(P)
    enc = NpNet(lib, P.enc, 10, 8, 64)
    trj, st = forward(enc, x, y, EXACT, clamp=4)
    assert st[0] == 0 and st[WORD] == 0, st
    n, tol = range_util.allowance(g, "s1")
    d = maxabs(trj[:3], g["s1_f64"])
    print("h64 s1 exact kernels: n = %.3g, max|dev - ref64| = %.3g (allowed %.3g)" % (n, d, tol))
    assert d <= tol and np.array_equal(trj[:3], trj[3:])
    assert _chain_status(lib, P, P.dec, EXACT) == (0, 0)


def _chain_status(lib, P, dec_sd, flags, B=3):
    enc, dec = NpNet(lib, P.enc, 10, 8, 64), NpNet(lib, dec_sd, 6, 6, 64)
    T, L = P.T, P.lat_dim
    # four rows (the first row once more): the encoder passes of the chain then take the exact-operand kernel too
    rep = lambda a: np.ascontiguousarray(np.concatenate([a, a[:1]]))
    x, cvx, cs, ct = rep(P.x), rep(P.cvx), rep(P.code_src), rep(P.code_trg)
    ye, yd = rep(P.y_in_enc.reshape(B, 8)), rep(P.y_in_dec.reshape(B, 6))
    eps = np.ascontiguousarray(np.concatenate([P.eps, P.eps[:, :, :1]], 2))
    B = B + 1
    outs = {k: np.full((2, B, T, c), np.nan, np.float32) for k, c in (("lat", 8), ("rec", 6), ("cv", 6), ("latcv", 8), ("reccyc", 6))}
    ws = np.full(lib.cycle_workspace_bytes(enc.d, dec.d, B, T, 2) // 4, np.float32(3.0), np.float32)
    lib.cycle_forward(enc.d, ptr(enc.prepared), dec.d, ptr(dec.prepared), ptr(x), ptr(cvx), 4, ptr(cs), ptr(ct), 2, ptr(ye), ptr(yd),
                      B, T, 2, L, ptr(eps), 0, ptr(outs["lat"]), ptr(outs["rec"]), ptr(outs["cv"]), ptr(outs["latcv"]),
                      ptr(outs["reccyc"]), ptr(ws), ws.nbytes, flags)
    st = lib.workspace_status(ptr(ws))
    return st[0], st[WORD]


def test_out_of_range_input_is_raised_and_fp32_kernels_meet_the_reference(lib):
    """s = 1e5: max|x^| = 5.5e5.  Fails without the guard (no word is raised)."""
    P = range_util.problem("h64")
    g = range_util.golden("h64")
    x, y = six_rows(P)
    enc = NpNet(lib, range_util.scaled_encoder(P, 1e5), 10, 8, 64)
    trj, st = forward(enc, x, y, EXACT, clamp=4)
    assert st[WORD] == RANGE and st[0] == 0, st
    trj, st = forward(enc, x, y, FP32, clamp=4)
    assert st[WORD] == 0 and st[0] == 0, st
    n, tol = range_util.allowance(g, "s1e5")
    d = maxabs(trj[:3], g["s1e5_f64"])
    print("h64 s1e5 fp32 kernels: n = %.3g, max|dev - ref64| = %.3g (allowed %.3g)" % (n, d, tol))
    assert np.isfinite(trj).all() and d <= tol, (d, tol)
    # the same workspace again, in range: the raise of an earlier call is not reported for a later one
    ws_lib_in_range = NpNet(lib, P.enc, 10, 8, 64)
    assert forward(ws_lib_in_range, x, y, EXACT, clamp=4)[1][WORD] == 0


def test_band_between_2048_and_the_bound(lib, options):
    """s = 1e4: max|x^| = 5.5e4, inside the fp16 range and beyond the 2048 up to which the (fp16, fp16, bf8) triple is exact: the
    default bound lets it through and the result meets the reference within its own noise; exact_range_at = 2048 raises it."""
    P = range_util.problem("h64")
    g = range_util.golden("h64")
    x, y = six_rows(P)
    enc = NpNet(lib, range_util.scaled_encoder(P, 1e4), 10, 8, 64)
    trj, st = forward(enc, x, y, EXACT, clamp=4)
    assert st[WORD] == 0 and st[0] == 0, st
    n, tol = range_util.allowance(g, "s1e4")
    d = maxabs(trj[:3], g["s1e4_f64"])
    print("h64 s1e4 exact kernels: n = %.3g, max|dev - ref64| = %.3g (allowed %.3g)" % (n, d, tol))
    assert d <= tol, (d, tol)
    options(exact_range_at=2048)
    assert lib.get_option("exact_range_at") == 2048
    trj2, st = forward(enc, x, y, EXACT, clamp=4)
    assert st[WORD] == RANGE and st[0] == 0, st
    assert np.array_equal(trj, trj2)          # the bound changes what is reported, not what is computed
    in_range = NpNet(lib, P.enc, 10, 8, 64)
    assert forward(in_range, x, y, EXACT, clamp=4)[1][WORD] == 0       # max|x^| = 3.5 < 2048


def _noise_and_ref(sd, x, y, h_in=None, clamp=4):
    """fp64 and fp32 runs of the stock-torch restatement of the reference's pass (tests/stacked_ref.py): the fp64 result and the
    allowance max(5e-6, 4 n), n = the fp32 run's own distance from it."""
    hi = None if h_in is None else h_in[None]
    r64 = stacked_ref.forward(sd, x, y, hi, clamp_lat_dim=clamp)[0]
    r32 = stacked_ref.forward(sd, x, y, hi, clamp_lat_dim=clamp, dtype=torch.float32)[0]
    n = float(np.max(np.abs(r32.astype(np.float64) - r64)))
    return r64, n, max(5e-6, 4.0 * n)


def test_carried_in_state_beyond_the_bound(lib):
    P = range_util.problem("h64")
    x, y = six_rows(P)
    enc = NpNet(lib, P.enc, 10, 8, 64)
    h = (0.5 * synth.normal("rng64/h_in", (6, 64))).astype(np.float32)
    assert forward(enc, x, y, EXACT, h_in=h, clamp=4)[1][WORD] == 0
    h[1, 5] = 1e5
    st = forward(enc, x, y, EXACT, h_in=h, clamp=4)[1]
    assert st[WORD] == RANGE and st[0] == 0, st
    h[1, 5] = np.nan                                   # NaN and inf count as out of range
    assert forward(enc, x, y, EXACT, h_in=h, clamp=4)[1][WORD] == RANGE
    h[1, 5] = 1e5
    # <= 3 rows: k_gru_steps_ll multiplies the fp32 state itself -- nothing to raise, and the result is the reference's
    trj, st = forward(enc, x[:3], y[:3], EXACT, h_in=h[:3], clamp=4)
    assert st[WORD] == 0 and st[0] == 0, st
    r64, n, tol = _noise_and_ref(P.enc, x[:3], y[:3], h[:3])
    d = maxabs(trj, r64)
    print("h64 h_in = 1e5 on k_gru_steps_ll: n = %.3g, max|dev - ref64| = %.3g (allowed %.3g)" % (n, d, tol))
    assert np.isfinite(trj).all() and d <= tol, (d, tol)


def test_weight_beyond_the_fp16_range(lib):
    P = range_util.problem("h64")
    x, y = six_rows(P)
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["gru.weight_hh_l0"][64 + 7, 3] = 1e5            # one recurrent weight of the z gate
    enc = NpNet(lib, sd, 10, 8, 64)
    ok = NpNet(lib, P.enc, 10, 8, 64)
    assert lib.net_prepared_in_range(ok.d, 1, ptr(ok.prepared)) is True
    # before anybody asked, a pass on the limb kernels raises the status (the prologue reads the image's flag) ...
    other = lib.new_context()
    st = forward(_with_lib(enc, other), x, y, EXACT, clamp=4)[1]
    other.close()
    assert st[WORD] == RANGE, st
    # ... once asked, the context runs that image on the fp32-operand kernels whatever flags it is given
    assert lib.net_prepared_in_range(enc.d, 1, ptr(enc.prepared)) is False
    trj, st = forward(enc, x, y, EXACT | _cabi.FLAG_SPLIT_F16, clamp=4)
    assert st[WORD] == 0 and st[0] == 0, st
    trj32, st = forward(enc, x, y, FP32, clamp=4)
    assert np.array_equal(trj, trj32) and np.isfinite(trj).all()
    r64, n, tol = _noise_and_ref(sd, x, y)
    d = maxabs(trj, r64)
    print("h64 W_hh entry 1e5: n = %.3g, max|dev - ref64| = %.3g (allowed %.3g)" % (n, d, tol))
    assert d <= tol, (d, tol)
    # a rebuilt image at the same address is asked about again
    enc2 = NpNet(lib, P.enc, 10, 8, 64)
    wp = {f: ptr(enc2.sd[k]) for f, k in _cabi.STATE_KEYS.items() if k in enc2.sd}
    scratch = np.zeros(lib.prepare_scratch_bytes(enc.d) // 8 + 1, np.float64)
    lib.net_prepare(enc.d, wp, ptr(enc.prepared), enc.prepared.nbytes, ptr(scratch), scratch.nbytes)
    assert lib.net_prepared_in_range(enc.d, 1, ptr(enc.prepared)) is True
    assert np.array_equal(forward(enc, x, y, EXACT, clamp=4)[0], forward(ok, x, y, EXACT, clamp=4)[0])


class _with_lib(object):
    """An NpNet's image driven through another context of the same library."""

    def __init__(self, net, lib):
        self.lib, self.d, self.prepared = lib, net.d, net.prepared


def test_chain_raises_where_an_intermediate_leaves_the_range(lib):
    """The decoder's scale_out bias lifts one channel of rec / cv to 1e6; no decoder pass has anything to report (its input is the
    code and the latent draw), the NEXT encoder pass re-normalises [cvx ; cv] and its prologue -- a pass that does not clear the
    status words, raising with the serial number of the call -- reports it.  The in-range chain on the same networks is clean (test_in_range_pass_and_chain_raise_nothing)."""
    P = range_util.problem("h64")
    dec = {k: v.copy() for k, v in P.dec.items()}
    dec["scale_out.bias"][1] = 1e6          # the bias only: the folded projection scale_out . out_1 -- the decoder IMAGE -- stays in range
    image = NpNet(lib, dec, 6, 6, 64)
    assert lib.net_prepared_in_range(image.d, 1, ptr(image.prepared)) is True
    assert _chain_status(lib, P, dec, EXACT) == (0, RANGE)
    assert _chain_status(lib, P, dec, FP32) == (0, 0)


@pytest.mark.parametrize("L", [2])
def test_stacked_network_checks_the_carried_in_states(lib, L):
    """hidden_layers = 2: layer 0's input side is an fp32 GEMM, so of the exchanged values only h_in takes the limb form (resident
    kernel); the any-H kernel multiplies fp32 operands and raises nothing."""
    P = synth.CycleVAEProblem(B=3, T=8, in_dim=10, out_dim=6, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1, tag="rngstk", hidden_layers=L)
    net = NpDeepNet(lib, P.enc, 10, 8, 64, L)
    assert lib.net_prepared_in_range(net.d, L, ptr(net.prepared)) is True
    h = (0.5 * synth.normal("rngstk/h_in", (L, 3, 64))).astype(np.float32)

    def status(h_in, flags):
        x = np.ascontiguousarray(P.x)
        y = np.ascontiguousarray(P.y_in_enc.reshape(3, 8))
        trj = np.full((3, 8, 8), np.nan, np.float32)
        ws = np.full(lib.pass_workspace_bytes_deep(net.d, L, 3, 8) // 4, np.float32(5.0), np.float32)
        lib.gru_rnn_forward_deep(net.d, L, ptr(net.prepared), lib.pass_input((ptr(x), 10, 10)), ptr(y), ptr(h_in), 3, 8, 4, ptr(trj),
                                 None, None, ptr(ws), ws.nbytes, flags)
        return lib.workspace_status(ptr(ws)), trj

    assert lib.plan_pass_deep(net.d, L, 3, 8, _cabi.FLAG_PERSISTENT) == 2          # the resident exact-operand kernel
    st, _ = status(h, _cabi.FLAG_PERSISTENT)
    assert st[0] == 0 and st[WORD] == 0, st
    h[0, 2, 9] = -1e5                                       # layer 0's state: only k_deep_slot0 sees it
    st, _ = status(h, _cabi.FLAG_PERSISTENT)
    assert st[0] == 0 and st[WORD] == RANGE, st
    st, trj = status(h, GENERIC)
    assert st[0] == 0 and st[WORD] == 0 and np.isfinite(trj).all(), st
    # a weight of an upper layer beyond the range: the image is unfit, its passes take the any-H kernel by themselves
    sd = {k: v.copy() for k, v in P.enc.items()}
    sd["gru.weight_ih_l1"][5, 5] = 7e4
    bad = NpDeepNet(lib, sd, 10, 8, 64, L)
    assert lib.net_prepared_in_range(bad.d, L, ptr(bad.prepared)) is False
    a = bad.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=_cabi.FLAG_PERSISTENT)[0]
    b = bad.forward(P.x, P.y_in_enc, clamp_lat_dim=4, flags=GENERIC)[0]
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_limb_window_over_binades(lib):
    """cvae_selftest_limbs swept over binades -- the figures of DESIGN.md 4.1: the transported triple (fp16, fp16, bf8) gives x back
    bit for bit for every |x| < 2048 (the bf8 clamp at 57344 does not engage: the third limb times 2^6 is at most 2^15); in
    [2048, 65504) the clamped byte costs at most one fp32 ulp, 2^-23 relative; from 65520 on the first limb is inf."""
    rng = np.random.default_rng(20190721)
    worst = 0.0
    for b in range(-14, 16):
        x = rng.uniform(2.0 ** b, 2.0 ** (b + 1), 40000).astype(np.float32)
        x[:4] = np.float32([2.0 ** b, np.nextafter(np.float32(2.0 ** (b + 1)), np.float32(0)), 1.5 * 2.0 ** b, 1.75 * 2.0 ** b])
        x *= rng.choice(np.float32([-1, 1]), x.size)
        y = np.zeros_like(x)
        lib.selftest_limbs(ptr(x), ptr(y), x.size)
        fits = np.abs(x) < 65504
        assert np.isfinite(y[fits]).all()
        rel = np.abs((y[fits].astype(np.float64) - x[fits]) / x[fits])
        if b < 11:
            assert rel.max() == 0.0, (b, rel.max())
        else:
            worst = max(worst, float(rel.max()))
    print("worst relative error of the transported triple in [2048, 65504): %.4g" % worst)
    assert 0.0 < worst <= 2.0 ** -23, worst                 # 1.19e-7
    x = np.float32([65520, 65536, 1e5, 3e38, -65520, -1e6, np.inf, np.nan])
    y = np.zeros_like(x)
    lib.selftest_limbs(ptr(x), ptr(y), x.size)
    assert not np.isfinite(y).any(), y
    x = np.float32([65504, -65504, 65519.99, 60000, 2048, 4096, 0, 1])
    lib.selftest_limbs(ptr(x), ptr(y), x.size)
    assert np.isfinite(y).all() and np.max(np.abs(y - x)) <= 16.0, y       # [65504, 65520) rounds to the largest half


def test_guarded_kernels_do_not_spill():
    """The kernels the guard touches (prologue, slot-0 fill of the stacked path, the prepare kernels that write limb images) use no
    scratch in the shipped build."""
    import __graft_entry__
    lib = os.path.join(__graft_entry__.PKG, "libcyclevae_hip.so")
    if not os.path.exists(__graft_entry__.RESOURCES) or os.path.getmtime(__graft_entry__.RESOURCES) < os.path.getmtime(lib):
        __graft_entry__.build(force=True)
    text = open(__graft_entry__.RESOURCES).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", text)[1:]
    want = ("k_prologue", "k_deep_slot0", "k_prep_wrec3", "k_prep_afold3l", "k_prep_wo3", "k_prep_wrec_h", "k_prep_afold_h", "k_prep_wrec_deep")
    seen = set()
    for b in blocks:
        name = b.split()[0]
        hit = [k for k in want if k in name]
        if not hit:
            continue
        seen.update(hit)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, "%s spills %d bytes per lane" % (name, scratch)
    assert seen == set(want), set(want) - seen


def test_status_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cyclevae_hip.h")).read()
    assert int(re.search(r"#define CVAE_STATUS_RANGE (\d+)", text).group(1)) == _cabi.STATUS_RANGE
    assert int(re.search(r"#define CVAE_STATUS_RANGE_WORD (\d+)", text).group(1)) == _cabi.STATUS_RANGE_WORD
    assert issubclass(_cabi.CvaeRangeError, _cabi.CvaeError)


def test_python_policies_on_the_emulator():
    """check_status -> CvaeRangeError, the lagged contract, word 0 and word 3 side by side, set_range_policy("retry") in
    GRU_RNN.forward and stage6.convert_pairs, and the image query of _Prepared: the drop-in module on the host-fiber build with a
    status sink in host memory, in a process of its own (tests/emu_range_policy.py)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "emu_range_policy.py")], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RANGE_POLICY_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_pair_flag_without_the_pair_kernel_raises_nothing(lib):
    """CVAE_FLAG_SPLIT_F16 on a geometry k_gru_steps_v5 is not built for (H = 64 with a 10-channel input: KFW = 3): the pass runs an
    fp32-operand kernel, so the out-of-range input is simply computed on.  On a geometry the pair kernel takes (6 channels: KFW = 2)
    the same flag reports it."""
    P = range_util.problem("h64")
    g = range_util.golden("h64")
    x, y = six_rows(P)
    enc = NpNet(lib, range_util.scaled_encoder(P, 1e5), 10, 8, 64)
    trj, st = forward(enc, x, y, _cabi.FLAG_PERSISTENT | _cabi.FLAG_SPLIT_F16, clamp=4)
    assert st[WORD] == 0 and st[0] == 0, st
    n, tol = range_util.allowance(g, "s1e5")
    assert maxabs(trj[:3], g["s1e5_f64"]) <= tol
    Q = synth.CycleVAEProblem(B=6, T=8, in_dim=6, out_dim=4, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.05, tag="rngpair")
    sd = {k: v.copy() for k, v in Q.enc.items()}
    sd["scale_in.weight"][2, 2, 0] *= np.float32(1e5)
    pair = NpNet(lib, sd, 6, 8, 64)
    assert forward(pair, Q.x, Q.y_in_enc, _cabi.FLAG_PERSISTENT | _cabi.FLAG_SPLIT_F16, clamp=4)[1][WORD] == RANGE
    assert forward(pair, Q.x, Q.y_in_enc, FP32, clamp=4)[1][WORD] == 0
    assert forward(NpNet(lib, Q.enc, 6, 8, 64), Q.x, Q.y_in_enc, _cabi.FLAG_PERSISTENT | _cabi.FLAG_SPLIT_F16, clamp=4)[1][WORD] == 0
