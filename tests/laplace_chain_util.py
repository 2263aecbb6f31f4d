"""Case table of the Laplace-posterior tests (tests/test_laplace_chain_cpu.py, tests/test_laplace_chain_gpu.py): the shapes and synth
seeds the golden was recorded at (tests/golden/make_golden_laplace_chain.py), the eps of the cases that have no golden, and the bounds.

Bounds: the project's own, unchanged (tests/stacked_util.py through tests/frontend_util.py), with frontend_util.bound_for on every
recorded output; the training bounds are those tests/test_gpu_train.py holds the Gaussian step to.

The fixture.  The Laplace clamp floors the encoder's log-scales at FLOOR; the golden problem must have log-scales exactly on the floor
and log-scales above it, so its biases are drawn from U(+-BIAS_SCALE) with BIAS_SCALE = 8: with the synth seed of TAG the four
log-scale biases of the encoder's out_1 are (-1.83, -2.78, -2.30, -7.75) -- the last one sits below the floor, the others above, and no
scale exp(s) is large.  tests/test_laplace_chain_cpu.py asserts both conditions (and both signs among the recorded eps) on the file."""
import numpy as np

import synth
from frontend_util import H64 as _H64

FLOOR = -7.2543288692621097        # clamp_vae_laplace (reference gru_vae.py:417)
TAG, BIAS_SCALE = "lapchain8", 8.0
H64 = dict(_H64, bias_scale=BIAS_SCALE)          # B 5, T 12, in 30, out 26, lat_dim 4, hidden 64, n_cyc 2
N_SMPL = 3                                       # draws of the stage-6 latent mean
KEYS = ("lat", "rec", "cv", "latcv", "reccyc")
LOSS_ROWS = ((False, None, None), (False, [0, 2], [5, 3, 9]), (True, [1], [4, 4, 4]), (False, [1], [2, 6, 1]))   # (half, select, flen_acc): tests/test_emu_train.py:181
TRAIN_LOSS_REL = 1e-5              # loss against the float64 reference (tests/test_gpu_train.py)
TRAIN_GRAD_REL = 2e-6              # flat gradient between the step forms


def problem_h64():
    return synth.CycleVAEProblem(tag=TAG, **H64)


def problem_h1024(B=4, T=12, tag="lapchain1024"):
    return synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag=tag)


def problem_train_h64(B=3, T=10):
    return synth.CycleVAEProblem(B=B, T=T, in_dim=30, out_dim=26, lat_dim=4, hidden=64, n_cyc=2, bias_scale=0.1, tag="laptrain64")


def uniform_eps(tag, shape):
    """eps as sampling_vae_laplace draws it: U(-0.4999, 0.5)."""
    return synth.uniform(tag, shape, -0.4999, 0.5, synth.SEED)


def stage6_pair(P, T=12, tag=TAG):
    """One (source, target) utterance pair of T frames each for the problem's nets, and the y_in of the stage-6 statements."""
    fs = synth.features(tag + "/s6src", 1, T, P.mu, P.sigma)[0]
    ft = synth.features(tag + "/s6trg", 1, T, P.mu, P.sigma)[0]
    y_pp = np.zeros((1, 1, 2 * P.lat_dim), np.float32)
    return fs, ft, y_pp, P.y_in_dec[:1].copy()


# ---- the checks, shared by the emulator (CPU tensors, gru_vae bound to the emulator build) and the device tests ----------------
def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def module(gv, sd, in_dim, out_dim, hidden, enc, dev, layers=1, train=False):
    import torch
    m = gv.GRU_RNN(in_dim=in_dim, out_dim=out_dim, hidden_units=hidden, hidden_layers=layers, kernel_size=3, dilation_size=2,
                   do_prob=0.5 if train else 0, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev)
    return m.train() if train else m.eval()


def modules(gv, P, dev, layers=1, train=False):
    return (module(gv, P.enc, P.in_dim, 2 * P.lat_dim, P.hidden, True, dev, layers, train),
            module(gv, P.dec, P.lat_dim + 2, P.out_dim, P.hidden, False, dev, layers, train))


def run_pass(gv, mod, seg0, y_in, clamp=-1, seg1=None, lat=None, lat_dim=0, eps=None, seed=0, draw_id=0, n_draws=0):
    """One eval pass straight through the C ABI (cvae_gru_rnn_forward_deep) on the module's prepared image: [seg0 ; seg1 | draw]."""
    import torch
    lib, dev = gv._lib(), seg0.device
    B, T_, w0 = seg0.shape
    d, image = mod.prepared(dev)
    ws = mod._prep.workspace(B, T_, dev)
    s1 = None if seg1 is None else (seg1.data_ptr(), seg1.shape[2], seg1.shape[2])
    pin = lib.pass_input((seg0.data_ptr(), w0, w0), s1, None if lat is None else lat.data_ptr(), lat_dim,
                         None if eps is None else eps.data_ptr(), seed=seed, draw_id=draw_id, n_draws=n_draws)
    y0 = y_in.reshape(B, mod.out_dim).contiguous()
    trj = torch.full((B, T_, mod.out_dim), float("nan"), dtype=torch.float32, device=dev)
    lib.gru_rnn_forward_deep(d, mod.hidden_layers, image.data_ptr(), pin, y0.data_ptr(), None, B, T_, clamp, trj.data_ptr(), None, None,
                             ws.data_ptr(), ws.numel(), gv._flags(mod.hidden_layers), gv._stream())
    return trj


def sample_laplace(gv, lat, L, eps=None, seed=0, draw_id=0):
    """cvae_sample_laplace on lat [B,T,2L] -> z [B,T,L]."""
    import torch
    z = torch.empty(lat.shape[:-1] + (L,), dtype=torch.float32, device=lat.device)
    gv._lib().sample_laplace(lat.data_ptr(), lat.numel() // (2 * L), L, None if eps is None else eps.data_ptr(), seed, draw_id,
                             z.data_ptr(), None, gv._stream())
    return z


def chain_by_passes(gv, enc, dec, P, dev, seed, n_cyc=2):
    """The fresh chain composed pass by pass, the draws inside the decoder passes' prologues with the chain's ids 3i + k."""
    import _cabi
    L = P.lat_dim
    x, cvx, cs, ct, ye, yd = (T(a, dev) for a in (P.x, P.cvx, P.code_src, P.code_trg, P.y_in_enc, P.y_in_dec))
    Ld, cl = L | _cabi.DRAW_LAPLACE, L | _cabi.CLAMP_LAPLACE
    out = {k: [] for k in KEYS}
    prev = None
    for i in range(n_cyc):
        lat = run_pass(gv, enc, x, ye, cl) if i == 0 else run_pass(gv, enc, x[:, :, :P.stdim].contiguous(), ye, cl, seg1=prev)
        rec = run_pass(gv, dec, cs, yd, lat=lat, lat_dim=Ld, seed=seed, draw_id=3 * i)
        cv = run_pass(gv, dec, ct, yd, lat=lat, lat_dim=Ld, seed=seed, draw_id=3 * i + 1)
        latcv = run_pass(gv, enc, cvx, ye, cl, seg1=cv)
        prev = run_pass(gv, dec, cs, yd, lat=latcv, lat_dim=Ld, seed=seed, draw_id=3 * i + 2)
        for k, v in zip(KEYS, (lat, rec, cv, latcv, prev)):
            out[k].append(v)
    import torch
    return {k: torch.stack(v) for k, v in out.items()}


def chain_args(P, dev):
    return [T(a, dev) for a in (P.x, P.cvx, P.code_src, P.code_trg, P.y_in_enc, P.y_in_dec)]


def np_u(e):
    e = np.asarray(e, np.float64)
    return -np.sign(e) * np.log1p(-2.0 * np.abs(e))


def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "laplace_chain.npz"))


def check_pass_supplied_eps(gv, dev, G, base):
    """1. a decoder pass that draws z = mu + exp(s) u(eps) in its prologue from the recorded latent and eps, against the golden."""
    import _cabi
    from frontend_util import bound_for
    P = problem_h64()
    dec = modules(gv, P, dev)[1]
    lat, eps = T(G["chain_lat"][0], dev), T(G["chain_eps"][0, 0], dev)
    rec = run_pass(gv, dec, T(P.code_src, dev), T(P.y_in_dec, dev), lat=lat, lat_dim=P.lat_dim | _cabi.DRAW_LAPLACE, eps=eps)
    d = maxdiff(N(rec), G["chain_rec"][0])
    print("pass, supplied eps: max|d| = %.3e (bound %.3e)" % (d, bound_for(G, "chain_rec", base)))
    assert d <= bound_for(G, "chain_rec", base)
    # and bit for bit the pass that is fed [code ; z] with z from cvae_sample_laplace on the same eps
    fed = run_pass(gv, dec, T(P.code_src, dev), T(P.y_in_dec, dev), seg1=sample_laplace(gv, lat, P.lat_dim, eps))
    assert np.array_equal(N(rec), N(fed))


def check_pass_philox(gv, dev, L):
    """1. the in-pass Philox draw equals cvae_sample_laplace with the same (seed, draw_id, frame, dim) bit for bit: the pass gives
    the outputs of a pass fed [code ; z].  L = 6: the lat_dim that is no multiple of four."""
    import _cabi
    B, T_, H, Co = 5, 12, 64, 26
    sd = synth.gru_rnn_state("lappass%d/dec" % L, L + 2, Co, H, scale_out=synth.feature_stats("lappass%d/stats" % L, Co), bias_scale=0.1)
    dec = module(gv, sd, L + 2, Co, H, False, dev)
    lat = 0.7 * synth.normal("lappass%d/lat" % L, (B, T_, 2 * L))
    code, y = synth.onehot_codes(B, T_)[0], np.zeros((B, 1, Co), np.float32)
    latd, coded, yd = T(lat, dev), T(code, dev), T(y, dev)
    for kw in (dict(seed=1234, draw_id=5), dict(eps=T(uniform_eps("lappass%d/eps" % L, (B, T_, L)), dev))):
        a = run_pass(gv, dec, coded, yd, lat=latd, lat_dim=L | _cabi.DRAW_LAPLACE, **kw)
        z = sample_laplace(gv, latd, L, **kw)
        b = run_pass(gv, dec, coded, yd, seg1=z)
        assert np.all(np.isfinite(N(a))) and np.array_equal(N(a), N(b)), sorted(kw)
        zr = lat[..., :L].astype(np.float64) + np.exp(lat[..., L:].astype(np.float64)) * np_u(N(kw["eps"])) if "eps" in kw else None
        assert zr is None or maxdiff(N(z), zr) <= 2e-6 * max(1.0, float(np.abs(zr).max()))
    # the Gaussian draw of the same pass differs: the flag is what switches
    g = run_pass(gv, dec, coded, yd, lat=latd, lat_dim=L, seed=1234, draw_id=5)
    assert not np.array_equal(N(a), N(g))


def check_chain_golden(gv, dev, G, base):
    """2. fresh form: all five trajectories of both cycles against the golden; carry form: two 6-frame windows against the
    reference's windowed composition."""
    from frontend_util import bound_for
    P = problem_h64()
    enc, dec = modules(gv, P, dev)
    chain = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior="laplace")
    args = chain_args(P, dev)
    out = chain(*args, eps=T(G["chain_eps"], dev))
    for k in KEYS:
        d = maxdiff(N(out[k]), G["chain_" + k])
        print("chain %-7s max|d| = %.3e (bound %.3e)" % (k, d, bound_for(G, "chain_" + k, base)))
        assert d <= bound_for(G, "chain_" + k, base), k
    s = N(out["lat"])[..., P.lat_dim:]
    assert np.any(s == np.float32(FLOOR)) and np.all(s >= np.float32(FLOOR))       # the Laplace floor, not ln(1e-6)
    eps = G["carry_eps"]
    win = lambda a, b: [v[:, a:b].contiguous() for v in args[:4]] + args[4:]
    oa, st = chain(*win(0, 6), eps=T(eps[:, :, :, 0:6], dev), return_state=True)
    ob = chain(*win(6, 12), eps=T(eps[:, :, :, 6:12], dev), state=st)
    for k in KEYS:
        d = maxdiff(np.concatenate((N(oa[k]), N(ob[k])), 2), G["carry_" + k])
        print("carry %-7s max|d| = %.3e (bound %.3e)" % (k, d, bound_for(G, "carry_" + k, base)))
        assert d <= bound_for(G, "carry_" + k, base), k


def check_chain_philox(gv, dev, kernels, layers=1, P=None):
    """2. / 3. the chain with Philox draws equals the pass-by-pass composition with the draw ids 3i + k."""
    P = problem_h64() if P is None else P
    enc, dec = modules(gv, P, dev, layers)
    out = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior="laplace")(*chain_args(P, dev), seed=77)
    ref = chain_by_passes(gv, enc, dec, P, dev, 77, P.n_cyc)
    for k in KEYS:
        d = maxdiff(N(out[k]), N(ref[k]))
        print("philox chain (%d layers) %-7s max|d| = %.3e" % (layers, k, d))
        assert np.all(np.isfinite(N(out[k]))) and d <= kernels, k
    # other draws than the Gaussian chain's with the same seed
    g = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc)(*chain_args(P, dev), seed=77)
    assert not np.array_equal(N(g["rec"]), N(out["rec"]))


def check_chain_default(gv, dev):
    """2. posterior="gauss" is the default call bit for bit."""
    P = problem_h64()
    enc, dec = modules(gv, P, dev)
    a = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc)(*chain_args(P, dev), eps=T(P.eps, dev))
    b = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior="gauss")(*chain_args(P, dev), eps=T(P.eps, dev))
    for k in KEYS:
        assert np.array_equal(N(a[k]), N(b[k])), k


def check_stage6_golden(gv, dev, G, base):
    """4. convert_pair(posterior="laplace", n_smpl_dec=3) with supplied eps [3,T,L] against the golden (B = 1 rows: cvae_mean_draws)."""
    import stage6
    from frontend_util import bound_for
    P = problem_h64()
    enc, dec = modules(gv, P, dev)
    fs, ft, y_pp, y_dec = stage6_pair(P)
    res = stage6.convert_pair(enc, dec, T(fs, dev), T(ft, dev), T(y_pp, dev), T(y_dec, dev), T(y_dec, dev), P.lat_dim, n_smpl_dec=N_SMPL,
                              eps_src=T(G["s6_eps_src"], dev), eps_trg=T(G["s6_eps_trg"], dev), posterior="laplace")
    for v, k in zip(res, ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg")):
        d = maxdiff(N(v), G["s6_" + k])
        print("stage 6 %-10s max|d| = %.3e (bound %.3e)" % (k, d, bound_for(G, "s6_" + k, base)))
        assert d <= bound_for(G, "s6_" + k, base), k


def check_latent_mean(gv, dev, L, n=3, frames=(1, 7, 33)):
    """4. cvae_latent_mean with the flag against numpy: out = mu + exp(s) * mean_k u(eps_k)."""
    import torch
    import _cabi
    lib = gv._lib()
    jobs, keep = [], []
    for q, fr in enumerate(frames):
        lat = 0.7 * synth.normal("laplm%d/lat%d" % (L, q), (fr, 2 * L))
        eps = uniform_eps("laplm%d/eps%d" % (L, q), (n, fr, L))
        out = torch.full((fr + 1, L), 7.0, dtype=torch.float32, device=dev)
        ld, ed = T(lat, dev), T(eps, dev)
        keep.append((lat, eps, out, ld, ed))
        jobs.append(_cabi.LatMeanJob(ld.data_ptr(), ed.data_ptr(), 0, fr, 0, out.data_ptr()))
    lib.latent_mean(jobs, L | _cabi.DRAW_LAPLACE, n, 0, gv._stream())
    for lat, eps, out, _, _ in keep:
        ref = lat[:, :L].astype(np.float64) + np.exp(lat[:, L:].astype(np.float64)) * np_u(eps).mean(0)
        o = N(out)
        assert np.all(o[-1] == 7.0)                     # the row behind the job's frames is untouched
        assert maxdiff(o[:-1], ref) <= 2e-6 * max(1.0, float(np.abs(ref).max()))
    # Philox: the same numbers as the single draws of cvae_sample_laplace with ids draw_id .. draw_id + n - 1, frame = t
    lat, _, out, ld, _ = keep[-1]
    fr = lat.shape[0]
    lib.latent_mean([_cabi.LatMeanJob(ld.data_ptr(), None, 4, fr, 0, out.data_ptr())], L | _cabi.DRAW_LAPLACE, n, 99, gv._stream())
    zs = np.stack([N(sample_laplace(gv, ld.reshape(1, fr, 2 * L), L, seed=99, draw_id=4 + k))[0] for k in range(n)]).astype(np.float64)
    assert maxdiff(N(out)[:-1], zs.mean(0)) <= 2e-6 * max(1.0, float(np.abs(zs).max()))


def check_sample_cat(gv, dev, parts):
    """5. cvae_sample_cat and its backward with the flag against torch autograd in float64; one eps is exactly 0."""
    import torch
    import _cabi
    lib = gv._lib()
    B, T_, L, nc = 3, 7, 6, 2
    lat = 0.7 * synth.normal("lapsc/lat", (B, T_, 2 * L))
    codes = [synth.normal("lapsc/code%d" % p, (B, T_, nc)) for p in range(parts)]
    eps = [uniform_eps("lapsc/eps%d" % p, (B, T_, L)) for p in range(parts)]
    eps[0][1, 2, 3] = 0.0
    dout = synth.normal("lapsc/dout", (parts * B, T_, nc + L))
    lt = torch.from_numpy(lat.astype(np.float64)).requires_grad_(True)
    et = [torch.from_numpy(e.astype(np.float64)) for e in eps]
    ref = torch.cat([torch.cat((torch.from_numpy(c.astype(np.float64)), lt[..., :L] - torch.exp(lt[..., L:]) * torch.sign(e) *
                                torch.log1p(-2 * e.abs())), 2) for c, e in zip(codes, et)], 0)
    ref.backward(torch.from_numpy(dout.astype(np.float64)))
    latd, cd, ed, dd = T(lat, dev), [T(c, dev) for c in codes], [T(e, dev) for e in eps], T(dout, dev)
    out = torch.empty(parts * B, T_, nc + L, dtype=torch.float32, device=dev)
    used = torch.empty(parts, B, T_, L, dtype=torch.float32, device=dev)
    dlat = torch.empty(B, T_, 2 * L, dtype=torch.float32, device=dev)
    lib.sample_cat(latd.data_ptr(), [c.data_ptr() for c in cd], [e.data_ptr() for e in ed], 0, list(range(parts)), B, T_,
                   L | _cabi.DRAW_LAPLACE, nc, out.data_ptr(), used.data_ptr(), gv._stream())
    lib.sample_cat_backward(dd.data_ptr(), latd.data_ptr(), used.data_ptr(), B, T_, L | _cabi.DRAW_LAPLACE, nc, parts, dlat.data_ptr(),
                            gv._stream())
    assert np.array_equal(N(used), np.stack(eps))
    rf, rg = ref.detach().numpy(), lt.grad.numpy()
    assert maxdiff(N(out), rf) <= 2e-6 * max(1.0, float(np.abs(rf).max()))
    assert maxdiff(N(dlat), rg) <= 2e-6 * max(1.0, float(np.abs(rg).max()))
    assert N(out)[1, 2, nc + 3] == np.float32(lat[1, 2, 3]) and np.isfinite(N(dlat)).all()      # eps = 0: z = mu
    # Philox: the eps it reports are cvae_sample_laplace's uniforms, the draw is made from them
    lib.sample_cat(latd.data_ptr(), [c.data_ptr() for c in cd], [None] * parts, 31, [5 + p for p in range(parts)], B, T_,
                   L | _cabi.DRAW_LAPLACE, nc, out.data_ptr(), used.data_ptr(), gv._stream())
    for p in range(parts):
        z = sample_laplace(gv, latd, L, seed=31, draw_id=5 + p)
        assert np.array_equal(N(out)[p * B:(p + 1) * B, :, nc:], N(z)), p
        u = N(used)[p]
        assert u.min() >= -0.4999 and u.max() < 0.5 and (u < 0).any() and (u > 0).any()


def check_stage4_loss(gv, dev, half, select, flen_acc):
    """6. cvae_stage4_loss with the flag (value and the four gradients) against torch in float64; one mu is exactly 0."""
    import torch
    import _cabi
    import stage4
    import laplace_chain_ref as R
    lib = gv._lib()
    B, T_, D, L, std = 3, 6, 5, 4, 2
    x = synth.normal("laps4/x", (B, T_, std + D))
    tr = {k: np.ascontiguousarray(0.7 * synth.normal("laps4/" + k, (B, T_, D if k in ("rec", "cv", "reccyc") else 2 * L)), np.float32)
          for k in KEYS}
    tr["lat"][0, 0, 1] = 0.0
    tr["latcv"][B - 1, 0, 0] = 0.0
    tt = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in tr.items()}
    ref = R.loss_terms([tt], torch.from_numpy(x.astype(np.float64)), std, L, flen_acc, select, half)
    ref.backward()
    ref = float(ref.detach())
    w, last, n_sel = stage4.frame_weights(B, T_, flen_acc, select)
    full = (not half) and n_sel > 0
    d = {k: T(v, dev) for k, v in tr.items()}
    g = {k: torch.full(tr[k].shape, float("nan"), dtype=torch.float32, device=dev) for k in ("rec", "reccyc", "lat", "latcv")}
    fl, loss = torch.zeros(B * T_, dtype=torch.float32, device=dev), torch.full((1,), 123.0, dtype=torch.float32, device=dev)
    xd, wd, ld = T(x, dev), T(np.asarray(w), dev), T(np.asarray(last), dev)
    p = lambda t_, on=True: t_.data_ptr() if on else None
    lib.stage4_loss(p(d["rec"]), p(d["reccyc"], full), p(d["lat"]), p(d["latcv"], full), xd.data_ptr(), std + D, std, wd.data_ptr(),
                    ld.data_ptr(), 2.0 if (full and n_sel > 1) else 1.0, B, T_, D, L | _cabi.DRAW_LAPLACE, p(g["rec"]), p(g["reccyc"], full),
                    p(g["lat"]), p(g["latcv"], full), fl.data_ptr(), loss.data_ptr(), False, gv._stream())
    assert abs(float(N(loss)[0]) - ref) <= 2e-6 * abs(ref)
    for k in ("rec", "lat") + (("reccyc", "latcv") if full else ()):
        assert maxdiff(N(g[k]), tt[k].grad.numpy()) <= 2e-6, k
    assert N(g["lat"])[0, 0, 1] == 0.0                     # sign(0) = 0, as torch.abs differentiates
    # the vectorised torch form of the unfused step is the same number
    t32 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in tr.items()}
    lt = stage4.loss_terms([t32], torch.from_numpy(x.astype(np.float64)), std, L, flen_acc, select, half, posterior="laplace")
    assert abs(float(lt) - ref) <= 1e-6 * max(1.0, abs(ref))       # (its frame weights 1 / n are float32)


def check_chain_f64(gv, dev, base, P=None):
    """3. the fresh chain at H = 1024 (B 4: the two cells of the rec || cv pass share one half-empty 32-row tile of the exact-operand
    recurrence, whose prologue builds the tile's draws) against the float64 reference."""
    import laplace_chain_ref as R
    P = problem_h1024() if P is None else P
    eps = uniform_eps("lapchain1024/eps", P.eps.shape)
    enc, dec = modules(gv, P, dev)
    out = gv.CycleChain(enc, dec, P.lat_dim, P.n_cyc, posterior="laplace")(*chain_args(P, dev), eps=T(eps, dev))
    ref = R.chain(P, eps)
    worst = {}
    for k in KEYS:
        worst[k] = maxdiff(N(out[k]), ref[k])
        print("chain H%d %-7s max|d| vs float64 = %.3e" % (P.hidden, k, worst[k]))
    for k in KEYS:
        assert worst[k] <= base, (k, worst)


def check_stage6_f64(gv, dev, base, T_=12, window=None):
    """4. convert_pair at H = 1024 against the float64 reference; window: the windowed wavefront gives the same values bit for bit.
    (A window must exceed twice the front-end's reach of 4 frames and a sliver of at most 8 frames joins the window before it, so the
    12-frame pair cannot be cut: the windowed call takes a 20-frame pair in two windows of 10.)"""
    import stage6
    import laplace_chain_ref as R
    P = problem_h1024()
    enc, dec = modules(gv, P, dev)
    fs, ft, y_pp, y_dec = stage6_pair(P, T_, tag="lapchain1024/%d" % T_)
    es, et = (uniform_eps("lapchain1024/%d/s6eps%d" % (T_, q), (N_SMPL, T_, P.lat_dim)) for q in range(2))
    call = lambda **kw: stage6.convert_pair(enc, dec, T(fs, dev), T(ft, dev), T(y_pp, dev), T(y_dec, dev), T(y_dec, dev), P.lat_dim,
                                            n_smpl_dec=N_SMPL, eps_src=T(es, dev), eps_trg=T(et, dev), posterior="laplace", **kw)
    res = call(window=window) if window else call()
    ref = R.stage6(P, fs, ft, y_pp, y_dec, y_dec, es, et)
    for v, r, k in zip(res, ref, ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg")):
        d = maxdiff(N(v), r)
        print("stage 6 H1024 T%d window=%s %-10s max|d| vs float64 = %.3e" % (T_, window, k, d))
        assert d <= base, k
    if window:
        assert len(stage6._window_edges(T_, window, 4)) > 2
        for a, b in zip(res, call()):
            assert np.array_equal(N(a), N(b))


def check_stage6_pairs_f64(gv, dev, base):
    """4. two pairs in one convert_pairs call at H = 1024: six decoder rows, one 32-row tile of the exact-operand recurrence, whose
    prologue takes the mean of the tile's draws; each pair against the float64 reference of that pair alone."""
    import stage6
    import laplace_chain_ref as R
    P = problem_h1024()
    enc, dec = modules(gv, P, dev)
    pairs, eps, refs = [], [], []
    for T_ in (12, 20):
        fs, ft, y_pp, y_dec = stage6_pair(P, T_, tag="lapchain1024/%d" % T_)
        es, et = (uniform_eps("lapchain1024/%d/s6eps%d" % (T_, q), (N_SMPL, T_, P.lat_dim)) for q in range(2))
        pairs.append((T(fs, dev), T(ft, dev)))
        eps.append((T(es, dev), T(et, dev)))
        refs.append(R.stage6(P, fs, ft, y_pp, y_dec, y_dec, es, et))
    res = stage6.convert_pairs(enc, dec, pairs, T(y_pp, dev), T(y_dec, dev), T(y_dec, dev), P.lat_dim, n_smpl_dec=N_SMPL, eps=eps,
                               posterior="laplace")
    for q, (got, ref) in enumerate(zip(res, refs)):
        for v, r, k in zip(got, ref, ("cvmcep", "cvmcep_src", "cvmcep_trg", "lat_src", "lat_trg")):
            d = maxdiff(N(v), r)
            print("stage 6 H1024 two pairs, pair %d %-10s max|d| vs float64 = %.3e" % (q, k, d))
            assert d <= base, (q, k)


def train_problem(hidden):
    """The step's problem: the last log-scale bias of the encoder is put below the Laplace floor, so that the clamp -- and the zero
    gradient under it -- is part of the step; every other bias stays small."""
    P = problem_train_h64() if hidden == 64 else problem_h1024(tag="laptrain1024")
    P.enc["out_1.bias"][-1] = -7.75
    return P, uniform_eps("laptrain%d/eps" % hidden, P.eps.shape)


def reference_step(P, eps):
    import laplace_chain_ref as R
    from train_util import make_masks
    masks = make_masks(P, 4, 6, tag="lapmasks")
    return masks, R.step(P, eps, masks)


def check_step(gv, dev, P, eps, masks_np, ref, forms):
    """7. Stage4Step(posterior="laplace") with supplied eps and dropout masks against the float64 reference: loss (1e-5 relative),
    every gradient (8e-6 of the tensor's largest entry: TIGHT_REL of tests/test_gpu_train.py) and the weights after Adam; the forms
    among themselves: 2e-6 relative on the flat gradient.  Adam's first step moves an entry by lr * g / (|g| + eps) -- about lr
    whichever way g points -- so an entry whose gradient is rounding noise may end 2 lr away from the reference's; every other entry
    agrees to 1e-6 (the rule of test_stage4step_forms_agree: at most 2e-3 of all entries differ by more)."""
    import torch
    import stage4
    ref_loss, ref_g, ref_after, n_floor = ref
    assert n_floor > 0
    masks = {k: [(T(a, dev), T(b, dev)) for a, b in v] for k, v in masks_np.items()}
    args = chain_args(P, dev) + [T(eps, dev)]
    flats = []
    for fused in forms:
        enc, dec = modules(gv, P, dev, train=True)
        step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=2, lr=1e-4, fused=fused, posterior="laplace")
        assert step.fused == fused
        loss = float(step(*args, masks=masks).item())
        print("laplace step H%d fused=%s: loss %.6f, float64 %.6f" % (P.hidden, fused, loss, ref_loss))
        assert abs(loss - ref_loss) <= TRAIN_LOSS_REL * abs(ref_loss)
        flats.append(N(step.grads.flat).astype(np.float64).copy())
        off = tot = 0
        for kind, m in (("enc", enc), ("dec", dec)):
            named = dict(m.named_parameters())
            for k in stage4.TRAINABLE:
                g, r = N(named[k].grad).astype(np.float64), ref_g[kind][k]
                e = float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r))))
                assert e <= 8e-6, (kind, k, e)
                d = np.abs(N(named[k]).astype(np.float64) - ref_after[kind][k])
                assert float(d.max()) <= 2.1e-4, (kind, k)
                off, tot = off + int((d > 1e-6).sum()), tot + d.size
        print("  weights after Adam: %d of %d entries off by more than 1e-6" % (off, tot))
        assert off <= 2e-3 * tot
    for f in flats[1:]:
        e = float(np.max(np.abs(f - flats[0]))) / max(1.0, float(np.max(np.abs(flats[0]))))
        print("  flat gradient, form against form: %.3e" % e)
        assert e <= TRAIN_GRAD_REL


def check_refusals(gv):
    """8. any other posterior raises ValueError naming the argument."""
    import pytest
    import stage4
    import stage6
    P = problem_h64()
    with pytest.raises(ValueError, match="posterior"):
        gv.CycleChain(None, None, 4, 2, posterior="cauchy")
    with pytest.raises(ValueError, match="posterior"):
        stage4.chain_forward(None, None, np.zeros((1, 1, 2)), None, None, None, None, None, 4, posterior="cauchy")
    with pytest.raises(ValueError, match="posterior"):
        stage4.loss_terms([], np.zeros((1, 1, 2)), 0, 4, posterior="cauchy")
    with pytest.raises(ValueError, match="posterior"):
        stage6.convert_pair(None, None, None, None, None, None, None, 4, posterior="cauchy")
    with pytest.raises(ValueError, match="posterior"):
        stage6.convert_pairs(None, None, [], None, None, None, 4, posterior="cauchy")
    with pytest.raises(ValueError, match="posterior"):
        stage6.convert_list(None, None, [[]], None, None, None, 4, posterior="cauchy")
    import torch
    enc, dec = modules(gv, P, torch.device("cpu"))
    with pytest.raises(ValueError, match="posterior"):
        stage4.Stage4Step(enc, dec, lat_dim=4, posterior="cauchy")
    with pytest.raises(NotImplementedError, match="script_loss"):
        stage4.Stage4Step(enc, dec, lat_dim=4, fused=False, script_loss=True, posterior="laplace")
