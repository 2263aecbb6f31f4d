"""Times one ten-pair call of stage 6 (decode.DecodePass.pairs) at the recipe's dimensions on the device, split by HIP events into
encoder, latent_mean, decoder, statistics, DTW, mc2e round 1, mc2e round 2 and post-filter / mod_pow, beside two baselines that are
the code paths the package had before decode.py:

  whole call   the same ten pairs through stage6.convert_many, the n_smpl_dec-draw latent means as torch ops, and per utterance the
               one-problem entry points stage6.mc2e (8), stage6.gv_postfilter (3), stage6.dtw_org_to_trg (11), stage6.mcd_aligned (6)
               with np.var on host copies (the script's own flow, decode_gru-cyclevae_gauss.py:302-475);
  mc2e kernel  cvae_mc2e_batch over the call's 80 matrices against cvae_mc2e looped over the same 80, device time between an event
               pair, the two sides alternated.

    python tools/decode_timing.py [--pairs 10] [--frames 637] [--n-smpl-dec 300] [--irlen 1024] [--runs 3] [--out profiles/decode_timing.json]

hu1024 networks (54 -> 64, 34 -> 50, lat 32), `pairs` utterance pairs of about `frames` frames (ragged, 70 % of them speech
frames), Philox draws.  One warm-up of each side, then alternating runs; min and max over `runs`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def baseline(enc, dec, items, y, lat_dim, n_smpl_dec, seed, stats, alpha, irlen):
    """The script's per-utterance loop on the entry points that existed before decode.py.  Returns one number per figure."""
    import numpy as np
    import torch
    import gru_vae
    import stage6
    L = lat_dim
    f64 = lambda t: t.to(torch.float64)
    gv_src, gv_trg, cg, cg_src, cg_trg = stats
    conv = stage6.convert_many(enc, dec, [(it[0], it[1]) for it in items], y[0], y[1], y[2], L, n_smpl_dec=n_smpl_dec, per_call=10, seed=seed,
                               first_pair_id=0)
    vals = []
    for it, (cv, cv_src, cv_trg, lat_src, lat_trg) in zip(items, conv):
        ix_s, ix_t, mcep, mcep_t = it[2], it[3], it[4], it[5]
        mcspc_s, mcspc_t = torch.index_select(mcep, 0, ix_s), torch.index_select(mcep_t, 0, ix_t)
        lf_s = torch.mean(gru_vae.sampling_vae_batch(lat_src.unsqueeze(0).repeat(n_smpl_dec, 1, 1), lat_dim=L), 0)
        lf_t = torch.mean(gru_vae.sampling_vae_batch(lat_trg.unsqueeze(0).repeat(n_smpl_dec, 1, 1), lat_dim=L), 0)
        for a, b in ((lat_src, lat_trg), (lf_s, lf_t)):                           # :332-360
            s, t = f64(torch.index_select(a, 0, ix_s)), f64(torch.index_select(b, 0, ix_t))
            al1 = stage6.dtw_org_to_trg(s, t)[0]
            c1 = stage6.dtw_org_to_trg(t, s, mcd=0)[2]
            al2 = stage6.dtw_org_to_trg(t, s)[0]
            c2 = stage6.dtw_org_to_trg(s, t, mcd=0)[2]
            vals += [float(torch.sqrt(torch.mean((al1 - t) ** 2, 0)).mean()), float(c1), float(torch.sqrt(torch.mean((al2 - s) ** 2, 0)).mean()),
                     float(c2)]
        cs = f64(torch.index_select(cv, 0, ix_s))
        for d0 in (0, 1):                                                         # :363-368
            fr = stage6.dtw_org_to_trg(cs[:, d0:], mcspc_t[:, d0:])[3].cpu().numpy()
            vals += [float(np.mean(fr)), float(np.std(fr))]
        for t in (cv, cv_src, cv_trg):                                            # :375, :389, :404
            vals.append(float(np.var(np.array(t.cpu().numpy(), dtype=np.float64)[:, 1:], axis=0).sum()))
        for mc, c, ix in ((mcspc_s, cv_src, ix_s), (mcspc_t, cv_trg, ix_t)):     # :377-393
            g = torch.index_select(c, 0, ix)
            for d0 in (0, 1):
                st = stage6.mcd_aligned(mc, g, d0=d0)[1].cpu().numpy()
                vals += [float(st[1]), float(st[2])]
        e_m, e_mt = stage6.mc2e(mcep, alpha, irlen), stage6.mc2e(mcep_t, alpha, irlen)
        outs = []
        for c, e_ref, gv, cgm in ((cv, e_m, gv_trg, cg), (cv_src, e_m, gv_src, cg_src), (cv_trg, e_mt, gv_trg, cg_trg)):
            dp = torch.log(e_ref / stage6.mc2e(c, alpha, irlen)) / 2.0             # :407-415
            x = f64(c)
            x[:, 0] += dp
            g, var = stage6.gv_postfilter(c, gv, cgm, dpow=dp)                     # :419-422
            vals.append(float(var.sum()))
            outs.append((x, g, e_ref))
        fr = stage6.dtw_org_to_trg(torch.index_select(outs[0][1], 0, ix_s)[:, 1:], mcspc_t[:, 1:])[3].cpu().numpy()      # :424
        vals += [float(np.mean(fr)), float(np.std(fr))]
        for mc, k, ix in ((mcspc_s, 1, ix_s), (mcspc_t, 2, ix_t)):                # :441, :458
            st = stage6.mcd_aligned(mc, torch.index_select(outs[k][1], 0, ix), d0=1)[1].cpu().numpy()
            vals += [float(st[1]), float(st[2])]
        for x, g, e_ref in outs:                                                  # :432, :449, :466
            g[:, 0] += torch.log(e_ref / stage6.mc2e(g, alpha, irlen)) / 2.0
        vals += [float((outs[0][0] - mcep).abs().sum()), float((outs[0][1] - mcep).abs().sum())]      # :470, :474
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--frames", type=int, default=637)
    ap.add_argument("--n-smpl-dec", type=int, default=300)
    ap.add_argument("--irlen", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import _cabi
    import decode
    import decode_util as U
    import gru_vae

    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = torch.device("cuda:0")
    n, T = a.pairs, a.frames
    jit = lambda k, q: T - 40 + (37 * k + 11 * q) % 61          # ragged lengths around T, fixed
    lens = tuple((jit(k, 0), jit(k, 1)) for k in range(n))
    P, items, _, y, stats = U.problem(tag="dectime", lens=lens, n_smpl=1, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05)
    dp = U.make_pass(P, dev, stats, n_smpl=a.n_smpl_dec, irlen=a.irlen)
    items = [U.to_dev(it, dev) for it in items]
    ty = U.to_dev(y, dev)
    tstats = U.to_dev(stats, dev)
    D = P.out_dim

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def staged(profile):
        passes = dp.net.network_passes(items, *ty, seed=5, profile=profile)
        return dp.metrics(items, passes, profile=profile)

    base = lambda: baseline(dp.enc, dp.dec, items, ty, P.lat_dim, a.n_smpl_dec, 5, tstats, U.ALPHA, a.irlen)
    res = {"pairs": n, "frames": T, "n_smpl_dec": a.n_smpl_dec, "irlen": a.irlen, "lens": lens,
           "speech_frames": [(int(it[2].numel()), int(it[3].numel())) for it in items]}
    parts = ("encoder", "latent_mean", "decoder") + decode.PROFILE_PARTS
    with torch.no_grad():
        _, got = wall(lambda: dp.pairs(items, *ty, seed=5))
        wall(base)
        runs = {k: [] for k in ("call", "baseline") + parts + ("mc2e_batch_80", "mc2e_loop_80")}
        for _ in range(a.runs):
            dp.reset()
            ms, _r = wall(lambda: dp.pairs(items, *ty, seed=5))
            runs["call"].append(ms)
            prof = {}
            wall(lambda: staged(prof))                          # (the split: the same call with event pairs around its parts)
            for k in parts:
                runs[k].append(prof[k])
            res.update({k: prof[k] for k in ("frames_1", "frames_2", "problems", "jobs")})
            ms, _r = wall(base)
            runs["baseline"].append(ms)
        # the mc2e kernels alone, on the call's 80 matrices
        mats = []
        for it, r, p in zip(items, got, dp.last_passes):
            mats += [it[4], it[5], p["cvmcep"], p["cvmcep_src"], p["cvmcep_trg"], r["cvmcep_gv"], r["cvmcep_src_gv"], r["cvmcep_trg_gv"]]
        mats = [m.contiguous() for m in mats]
        lib, st = gru_vae._lib(), torch.cuda.current_stream().cuda_stream
        frames = sum(m.shape[0] for m in mats)
        e_b, e_l = torch.empty(frames, dtype=torch.float64, device=dev), torch.empty(frames, dtype=torch.float64, device=dev)
        offs = [0]
        for m in mats:
            offs.append(offs[-1] + m.shape[0])
        jobs = [_cabi.Mc2eJob(m.data_ptr(), int(m.dtype == torch.float64), m.shape[0], D, 0, D, e_b.data_ptr() + 8 * o) for m, o in zip(mats, offs)]
        nb = lib.mc2e_batch_work_bytes(len(jobs), D, a.irlen)
        work = torch.empty(nb, dtype=torch.uint8, device=dev)

        def batch():
            lib.mc2e_batch(jobs, U.ALPHA, a.irlen, work.data_ptr(), nb, st)

        def loop():
            for m, o in zip(mats, offs):
                lib.mc2e(m.data_ptr(), m.dtype == torch.float64, D, m.shape[0], D, U.ALPHA, a.irlen, e_l.data_ptr() + 8 * o, st)

        def device_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        device_ms(batch)
        device_ms(loop)
        for _ in range(a.runs):
            runs["mc2e_batch_80"].append(device_ms(batch))
            runs["mc2e_loop_80"].append(device_ms(loop))
        res["mc2e_matrices"], res["mc2e_frames"] = len(mats), frames
        res["mc2e_batch_vs_loop_rel"] = float((e_b / e_l - 1.0).abs().max())
    res["ms"] = {k: {"min": min(v), "max": max(v), "runs": v} for k, v in runs.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
