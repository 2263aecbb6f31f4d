"""Times one ten-pair call of stage 5 (stage5.CvgvPass.pairs) at the recipe's dimensions on the device, split by HIP events into
encoder, latent_mean, decoder, statistics and DTW, beside the same ten pairs through what the package offered before stage5:
stage6.convert_many, the n_smpl_dec-draw latent means as torch ops, and per utterance the one-problem entry points
stage6.dtw_org_to_trg / stage6.mcd_aligned with np.var on host copies of the three trajectories (the script's own flow,
calc_cvgv_gru-cyclevae_gauss.py:179-283).

    python tools/stage5_timing.py [--pairs 10] [--frames 637] [--n-smpl-dec 300] [--runs 3] [--out profiles/stage5_timing.json]

hu1024 networks (54 -> 64, 34 -> 50, lat 32), `pairs` utterance pairs of about `frames` frames (ragged, 70 % of them speech
frames), Philox draws.  Alternating runs after a warm-up of each; min and max over `runs`.  The baseline is not the code under
test."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def baseline(enc, dec, items, y, lat_dim, n_smpl_dec, seed):
    """The script's per-utterance loop on the entry points that existed before stage5.  Returns one number per figure."""
    import numpy as np
    import torch
    import gru_vae
    import stage6
    L = lat_dim
    f64 = lambda t: t.to(torch.float64)
    conv = stage6.convert_many(enc, dec, [(it[0], it[1]) for it in items], y[0], y[1], y[2], L, n_smpl_dec=n_smpl_dec, per_call=10, seed=seed,
                               first_pair_id=0)
    vals = []
    for it, (cv, cv_src, cv_trg, lat_src, lat_trg) in zip(items, conv):
        ix_s, ix_t, mc_s, mc_t = it[2], it[3], it[4], it[5]
        for t in (cv, cv_src, cv_trg):                                            # :195-205: to the host, float64, np.var
            vals.append(float(np.var(np.array(t.cpu().numpy(), dtype=np.float64)[:, 1:], axis=0).sum()))
        cs = f64(torch.index_select(cv, 0, ix_s))
        for d0 in (0, 1):                                                         # :210-215
            fr = stage6.dtw_org_to_trg(cs[:, d0:], mc_t[:, d0:])[3].cpu().numpy()
            vals += [float(np.mean(fr)), float(np.std(fr))]
        for mc, c, ix in ((mc_s, cv_src, ix_s), (mc_t, cv_trg, ix_t)):           # :224-243
            g = torch.index_select(c, 0, ix)
            for d0 in (0, 1):
                st = stage6.mcd_aligned(mc, g, d0=d0)[1].cpu().numpy()
                vals += [float(st[1]), float(st[2])]
        # :180-184 as the script forms it: n draws of the repeated rows, then the mean
        lf_s = torch.mean(gru_vae.sampling_vae_batch(lat_src.unsqueeze(0).repeat(n_smpl_dec, 1, 1), lat_dim=L), 0)
        lf_t = torch.mean(gru_vae.sampling_vae_batch(lat_trg.unsqueeze(0).repeat(n_smpl_dec, 1, 1), lat_dim=L), 0)
        for a, b in ((lat_src, lat_trg), (lf_s, lf_t)):                           # :255-282
            s, t = f64(torch.index_select(a, 0, ix_s)), f64(torch.index_select(b, 0, ix_t))
            al1 = stage6.dtw_org_to_trg(s, t)[0]
            c1 = stage6.dtw_org_to_trg(t, s, mcd=0)[2]
            al2 = stage6.dtw_org_to_trg(t, s)[0]
            c2 = stage6.dtw_org_to_trg(s, t, mcd=0)[2]
            vals += [float(torch.sqrt(torch.mean((al1 - t) ** 2, 0)).mean()), float(c1), float(torch.sqrt(torch.mean((al2 - s) ** 2, 0)).mean()),
                     float(c2)]
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--frames", type=int, default=637)
    ap.add_argument("--n-smpl-dec", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import stage5_util as S

    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = torch.device("cuda:0")
    n, T = a.pairs, a.frames
    jit = lambda k, q: T - 40 + (37 * k + 11 * q) % 61          # ragged lengths around T, fixed
    lens = tuple((jit(k, 0), jit(k, 1)) for k in range(n))
    P, items, _, y, gv = S.problem(tag="s5time", lens=lens, n_smpl=1, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05)
    cp = S.make_pass(P, dev, gv, a.n_smpl_dec)
    items = [S.to_dev(it, dev) for it in items]
    ty = S.to_dev(y, dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def staged(profile):
        passes = cp.network_passes(items, *ty, seed=5, profile=profile)
        return cp.metrics(items, passes, profile=profile)

    res = {"pairs": n, "frames": T, "n_smpl_dec": a.n_smpl_dec, "lens": lens, "speech_frames": [(int(it[2].numel()), int(it[3].numel())) for it in items]}
    with torch.no_grad():
        wall(lambda: cp.pairs(items, *ty, seed=5))
        wall(lambda: baseline(cp.enc, cp.dec, items, ty, P.lat_dim, a.n_smpl_dec, 5))
        runs = {k: [] for k in ("call", "baseline", "encoder", "latent_mean", "decoder", "stats", "dtw")}
        for _ in range(a.runs):
            cp.reset()
            ms, _r = wall(lambda: cp.pairs(items, *ty, seed=5))
            runs["call"].append(ms)
            prof = {}
            wall(lambda: staged(prof))                          # (the split: the same call with event pairs around its five parts)
            for k in ("encoder", "latent_mean", "decoder", "stats", "dtw"):
                runs[k].append(prof[k])
            res.update(jobs=prof["jobs"], problems=prof["problems"], work_bytes=prof["work_bytes"])
            ms, _r = wall(lambda: baseline(cp.enc, cp.dec, items, ty, P.lat_dim, a.n_smpl_dec, 5))
            runs["baseline"].append(ms)
    res["ms"] = {k: {"min": min(v), "max": max(v), "runs": v} for k, v in runs.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
