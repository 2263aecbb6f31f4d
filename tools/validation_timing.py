"""Times the metric half of one validation batch on the device: batched (validation.ValidationPass.metrics: cvae_eval_stats,
cvae_dtw_batch, cvae_eval_stats, one D2H copy) against the same alignments and reductions issued one by one through the existing
one-problem entry points (stage6.dtw_org_to_trg, stage6.mcd_aligned, gru_vae.TWFSEloss / loss_vae, torch reductions).

    python tools/validation_timing.py [--pairs 8] [--frames 650] [--runs 3] [--out profiles/validation_timing.json]

hu1024 networks of the recipe's dimensions (54 -> 64, 34 -> 50), `pairs` utterance pairs of about `frames` frames (ragged, 70 % of
them speech frames).  Alternating runs after a warm-up of each; min and max over `runs`.  Also: the two local-cost strategies of
cvae_dtw_batch (option dtw_batch_cost) alternated on the same problems, and the work-buffer sizes at P = 96.
What is NOT the code under test: the network passes (timed once, for the split) and the baseline."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def baseline_metrics(src, trg, o, lat_dim, stdim):
    """The reference's per-utterance loop (train...:887-1019) with every array left on the device and every library call the
    one-problem entry point that existed before the batched ones.  One synchronising copy at the end."""
    import torch
    import gru_vae
    import stage6
    L, sd = lat_dim, stdim
    crit = gru_vae.TWFSEloss()
    f64 = lambda t: t.to(torch.float64)
    vals = []
    B = src["feat"].shape[0]
    for j in range(B):
        fs, ft = int(src["flens"][j]), int(trg["flens"][j])
        ix = {"s": src["spcidx"][j, :int(src["flens_spc"][j])], "t": trg["spcidx"][j, :int(trg["flens_spc"][j])],
              "sp": src["spcidx_par"][j, :int(src["flens_spc_par"][j])], "tp": trg["spcidx_par"][j, :int(trg["flens_spc_par"][j])]}
        for t, n in (("trj_src_src", fs), ("trj_src_trg", fs), ("trj_src_trg_src", fs), ("trj_trg_trg", ft), ("trj_trg_src", ft),
                     ("trj_trg_src_trg", ft)):
            vals.append(torch.var(f64(o[t][j, :n, 1:]), 0, unbiased=False).sum())
        for par, own, ip, io in (("lat_srctrg", "lat_src", ix["sp"], ix["s"]), ("lat_trgsrc", "lat_trg", ix["tp"], ix["t"])):
            p_, o_ = f64(torch.index_select(o[par][j], 0, ip)), f64(torch.index_select(o[own][j], 0, io))
            al1 = stage6.dtw_org_to_trg(o_, p_)[0]
            c1 = stage6.dtw_org_to_trg(p_, o_, mcd=0)[2]
            al2 = stage6.dtw_org_to_trg(p_, o_)[0]
            c2 = stage6.dtw_org_to_trg(o_, p_, mcd=0)[2]
            vals += [torch.sqrt(torch.mean((al1 - p_) ** 2, 0)).mean(), torch.sqrt(torch.mean((al2 - o_) ** 2, 0)).mean(), c1, c2]
        for S, a, b, ia, ib in ((trg, "trg", "src", ix["t"], ix["tp"]), (src, "src", "trg", ix["s"], ix["sp"])):
            own_spc = torch.index_select(S["feat"][j][:, sd:], 0, ia)
            for n in ("%s_%s" % (a, a), "%s_%s_%s" % (a, b, a)):
                cv = torch.index_select(o["trj_" + n][j], 0, ia)
                vals += [stage6.mcd_aligned(own_spc, cv, d0=0)[1][1], stage6.mcd_aligned(own_spc, cv, d0=1)[1][1]]
            cv = f64(torch.index_select(o["trj_%s_%s" % (a, b)][j], 0, ia))
            par = f64(torch.index_select(S["feat_par"][j][:, sd:], 0, ib))
            vals += [stage6.dtw_org_to_trg(cv, par)[2], stage6.dtw_org_to_trg(cv[:, 1:], par[:, 1:])[2]]
        for n, S, nfr in (("trg_trg", trg, ft), ("trg_src", trg, ft), ("src_src", src, fs), ("src_trg", src, fs), ("trg_src_trg", trg, ft),
                          ("src_trg_src", src, fs)):
            vals.append(crit(o["trj_" + n][j, :nfr], S["feat"][j, :nfr, sd:], L2=False, GV=False)[1].to(torch.float64))
        for t, nfr in (("lat_trg", ft), ("lat_src", fs), ("lat_trg_src", ft), ("lat_src_trg", fs)):
            vals.append(gru_vae.loss_vae(o[t][j, :nfr], lat_dim=L).to(torch.float64))
    return torch.stack([v.reshape(()) for v in vals]).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=650)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import gru_vae
    import validation
    import validation_util as U

    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = torch.device("cuda:0")
    lib = gru_vae._lib()
    n, T = a.pairs, a.frames
    jit = lambda k, q: T - 40 + (37 * k + 11 * q) % 61          # ragged lengths around T, fixed
    lens = (tuple((jit(k, 0), jit(k, 1)) for k in range(n)), tuple((jit(k, 2), jit(k, 3)) for k in range(n)))
    P, batches, (y_pp, y_src, y_trg), (gv_src, gv_trg) = U.e2e_problem(tag="valtime", batches=(lens,), in_dim=54, out_dim=50, lat_dim=32,
                                                                       hidden=1024, bias_scale=0.05)
    enc, dec = U.modules(P, dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    src, trg, _ = batches[0]
    ts, tt = U.side_to_torch(src, dev), U.side_to_torch(trg, dev)
    vp = validation.ValidationPass(enc.eval(), dec.eval(), P.lat_dim, P.stdim, gv_src, gv_trg)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    torch.manual_seed(1)
    wall(lambda: vp.network_passes(ts, tt, t(y_pp), t(y_src), t(y_trg)))
    pass_ms, o = wall(lambda: vp.network_passes(ts, tt, t(y_pp), t(y_src), t(y_trg)))
    res = {"pairs": n, "frames": T, "speech_frames": [int(v) for v in src["flens_spc"]], "network_passes_ms": pass_ms}
    wall(lambda: vp.metrics(ts, tt, o))
    wall(lambda: baseline_metrics(ts, tt, o, P.lat_dim, P.stdim))
    runs = {"batched": [], "baseline": [], "stats": [], "dtw": [], "latdist": []}
    for _ in range(a.runs):
        prof = {}
        ms, _r = wall(lambda: vp.metrics(ts, tt, o, profile=prof))
        runs["batched"].append(ms)
        for k in ("stats", "dtw", "latdist"):
            runs[k].append(prof[k])
        res.update(jobs=prof["jobs"], problems=prof["problems"], work_bytes=prof["work_bytes"])
        ms, _r = wall(lambda: baseline_metrics(ts, tt, o, P.lat_dim, P.stdim))
        runs["baseline"].append(ms)
    res["ms"] = {k: {"min": min(v), "max": max(v), "runs": v} for k, v in runs.items()}
    # the two local-cost strategies, alternated
    cost = {"slab": [], "on_the_fly": []}
    for _ in range(a.runs + 1):
        for name, v in (("slab", 1), ("on_the_fly", 0)):
            lib.set_option("dtw_batch_cost", v)
            prof = {}
            vp.metrics(ts, tt, o, profile=prof)
            cost[name].append(prof["dtw"])
            res["work_bytes_" + name] = prof["work_bytes"]
    lib.reset_options()
    res["dtw_cost_strategy_ms"] = {k: {"min": min(v[1:]), "max": max(v[1:]), "runs": v[1:]} for k, v in cost.items()}      # (first: warm-up)
    sizes = {}
    for name, v in (("slab", 1), ("on_the_fly", 0)):
        lib.set_option("dtw_batch_cost", v)
        sizes[name] = {"P96_T650": lib.dtw_batch_work_bytes(96, 650, 650), "P96_T2200": lib.dtw_batch_work_bytes(96, 2200, 2200),
                       "P1_T2200": lib.dtw_batch_work_bytes(1, 2200, 2200)}
    lib.reset_options()
    res["work_bytes_table"] = sizes
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
