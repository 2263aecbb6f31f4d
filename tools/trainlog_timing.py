"""What the training monitor costs per step on the MI355X: hu1024 / ld32 / cyc2, T = 80, at one, eight and 64 utterances.

Legs (per batch size, alternated repetition by repetition in ONE child process that runs under its own timeout; median over the
repetitions after warm-up; every figure is per step, HIP events around a run of steps and host wall time around the same run):
  step_sync / step_lagged          stage4.Stage4Step alone (sync=True / sync=False): the parent's step
  mon_sync / mon_lagged            the same step inside trainlog.TrainLog.before / after / lines
  script                           Stage4Step(fused=False, script_loss=True) plus the script's four host calc_mcd per utterance and
                                   cycle (tests/trainlog_ref.window_record on host copies): the unchanged script's flow, for scale
  kernel                           cvae_trainlog_window alone, event-timed, with the bytes it moves
  before                           one closing TrainLog.before (encoder pass, jobs, six alignments per utterance), wall and device

    python tools/trainlog_timing.py [--out profiles/trainlog_timing.json] [--reps 7] [--steps 20]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(B, reps, steps):
    import numpy as np
    import torch
    import gru_vae
    import stage4
    import synth
    import trainlog
    import trainlog_ref as tref
    import trainlog_util as U
    from validation_util import modules
    dev = torch.device("cuda:0")
    T, F = 80, 160
    P = synth.CycleVAEProblem(B=B, T=T, tag="tlt", bias_scale=0.05)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.RandomState(3)
    ns = [F * 2 // 3] * B
    batch = dict(feat=synth.features("tlt/feat", B, F, P.mu, P.sigma), par=synth.features("tlt/par", B, F, P.mu, P.sigma),
                 cv=synth.features("tlt/cv", B, F, P.mu[:P.stdim], P.sigma[:P.stdim]), files=["/d/SF1/%d.h5" % j for j in range(B)],
                 files_trg=["/d/TF1/%d.h5" % j for j in range(B)], flens=np.full(B, F), flens_trg=np.full(B, F), ns=np.array(ns),
                 ns_trg=np.array(ns))
    batch["own"], batch["other"] = synth.onehot_codes(B, F)
    batch["spc"] = np.stack([np.sort(rng.choice(F, size=ns[0], replace=False)) for _ in range(B)]).astype(np.int64)
    batch["spc_trg"] = batch["spc"].copy()
    wins = list(U.yields(batch, T, t))
    y_pp, y_dec = t(P.y_in_enc), t(P.y_in_dec)
    gv = np.ones(P.out_dim - 1)

    def make(sync, monitor, script=False):
        enc, dec = modules(P, dev)
        enc.train()
        dec.train()
        step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=2, lr=1e-6, sync=sync, **(dict(fused=False, script_loss=True) if script else {}))
        tl = trainlog.TrainLog(enc, dec, P.lat_dim, P.stdim, gv, gv, n_cyc=2, spk_src="SF1") if monitor else None
        return step, tl

    def run(leg, n):
        """n steps over the two windows; returns (wall ms, device ms) per step."""
        step, tl, script = leg["step"], leg["tl"], leg.get("script", False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        carry = leg.get("carry")
        for k in range(n):
            items = wins[k % 2]
            s, e = items[5], items[6]
            if s == 0:
                carry = None
            if tl is not None and s > 0:        # (the closing before() is timed on its own: here the windows of one utterance batch repeat)
                tl.before(items, y_pp)
            elif tl is not None:
                tl._fresh = True
            loss, carry = step(items[0][:, s:e + 1], items[4][:, s:e + 1], items[1], items[2], y_pp, y_dec, None,
                               flen_acc=[int(v) for v in items[20]], select_utt_idx=list(items[19]), carry=carry, return_state=True)
            if tl is not None:
                tl.after(items, step.last_trajs, loss)
                tl.lines()
            if script:
                trajs = [{q: v.detach().cpu().numpy() for q, v in tr.items()} for tr in step.last_trajs]
                tref.window_record(trajs, items[0][:, s:e + 1].cpu().numpy(), P.stdim, P.lat_dim, batch["spc"], list(items[19]), items[20],
                                   items[7], items[8], s)
                loss.item()
        e1.record()
        if hasattr(step, "finish"):
            step.finish()
        torch.cuda.synchronize()
        leg["carry"] = None
        if tl is not None:
            tl.epoch_end()
        return (time.perf_counter() - w0) * 1e3 / n, e0.elapsed_time(e1) / n

    legs = {}
    for name, (sync, mon, script) in (("step_sync", (True, False, False)), ("step_lagged", (False, False, False)),
                                      ("mon_sync", (True, True, False)), ("mon_lagged", (False, True, False)),
                                      ("script", (True, False, True))):
        step, tl = make(sync, mon, script)
        legs[name] = dict(step=step, tl=tl, script=script)
    res = {k: [] for k in legs}
    for rep in range(reps + 2):                     # two warm-up repetitions
        for name, leg in legs.items():
            n = max(2, steps // 4) if name == "script" else steps
            r = run(leg, n)
            if rep >= 2:
                res[name].append(r)
    out = {"B": B, "T": T, "reps": reps, "steps": steps}
    for name, v in res.items():
        w, d = np.array([a for a, _ in v]), np.array([b for _, b in v])
        out[name] = dict(wall_ms=float(np.median(w)), wall_min=float(w.min()), wall_max=float(w.max()), dev_ms=float(np.median(d)),
                         dev_min=float(d.min()), dev_max=float(d.max()))
    # the kernel alone, on the trajectories of the last step
    step, tl = legs["mon_lagged"]["step"], legs["mon_lagged"]["tl"]
    items = wins[0]
    loss, _ = step(items[0][:, :T], items[4][:, :T], items[1], items[2], y_pp, y_dec, None, flen_acc=[int(v) for v in items[20]],
                   select_utt_idx=list(items[19]), return_state=True)
    step.finish()
    tl._fresh = True
    ks = []
    for rep in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            tl.after(items, step.last_trajs, loss)
            tl._fresh = False                    # (the accumulators of an utterance batch are allocated once, at its first window)
            tl.poll()
        e1.record()
        torch.cuda.synchronize()
        tl.epoch_end()
        ks.append(e0.elapsed_time(e1) / 20)
    # ... and the launch by itself: the argument block of the latest after(), 50 launches back to back
    args, lib, st = tl.last_args[0], gru_vae._lib(), gru_vae._stream()
    pure = []
    for rep in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        for _ in range(50):
            lib.trainlog_window(args, st)
        e1.record()
        w1 = time.perf_counter()
        torch.cuda.synchronize()
        pure.append((e0.elapsed_time(e1) / 50, (w1 - w0) * 1e3 / 50))
    D, L = P.out_dim, P.lat_dim
    # per cycle 3 D-wide and 2 2L-wide trajectories read, the targets read, cycle 0's four trajectories written
    moved = 4 * B * T * (2 * (3 * D + 2 * 2 * L) + 2 * D + (3 * D + 2 * L))
    k_ms = float(np.median([a for a, _ in pure[2:]]))
    out["kernel"] = dict(launch_ms=k_ms, min=float(min(a for a, _ in pure[2:])), max=float(max(a for a, _ in pure[2:])),
                         host_ms_per_launch=float(np.median([b for _, b in pure[2:]])), bytes=int(moved),
                         hbm_fraction=float(moved / (k_ms * 1e-3) / 8e12), after_poll_ms=float(np.median(ks[2:])),
                         note="launch_ms: events around 50 back-to-back launches (an upper bound of the kernel where the host enqueues slower "
                              "than the device runs: compare host_ms_per_launch); after_poll_ms: events around back-to-back after() + poll() "
                              "calls, host-bound; HBM peak taken as 8 TB/s")
    # the closing before()
    bs = []
    for rep in range(3):
        tl._fresh = True
        tl.after(wins[0], step.last_trajs, loss)
        tl.after(wins[1], [{q: v[:, :wins[1][6] - wins[1][5] + 1] for q, v in tr.items()} for tr in step.last_trajs], loss)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        e0.record()
        tl.before(wins[0], y_pp)
        e1.record()
        w1 = time.perf_counter()
        torch.cuda.synchronize()
        tl.epoch_end()
        bs.append(((w1 - w0) * 1e3, e0.elapsed_time(e1)))
    out["before"] = dict(host_ms=float(np.median([a for a, _ in bs])), dev_ms=float(np.median([b for _, b in bs])), utterances=B)
    gru_vae.check_status()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainlog_timing.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.steps)
        return
    results = []
    for B in (int(v) for v in a.batches.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--reps", str(a.reps), "--steps", str(a.steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("B = %d: no result within %d s; stopping" % (B, a.timeout))
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("B = %d: the leg ended with status %d; stopping\n%s" % (B, p.returncode, p.stderr[-3000:]))
            break
        r = json.loads(line[-1][7:])
        results.append(r)
        print("B = %2d  step %.2f / %.2f ms (sync / lagged, wall)   monitored %.2f / %.2f ms   script flow %.2f ms   kernel %.3f ms (%.1f %% of HBM peak)   "
              "before() %.2f ms host, %.2f ms device" % (B, r["step_sync"]["wall_ms"], r["step_lagged"]["wall_ms"], r["mon_sync"]["wall_ms"],
                                                         r["mon_lagged"]["wall_ms"], r["script"]["wall_ms"], r["kernel"]["launch_ms"],
                                                         100 * r["kernel"]["hbm_fraction"], r["before"]["host_ms"], r["before"]["dev_ms"]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"config": "hu1024 ld32 cyc2 T=80", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
