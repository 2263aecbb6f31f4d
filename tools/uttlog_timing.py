"""What a training step on an utterance-length mini-batch (batch_size == 0) costs on the MI355X, alone and with the monitor around it:
hu1024 / ld32 / cyc2, ONE utterance, T = 637 and T = 1501 frames (two thirds of them speech, a parallel utterance of the same length).

Legs (per T, alternated repetition by repetition in ONE child process that runs under its own timeout; median and spread over the
repetitions after two warm-up repetitions; every figure is per step, HIP events around a run of steps and host wall time around
the same run):
  step        stage4.Stage4Step(sync=False) alone on stage4.utterance_step_args(items)
  mon         the same step inside trainlog.UttLog.before / after / lines

    python tools/uttlog_timing.py [--out profiles/uttlog_timing.json] [--reps 5] [--steps 4] [--frames 637,1501]
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


def child(T, reps, steps):
    import numpy as np
    import torch
    import gru_vae
    import stage4
    import synth
    import trainlog
    from validation_util import modules
    dev = torch.device("cuda:0")
    B = 1
    P = synth.CycleVAEProblem(B=B, T=T, tag="ult", bias_scale=0.05)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.RandomState(3)
    ns = T * 2 // 3
    spc = np.sort(rng.choice(T, size=ns, replace=False)).astype(np.int64)[None]
    own, other = synth.onehot_codes(B, T)
    items = (t(P.x), t(own), t(other), t(synth.features("ult/par", B, T, P.mu, P.sigma)), t(P.cvx), 0, 0, t(spc), t(spc.copy()), ["/d/SF1/0.h5"],
             ["/d/TF1/0.h5"], np.array([T]), np.array([T]), np.array([ns]), np.array([ns]), B)
    y_pp, y_dec = t(P.y_in_enc), t(P.y_in_dec)
    gv = np.ones(P.out_dim - 1)
    kw = stage4.utterance_step_args(items)

    def make(monitor):
        enc, dec = modules(P, dev)
        enc.train()
        dec.train()
        step = stage4.Stage4Step(enc, dec, lat_dim=P.lat_dim, n_cyc=2, lr=1e-6, sync=False)
        ul = trainlog.UttLog(enc, dec, P.lat_dim, P.stdim, gv, gv, n_cyc=2, spk_src="SF1") if monitor else None
        return step, ul

    def run(step, ul, n):
        """n steps; returns (wall ms, device ms) per step."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            if ul is not None:
                ul.before(items, y_pp)
            loss = step(y_in_enc=y_pp, y_in_dec=y_dec, eps=None, **kw)
            if ul is not None:
                ul.after(items, step.last_trajs, loss)
                ul.lines()
        e1.record()
        step.finish()
        torch.cuda.synchronize()
        if ul is not None:
            ul.epoch_end()
        return (time.perf_counter() - w0) * 1e3 / n, e0.elapsed_time(e1) / n

    legs = {"step": make(False), "mon": make(True)}
    res = {k: [] for k in legs}
    for rep in range(reps + 2):                     # two warm-up repetitions
        for name, (step, ul) in legs.items():
            r = run(step, ul, steps)
            if rep >= 2:
                res[name].append(r)
    out = {"B": B, "T": T, "speech_frames": ns, "reps": reps, "steps": steps,
           "fallbacks": {k: v[0].fallbacks for k, v in legs.items()}, "skipped": {k: v[0].skipped for k, v in legs.items()}}
    for name, v in res.items():
        w, d = np.array([a for a, _ in v]), np.array([b for _, b in v])
        out[name] = dict(wall_ms=float(np.median(w)), wall_min=float(w.min()), wall_max=float(w.max()), dev_ms=float(np.median(d)),
                         dev_min=float(d.min()), dev_max=float(d.max()))
    gru_vae.check_status()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uttlog_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--frames", default="637,1501")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.steps)
        return
    results = []
    for T in (int(v) for v in a.frames.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(T), "--reps", str(a.reps), "--steps", str(a.steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("T = %d: no result within %d s; stopping" % (T, a.timeout))
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("T = %d: the leg ended with status %d; stopping\n%s" % (T, p.returncode, p.stderr[-3000:]))
            break
        r = json.loads(line[-1][7:])
        results.append(r)
        s, m = r["step"], r["mon"]
        print("T = %4d  step alone %.2f ms device (%.2f .. %.2f), %.2f ms wall   with UttLog %.2f ms device (%.2f .. %.2f), %.2f ms wall   "
              "monitor %.2f ms = %.1f %% of the step   fallbacks %s" % (T, s["dev_ms"], s["dev_min"], s["dev_max"], s["wall_ms"], m["dev_ms"], m["dev_min"],
                                                                        m["dev_max"], m["wall_ms"], m["dev_ms"] - s["dev_ms"],
                                                                        100.0 * (m["dev_ms"] - s["dev_ms"]) / s["dev_ms"], r["fallbacks"]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"config": "hu1024 ld32 cyc2, one utterance", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
