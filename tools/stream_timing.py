"""Times a step of stream.StreamConverter at the recipe's dimensions on the device: HIP-event device time and wall time per step in
steady state (every session pushes `hop` frames from the host before every step, so every step appends, compacts, runs both passes
and packs), for 1, 3, 4, 16 and 32 sessions and hops of 8 and 40 frames -- beside the same frames through stage6.convert_pairs
(ten pairs per call, whole utterances), for scale.

    python tools/stream_timing.py [--sessions 1,3,4,16,32] [--hops 8,40] [--steps 20] [--reps 5] [--out profiles/stream_timing.json]

hu1024 networks (54 -> 64, 34 -> 50, lat 32), n_smpl_dec = 1, Philox draws.  Per configuration: `warmup` steps, then `reps`
repetitions of `steps` steps, the configurations alternated between repetitions; the median over repetitions of the per-step mean.
One session and three sessions run the word-exchange kernels (max_sessions = live sessions), four and more the dataflow kernel.
The steps follow each other with no wait for the device in between; nothing here checks values (tests/test_stream_gpu.py does, also
for pushes and steps that run ahead of the device)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,3,4,16,32")
    ap.add_argument("--hops", default="8,40")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import numpy as np

    import gru_vae
    import stage6
    import stream
    import synth

    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = torch.device("cuda:0")
    sessions, hops = [int(v) for v in a.sessions.split(",")], [int(v) for v in a.hops.split(",")]
    frames = (a.warmup + a.steps * a.reps + 2) * max(hops)
    P = synth.CycleVAEProblem(B=1, T=frames, in_dim=54, out_dim=50, lat_dim=32, hidden=1024, bias_scale=0.05, tag="streamtime")

    def module(sd, i, o, enc):
        m = gru_vae.GRU_RNN(in_dim=i, out_dim=o, hidden_units=1024, kernel_size=3, dilation_size=2, scale_in_flag=enc, scale_out_flag=not enc)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(dev).eval()
    enc, dec = module(P.enc, 54, 64, True), module(P.dec, 34, 50, False)
    ypp, yt = torch.from_numpy(P.y_in_enc[:1]).to(dev), torch.from_numpy(P.y_in_dec[:1]).to(dev)
    trg_code = torch.tensor([[0.0, 1.0]])
    x = torch.from_numpy(np.ascontiguousarray(P.x[0])).pin_memory()
    configs = [(n, h) for n in sessions for h in hops]
    state = {}
    for n, h in configs:
        sc = stream.StreamConverter(enc, dec, ypp, yt, 32, max_sessions=n, hop=h, max_pending=max(64, 2 * h), n_smpl_dec=1, seed=1)
        state[(n, h)] = {"sc": sc, "sids": [sc.open(trg_code, draw_id=i) for i in range(n)], "at": 0, "dev": [], "wall": []}

    def steps(cfg, count):
        st, h = state[cfg], cfg[1]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(count):
            for sid in st["sids"]:
                st["sc"].push(sid, x[st["at"]:st["at"] + h])
            st["at"] += h
            st["sc"].step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / count, (time.perf_counter() - t0) * 1e3 / count

    with torch.no_grad():
        for cfg in configs:
            steps(cfg, a.warmup)
        for _ in range(a.reps):
            for cfg in configs:      # (alternated: drift of the clocks hits every configuration alike)
                d, w = steps(cfg, a.steps)
                state[cfg]["dev"].append(d)
                state[cfg]["wall"].append(w)
        gru_vae.check_status(sync=True)
        # for scale: ten whole pairs of 640 frames per convert_pairs call
        u = x[:640].to(dev)
        pairs = [(u, u)] * 10
        off = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage6.convert_pairs(enc, dec, pairs, ypp, yt, yt, 32, n_smpl_dec=1, seed=1)
            torch.cuda.synchronize()
            if r:
                off.append((time.perf_counter() - t0) * 1e3)
    res = {"steps": a.steps, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "configs": []}
    for n, h in configs:
        st = state[(n, h)]
        d, w = statistics.median(st["dev"]), statistics.median(st["wall"])
        res["configs"].append({"sessions": n, "hop": h, "device_ms_per_step": d, "wall_ms_per_step": w,
                               "us_per_dependent_step": 1e3 * d / (2 * h), "frames_per_s": n * h / (w * 1e-3),
                               "device_ms_runs": st["dev"], "wall_ms_runs": st["wall"]})
    ms = statistics.median(off)
    res["convert_pairs_10x640"] = {"wall_ms": ms, "frames_per_s": 20 * 640 / (ms * 1e-3), "runs": off}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
