"""Times the eval pass of a stacked (hidden_layers = 2) encoder next to the one-layer pass, on the device.

    python tools/stacked_timing.py [--rows 64] [--frames 80] [--reps 40] [--out profiles/stacked_timing.json]

hu1024 encoder (54 -> 64), three variants on the same inputs, alternated within every repetition after a warm-up:
    one_layer   GRU_RNN(hidden_layers=1): k_gru_steps_v6 (the yardstick)
    resident    hidden_layers=2 on k_gru_steps_deep3 (one launch per pass)
    generic     hidden_layers=2 forced onto k_gru_steps_deep (CVAE_FLAG_GENERIC_STEP)
Per variant: ms per pass (HIP events around the whole forward call: prologue, front-end, recurrence, projection), ms of the
recurrence launch alone (the library's own event bracket, CVAE_FLAG_PROFILE, in a separate set of repetitions), us per dependent
sub-step (frames x layers), and the algorithmic MACs over the fp32-MFMA peak (157.3 TFLOP/s, MI355X): per frame and row
L x 2 x 3H^2 recurrent MACs (one layer: 3H^2 recurrent + the feedback 3H x Cout + Cout x H) plus front-end 3H x 9Cin and
projection Cout x H.  A share of the peak of an end-to-end pass time: launch gaps and hand-off latency included."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_FP32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import _cabi
    import gru_vae
    import synth

    dev = torch.device("cuda:0")
    B, T, H, Cin, Co = a.rows, a.frames, 1024, 54, 64
    P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="stk1024h", hidden_layers=2)

    def mod(layers):
        m = gru_vae.GRU_RNN(in_dim=Cin, out_dim=Co, hidden_units=H, hidden_layers=layers, scale_in_flag=True, scale_out_flag=False)
        sd = {k: v for k, v in P.enc.items() if layers == 2 or not k.endswith("_l1")}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(dev).eval()

    one, two = mod(1), mod(2)
    x, y0 = torch.from_numpy(P.x).to(dev), torch.from_numpy(P.y_in_enc).to(dev)
    variants = [("one_layer", one, 0, 1), ("resident", two, 0, 2), ("generic", two, _cabi.FLAG_GENERIC_STEP, 2)]

    def run(m, extra):
        gru_vae._flags_extra = extra
        try:
            return m(x, y0, clamp_vae=True, lat_dim=32)
        finally:
            gru_vae._flags_extra = 0

    whole = {n: [] for n, _, _, _ in variants}
    kern = {n: [] for n, _, _, _ in variants}
    with torch.no_grad():
        for _ in range(a.warmup):
            for n, m, fl, _ in variants:
                run(m, fl)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for n, m, fl, _ in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(m, fl)
                e1.record()
                e1.synchronize()
                whole[n].append(e0.elapsed_time(e1))
        lib = gru_vae._lib()
        lib.profile_collect()
        for _ in range(a.reps):
            for n, m, fl, _ in variants:
                run(m, fl | _cabi.FLAG_PROFILE)
                torch.cuda.synchronize()
                ms, launches = lib.profile_collect()
                kern[n].append((ms, launches))
    gru_vae.check_status(sync=True)

    res = {"rows": B, "frames": T, "hidden": H, "reps": a.reps, "peak_fp32_mfma_flops": PEAK_FP32_MFMA, "variants": {}}
    for n, _, _, L in variants:
        w = np.array(whole[n])
        k = np.array([v[0] for v in kern[n]])
        rec = L * 2 * 3 * H * H if L > 1 else 3 * H * H + 3 * H * Co + Co * H
        macs = float(B) * T * (rec + 3 * H * 9 * Cin + Co * H)
        res["variants"][n] = {
            "layers": L, "ms_per_pass_median": float(np.median(w)), "ms_per_pass_min": float(w.min()), "ms_per_pass_max": float(w.max()),
            "recurrence_ms_median": float(np.median(k)), "recurrence_launches": int(kern[n][0][1]),
            "us_per_substep_of_recurrence": float(np.median(k)) * 1e3 / (T * L),
            "algorithmic_macs": macs, "share_of_fp32_mfma_peak_of_pass": 2.0 * macs / (float(np.median(w)) * 1e-3) / PEAK_FP32_MFMA,
            "share_of_fp32_mfma_peak_of_recurrence": 2.0 * float(B) * T * rec / (float(np.median(k)) * 1e-3) / PEAK_FP32_MFMA}
    v = res["variants"]
    res["resident_over_2x_one_layer_pass"] = v["resident"]["ms_per_pass_median"] / (2.0 * v["one_layer"]["ms_per_pass_median"])
    res["resident_over_2x_one_layer_recurrence"] = v["resident"]["recurrence_ms_median"] / (2.0 * v["one_layer"]["recurrence_ms_median"])
    res["generic_over_resident_pass"] = v["generic"]["ms_per_pass_median"] / v["resident"]["ms_per_pass_median"]
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
