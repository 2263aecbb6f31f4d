"""Times the eval pass of the hu1024 encoder at the three front-end depths (reference dilation_size), on the device.

    python tools/frontend_depth_timing.py [--rows 64] [--frames 80] [--reps 40] [--out profiles/frontend_depth_timing.json]

hu1024 encoder (54 -> 64), alternated within every repetition after a warm-up:
    ds2       dilation_size 2: k_gru_steps_v6<16, 8>, front-end fused (the yardstick, unchanged)
    ds1       dilation_size 1: k_gru_steps_v6<16, 3>, front-end fused
    ds3_v6h   dilation_size 3: front-end GEMM (27 x 56 = 1512 k) + k_gru_steps_v6<16, 0> (form V6H)
    ds3_v2    the same pass forced onto k_gru_steps_v2 (CVAE_FLAG_HOISTED_FRONTEND)
Per variant: ms per pass (HIP events around the whole forward call: prologue, front-end, recurrence, projection) and ms of the
library's own event bracket (CVAE_FLAG_PROFILE, in a separate set of repetitions) -- the recurrence launch, and for the hoisted
forms the front-end GEMM in front of it, which the bracket includes.  The GEMM on its own cannot be bracketed from outside
the library; `ds3_gemm_upper_ms` is the bracket of a ONE-frame pass over rows x (frames + 26) / 27 rows -- the same GEMM shape
([rows x padded frames] x 1512 by 1512 x 3072) with a single per-step launch behind it: an upper bound."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cyclevae-vc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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
    names = {v: k[5:] for k, v in vars(_cabi).items() if k.startswith("EVAL_")}

    def mod(ds):
        P = synth.CycleVAEProblem(B=B, T=T, bias_scale=0.05, tag="fetime%d" % ds, dilation_size=ds)
        m = gru_vae.GRU_RNN(in_dim=Cin, out_dim=Co, hidden_units=H, dilation_size=ds, scale_in_flag=True, scale_out_flag=False)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in P.enc.items()})
        return m.to(dev).eval(), torch.from_numpy(P.x).to(dev), torch.from_numpy(P.y_in_enc).to(dev)

    m1, m2, m3 = mod(1), mod(2), mod(3)
    variants = [("ds2", m2, 0), ("ds1", m1, 0), ("ds3_v6h", m3, 0), ("ds3_v2", m3, _cabi.FLAG_HOISTED_FRONTEND)]

    def run(mx, extra):
        m, x, y0 = mx
        gru_vae._flags_extra = extra
        try:
            return m(x, y0, clamp_vae=True, lat_dim=32)
        finally:
            gru_vae._flags_extra = 0

    lib = gru_vae._lib()
    whole = {n: [] for n, _, _ in variants}
    kern = {n: [] for n, _, _ in variants}
    forms = {}
    with torch.no_grad():
        for _ in range(a.warmup):
            for n, mx, fl in variants:
                run(mx, fl)
        torch.cuda.synchronize()
        for n, mx, fl in variants:
            gru_vae._flags_extra = fl
            forms[n] = names[lib.plan_pass(mx[0].prepared(dev)[0], B, T, gru_vae._flags())]
            gru_vae._flags_extra = 0
        for _ in range(a.reps):
            for n, mx, fl in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mx, fl)
                e1.record()
                e1.synchronize()
                whole[n].append(e0.elapsed_time(e1))
        lib.profile_collect()
        for _ in range(a.reps):
            for n, mx, fl in variants:
                run(mx, fl | _cabi.FLAG_PROFILE)
                torch.cuda.synchronize()
                kern[n].append(lib.profile_collect())
        # the front-end GEMM of ds 3 over the same rows x padded frames, bracketed with ONE step launch behind it (a T = 1 pass
        # plans PER_STEP; rows * (T + 26) padded frames = (rows * (T + 26) / 27) one-frame rows)
        rows1 = max(1, B * (T + 26) // 27)
        m, x, y0 = m3
        x1 = x.reshape(-1, 1, Cin)[:1].expand(rows1, 1, Cin).contiguous()
        y1 = y0[:1].expand(rows1, 1, Co).contiguous()
        gemm = []
        for i in range(a.warmup + a.reps):
            gru_vae._flags_extra = _cabi.FLAG_PROFILE
            m(x1, y1, clamp_vae=True, lat_dim=32)
            gru_vae._flags_extra = 0
            torch.cuda.synchronize()
            ms, _ = lib.profile_collect()
            if i >= a.warmup:
                gemm.append(ms)
    gru_vae.check_status(sync=True)

    res = {"rows": B, "frames": T, "hidden": H, "reps": a.reps, "variants": {}, "ds3_gemm_upper_rows": rows1,
           "ds3_gemm_upper_ms": float(np.median(np.array(gemm)))}
    for n, _, _ in variants:
        w = np.array(whole[n])
        k = np.array([v[0] for v in kern[n]])
        res["variants"][n] = {"form": forms[n], "ms_per_pass_median": float(np.median(w)), "ms_per_pass_min": float(w.min()),
                              "ms_per_pass_max": float(w.max()), "bracket_ms_median": float(np.median(k)),
                              "bracket_launches": int(kern[n][0][1]), "us_per_frame_of_bracket": float(np.median(k)) * 1e3 / T}
    v = res["variants"]
    res["ds3_v6h_over_v2_pass"] = v["ds3_v6h"]["ms_per_pass_median"] / v["ds3_v2"]["ms_per_pass_median"]
    res["ds3_v6h_over_ds2_pass"] = v["ds3_v6h"]["ms_per_pass_median"] / v["ds2"]["ms_per_pass_median"]
    res["ds1_over_ds2_pass"] = v["ds1"]["ms_per_pass_median"] / v["ds2"]["ms_per_pass_median"]
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
