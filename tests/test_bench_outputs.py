"""bench.py's plain run and `--dump-outputs` on the emulator backend (CYCLEVAE_BENCH_BACKEND=emu: the host-fiber build of the library
behind the drop-in module, device selection only): a plain run times the headline chain and nothing else, `--steps` sets the number of
timed chains, and the arrays the last timed chain returned are written as float32 .npy files that are identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lat", "rec", "cv", "latcv", "reccyc")


def _bench(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["CYCLEVAE_BENCH_BACKEND"] = "emu"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch-per-gpu", "2", "--frames", "4", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(str(out_dir), n + ".npy")) for n in NAMES}


@pytest.mark.timeout(900)
def test_plain_bench_run_dumps_the_last_timed_step(tmp_path):
    import emu_bench_backend
    import emu_util
    emu_util.build_emu()
    d = emu_bench_backend.DIMS
    res, a = _bench(tmp_path / "a", 2)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["metric"] == "mcep_frames_per_sec_hu1024_ld32_cyc2" and res["steps"] == 2 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and abs(res["value"] - 2 * 4 / (1e-3 * res["ms_per_step"])) <= 1e-6 * res["value"]
    # what only --full measures stays out of a plain run
    assert res["other_kernels"] == {}
    for k in ("train_step", "sub_paths", "cpu_baseline", "mcd_db_vs_cpu"):
        assert k not in res, k
    L, C = d["lat_dim"], d["out_dim"]
    shapes = {"lat": 2 * L, "rec": C, "cv": C, "latcv": 2 * L, "reccyc": C}
    for n in NAMES:
        assert a[n].dtype == np.float32 and a[n].shape == (2, 2, 4, shapes[n]), (n, a[n].dtype, a[n].shape)
        assert np.all(np.isfinite(a[n])), n
    # same arguments, same inputs: the same outputs, bit for bit
    _, b = _bench(tmp_path / "b", 2)
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    # one timed step fewer: the last timed chain draws its latents with another seed, so the dump is another one
    _, c = _bench(tmp_path / "c", 1)
    assert any(not np.array_equal(a[n], c[n]) for n in ("rec", "cv", "reccyc"))
