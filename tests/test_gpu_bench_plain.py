"""bench.py as it is run for every change: a plain one-GPU run (no --full) times its steps and prints the line, nothing else,
and --dump-outputs writes what the last timed step computed. One functional run, no loops."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, TRIS, DEPTH = 256, 144, 8, 20000, 5


@pytest.mark.timeout(600)
def test_plain_run_times_its_steps_and_dumps_the_last_frame(hip_ctx, tmp_path):
    """The line carries the headline fields and the diagnostics blocks stay empty; film.npy is the one-process frame bit for
    bit and rays.npy its ray counts."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PBRT_BENCH_FAIL"):
        env.pop(k, None)
    out = tmp_path / "out"
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--tris", str(TRIS),
            "--max-depth", str(DEPTH), "--spp-per-pass", str(SPP), "--watchdog-s", "240", "--dump-outputs", str(out)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == ("Mrays/s", "Mrays/s", True, "f32")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["ms_per_step"] == pytest.approx(line["config"]["sec_per_frame"] * 1e3, abs=0.1)
    assert all(line[k] is None for k in ("roofline", "cpu_baseline", "secondary", "config4_n1"))
    assert line["config"]["film_check"] is None and "warnings" not in line and "error" not in line
    assert sorted(os.listdir(out)) == ["film.npy", "rays.npy"]
    film, rays = np.load(out / "film.npy"), np.load(out / "rays.npy")
    assert film.dtype == np.float32 and rays.dtype == np.float64
    sc = scenes.random_triangles(TRIS, seq=1)
    g = pbrt_hip.Scene(hip_ctx, sc, bvh=pbrt_hip.bvh_build(sc["positions"], sc["indices"], 4, pbrt_hip.SPLIT_SAH))
    ref, st = g.render(scenes.random_triangles_camera(W, H), W, H, SPP, max_depth=DEPTH, rr_threshold=1.0, light_strategy=1, seed=0)
    g.close()
    assert film.shape == ref.shape and film.tobytes() == ref.tobytes()
    assert rays.tolist() == [st["rays_closest"], st["rays_shadow"]]
    assert line["config"]["rays_per_frame"] == st["rays_closest"] + st["rays_shadow"]
