"""Cost of an image environment map on BASELINE config 3 (1 M random triangles, PathIntegrator depth 5, 1920x1080x64 spp):
bench.py's frame (rr_threshold 1, power light distribution, seed 0) lit by the constant infinite light and by a synthetic 2048x1024 HDR sky on that light
(Scene.set_environment_map: ~100 MB of tables beside the ~95 MB tree). Prints one JSON line per mode and one summary line.

  python tools/bench_envmap.py [--mode both|const|map] [--steps 5] [--warmup 2] [--spp 64]
  python tools/bench_envmap.py --rocprof DIR      each mode once more in a child under rocprofv3 --kernel-trace --stats,
                                                  and the k_shade rows of their kernel-stats CSVs"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-rs_amd"))


def synthetic_sky(w=2048, h=1024, seed=1):
    """an HDR sky: a blue gradient brighter at the horizon, a little noise, a sun of 6 x 6 texels at 5e4"""
    t, s = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    theta = t * np.pi
    horizon = np.exp(-((theta - np.pi / 2) / 0.35) ** 2)
    up = np.clip(np.cos(theta), 0, None)
    rng = np.random.default_rng(seed)
    sky = np.stack([0.3 + 0.9 * horizon, 0.45 + 0.9 * horizon, 0.8 + 0.6 * horizon + 0.3 * up], axis=-1)
    sky *= (1.0 + 0.05 * rng.standard_normal((h, w)))[..., None]
    sky[theta > np.pi / 2] *= 0.2  # ground
    r0, c0 = int(0.3 * h), int(0.62 * w)
    sky[r0:r0 + 6, c0:c0 + 6] = (5.0e4, 4.6e4, 4.0e4)
    return np.clip(sky, 0, None).astype(np.float32)


def run(mode, steps, warmup, spp):
    import pbrt_hip
    from pbrt_hip import scenes
    w, h = 1920, 1080
    ctx = pbrt_hip.Context(0)
    sc = pbrt_hip.Scene(ctx, scenes.random_triangles(1_000_000, seq=1))
    if mode == "map":
        sc.set_environment_map(0, synthetic_sky())
    cam = scenes.random_triangles_camera(w, h)
    times, rays = [], []
    for i in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        film, st = sc.render(cam, w, h, spp, max_depth=5, rr_threshold=1.0, light_strategy=1, seed=0, spp_per_pass=0)  # bench.py's
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
            rays.append(st["rays_closest"] + st["rays_shadow"])
    rgb = pbrt_hip.film_to_rgb(film)
    out = dict(mode=mode, spp=spp, steps=steps, ms_per_frame=round(1e3 * float(np.median(times)), 2),
               mrays_per_s=round(float(np.median(np.array(rays) / np.array(times))) / 1e6, 1), rays_per_frame=int(np.median(rays)),
               image_mean=[round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], finite=bool(np.isfinite(rgb).all()))
    sc.close()
    ctx.close()
    return out


def shade_rows(csv_path):
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            if "k_shade" in r["Name"]:
                rows.append(dict(kernel=r["Name"].split("(")[0].replace("void ", ""), calls=int(r["Calls"]),
                                 total_ms=round(int(r["TotalDurationNs"]) / 1e6, 2), avg_us=round(float(r["AverageNs"]) / 1e3, 1),
                                 percent=float(r["Percentage"])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=["both", "const", "map"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rocprof", default="", help="output directory: run each mode in a child under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if a.rocprof:
        res = {}
        for mode in ("const", "map"):
            d = os.path.join(a.rocprof, mode)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", mode, "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--mode", mode, "--steps", "1", "--warmup", "1", "--spp", str(a.spp)]
            r = subprocess.run(cmd, timeout=900)
            if r.returncode != 0:
                sys.exit(f"rocprofv3 run of {mode} failed ({r.returncode})")
            stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            res[mode] = shade_rows(stats[0]) if stats else []
        print(json.dumps(dict(k_shade_stats=res)))
        return
    modes = ["const", "map"] if a.mode == "both" else [a.mode]
    res = {m: run(m, a.steps, a.warmup, a.spp) for m in modes}
    for m in modes:
        print(json.dumps(res[m]))
    if len(modes) == 2:
        c, m = res["const"], res["map"]
        print(json.dumps(dict(summary="map vs constant", frame_ratio=round(m["ms_per_frame"] / c["ms_per_frame"], 3),
                              mrays_ratio=round(m["mrays_per_s"] / c["mrays_per_s"], 3))))


if __name__ == "__main__":
    main()
