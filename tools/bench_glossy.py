"""Cost of plastic and metal on BASELINE config 3 (1 M random triangles, PathIntegrator depth 5, 1920x1080x64 spp, constant
infinite light): bench.py's frame (rr_threshold 1, power light distribution, seed 0) with its one matte material as it is,
switched to pbrt-v3's PlasticMaterial (Kd 0.5, Ks 0.25, roughness 0.1) and to MetalMaterial (gold-like eta / k, roughness 0.01).
The glossy scenes run k_shade's glossy instantiation. Prints one JSON line per mode and one summary line. A report, not a gate.

  python tools/bench_glossy.py [--mode all|matte|plastic|metal] [--steps 5] [--warmup 2] [--spp 64]
  python tools/bench_glossy.py --rocprof DIR      each mode once more in a child under rocprofv3 --kernel-trace --stats,
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

MODES = ("matte", "plastic", "metal")


def scene_for(mode):
    from pbrt_hip import scenes
    sc = scenes.random_triangles(1_000_000, seq=1)
    if mode == "plastic":
        sc["materials"] = scenes._materials([scenes.plastic((0.5, 0.5, 0.5), (0.25, 0.25, 0.25), 0.1)])
    elif mode == "metal":
        sc["materials"] = scenes._materials([scenes.metal((0.2, 0.92, 1.1), (3.9, 2.45, 2.14), 0.01)])
    return sc


def run(mode, steps, warmup, spp):
    import pbrt_hip
    from pbrt_hip import scenes
    w, h = 1920, 1080
    ctx = pbrt_hip.Context(0)
    sc = pbrt_hip.Scene(ctx, scene_for(mode))
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
    ap.add_argument("--mode", default="all", choices=["all", *MODES])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rocprof", default="", help="output directory: run each mode in a child under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if a.rocprof:
        res = {}
        for mode in MODES:
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
    modes = list(MODES) if a.mode == "all" else [a.mode]
    res = {m: run(m, a.steps, a.warmup, a.spp) for m in modes}
    for m in modes:
        print(json.dumps(res[m]))
    if len(modes) == 3:
        c = res["matte"]
        print(json.dumps(dict(summary="vs matte", **{m: dict(frame_ratio=round(res[m]["ms_per_frame"] / c["ms_per_frame"], 3),
                                                             mrays_ratio=round(res[m]["mrays_per_s"] / c["mrays_per_s"], 3))
                                                     for m in ("plastic", "metal")})))


if __name__ == "__main__":
    main()
