"""Cost of the lobe-list shading build (profiles/r12_lobe_materials.txt, section 3): scenes.mixed_materials_scene(n_tris=200000)
(matte, mirror, glass; an area light and an environment light) at 1920x1080x16, PathIntegrator max_depth 5, shade_order 0, as it
is and with its matte row replaced by scenes.uber(kd) at pbrt-v3's defaults (LambertianReflection and MicrofacetReflection,
read per lane from the DevLobeRow in global memory). Frame time = PbrtRenderStats.total_ms of frames 2-4 of four, as
profiles/r09_disney.txt measured the Disney row. A report, not a gate.

  python tools/bench_lobes.py [--mode all|matte|uber]
  python tools/bench_lobes.py --rocprof DIR       each mode once more in a child under rocprofv3 --kernel-trace --stats, and the
                                                  k_shade rows of their kernel-stats CSVs"""
import argparse
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-rs_amd"))

MODES = ("matte", "uber")


def run(mode, frames=4):
    import pbrt_hip
    from pbrt_hip import scenes
    w, h = 1920, 1080
    sc = scenes.mixed_materials_scene(n_tris=200000)
    if mode == "uber":
        sc["lobe_descs"] = {0: scenes.uber(kd=tuple(float(c) for c in sc["materials"][0]["kd"]))}
    ctx = pbrt_hip.Context(0)
    scene = pbrt_hip.Scene(ctx, sc)
    cam = scenes.random_triangles_camera(w, h)
    ms, rays = [], []
    for _ in range(frames):
        _, st = scene.render(cam, w, h, 16, max_depth=5, seed=0, shade_order=0)
        ms.append(round(st["total_ms"], 2))
        rays.append(st["rays_closest"] + st["rays_shadow"])
    scene.close()
    ctx.close()
    return dict(mode=mode, frame_ms=ms, rays_per_frame=rays[-1])


def shade_rows(csv_path):
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            if "k_shade" in r["Name"] or "k_trace" in r["Name"]:
                rows.append(dict(kernel=r["Name"].split("(")[0].replace("void ", ""), calls=int(r["Calls"]),
                                 total_ms=round(int(r["TotalDurationNs"]) / 1e6, 2), avg_us=round(float(r["AverageNs"]) / 1e3, 1)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", *MODES])
    ap.add_argument("--rocprof", default="", help="output directory: run each mode in a child under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if a.rocprof:
        res = {}
        for mode in MODES:
            d = os.path.join(a.rocprof, mode)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", mode, "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--mode", mode]
            r = subprocess.run(cmd, timeout=300)
            if r.returncode != 0:
                sys.exit(f"rocprofv3 run of {mode} failed ({r.returncode})")
            stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            res[mode] = shade_rows(stats[0]) if stats else []
        print(json.dumps(dict(kernel_stats=res)))
        return
    for m in (MODES if a.mode == "all" else [a.mode]):
        print(json.dumps(run(m)))


if __name__ == "__main__":
    main()
