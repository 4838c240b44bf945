"""Records tests/golden/dispatch_matrix.json: one small render (and, for the traversal cases, one intersect / intersect_p batch) per
kernel the host driver can select, from the library the binding loads. Run it with PBRT_HIP_LIB naming the library of the commit
BEFORE a change to kernel selection; tests/test_gpu_dispatch_matrix.py then holds the tree's own library to what that one computed.

  PBRT_HIP_LIB=<library of the parent commit> python tests/golden/make_dispatch_matrix.py      (needs the GPU; rewrites the .json)

Per case: the SHA-256 of the film's bytes, the PbrtRenderStats ray counts, for the traversal cases the SHA-256 of the hit records and
of the occlusion flags, and the traversal counters where counting is on. Every case runs twice; a case whose two runs disagree goes to
the fixture's "excluded" list instead (at most 5 % of the cases, and every integrator x feature cell keeps one). Data only.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "pbrt-rs_amd"))
import pbrt_hip  # noqa: E402
from pbrt_hip import scenes  # noqa: E402

FIXTURE = os.path.join(HERE, "dispatch_matrix.json")
W, H, SPP, DEPTH = 40, 24, 4, 3          # 40 x 24: partial 16 x 16 tiles
N_RAYS = 4096
PATH, DIRECT, WHITTED, AO = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO
AUTO, STACK, STACKLESS = pbrt_hip.TRAVERSAL_AUTO, pbrt_hip.TRAVERSAL_STACK, pbrt_hip.TRAVERSAL_STACKLESS
FEATURES = ("matte", "plastic", "matdesc", "disney", "maps", "shapes")
INTEGRATORS = dict(path=PATH, direct=DIRECT, whitted=WHITTED, ao=AO)


# ---- scenes: the Cornell box with one material row or one light swapped, and the smallest scene of every other kind ----
def _translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def _cornell_with_row(row, material):
    sc = scenes.cornell_box()
    m = sc["materials"].copy()
    m[row] = material
    return dict(sc, materials=m)


def _cornell_maps():
    sc = scenes.cornell_box()
    down = _translate(278.0, 500.0, 279.0)
    down[:3, :3] = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]   # light-space +z looks down the box's -y
    sc = scenes.with_lights(sc, [scenes.projection_light(down, (4.0e5, 3.5e5, 3.0e5), 70.0)])
    rgb = (0.25 + 0.75 * scenes.pcg32_float(91, 4 * 8 * 3)).reshape(4, 8, 3).astype(np.float32)
    return dict(sc, light_maps={len(sc["lights"]) - 1: rgb})


def _cornell_shapes():
    sc = scenes.cornell_box()
    up = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)  # object +z = world +y
    recs = [scenes.sphere_shape(70.0, to_world=_translate(185.0, 235.0, 169.0), material=1),
            scenes.cylinder(40.0, 0.0, 120.0, to_world=_translate(420.0, 0.0, 120.0) @ up, material=2),
            scenes.disk(120.0, 40.0, to_world=_translate(420.0, 0.0, 120.0) @ up, material=2)]
    return dict(sc, shapes=scenes.shapes(*recs))


SCENES = {
    "matte": lambda: (scenes.cornell_box(), scenes.cornell_camera),
    "plastic": lambda: (_cornell_with_row(1, scenes.plastic((0.65, 0.05, 0.05), (0.3, 0.3, 0.3), 0.15)), scenes.cornell_camera),
    "matdesc": lambda: (dict(scenes.cornell_box(), material_descs={2: scenes.substrate((0.12, 0.45, 0.15), (0.2, 0.2, 0.2), 0.2)}),
                        scenes.cornell_camera),
    "disney": lambda: (dict(scenes.cornell_box(), disney_descs={1: scenes.disney((0.65, 0.05, 0.05), metallic=0.3, roughness=0.4,
                                                                                 clearcoat=0.5)}), scenes.cornell_camera),
    "maps": lambda: (_cornell_maps(), scenes.cornell_camera),
    "shapes": lambda: (_cornell_shapes(), scenes.cornell_camera),
    "spheres": lambda: (scenes.sphere_scene(), scenes.sphere_camera),
    "instanced": lambda: (scenes.instanced_scene(200, 5, extent=1.5), lambda w, h: scenes.instanced_camera(w, h, 1.5)),
    "two_level": lambda: (scenes.two_level_scene(30), scenes.two_level_camera),
    "rand20k": lambda: (scenes.random_triangles(20_000, seq=3, size=0.05), scenes.random_triangles_camera),
}
# the scenes whose AUTO traversal is meant to run the wide kernels (Scene.wide_records() > 0 is asserted for them)
WIDE_SCENES = ("matte", "instanced", "two_level")
# random_rays per traversal scene: (centre, origin_extent) of rays that start inside and around the geometry
RAY_BOX = dict(matte=(278.0, 300.0), spheres=(0.0, 3.0), shapes=(278.0, 300.0), instanced=(0.0, 2.0), two_level=(0.0, 3.0))


def cases():
    """Every case as a dict: id, kind ("shade" / "trace" / "raysort"), scene, and the render arguments or the traversal settings."""
    out = []

    def shade(cid, scene, integ, w=W, h=H, **kw):
        out.append(dict(id=cid, kind="shade", scene=scene, integrator=integ, feature=scene, width=w, height=h, kw=kw))

    for f in FEATURES:
        shade(f"shade-{f}-path", f, "path")
        for ls in (0, 1):
            shade(f"shade-{f}-direct-ls{ls}", f, "direct", light_strategy=ls)
        shade(f"shade-{f}-whitted", f, "whitted")
        shade(f"shade-{f}-ao", f, "ao", ao_samples=4)
        for so in (0, 1, 2):  # 64 x 64 x 4: more than 1024 paths to shade after the camera hits, so shade_order 2 sorts the queue
            shade(f"shade-{f}-path-order{so}", f, "path", w=64, h=64, shade_order=so)
    for f in ("matte", "maps", "shapes"):  # the three builds of the spatial light table (each scene holds two lights or more)
        shade(f"shade-{f}-path-spatial", f, "path", light_strategy=2)
    shade("shade-matte-path-two-passes", "matte", "path", spp_per_pass=2)

    def trace(scene, traversal, counting):
        name = {AUTO: "auto", STACK: "stack", STACKLESS: "stackless"}[traversal]
        out.append(dict(id=f"trace-{scene}-{name}-count{counting}", kind="trace", scene=scene, traversal=traversal, counting=counting,
                        wide=scene in WIDE_SCENES and traversal == AUTO and counting != 1))

    for c in (0, 1, 2):
        trace("matte", AUTO, c)
    for c in (0, 1):
        trace("matte", STACK, c)
    trace("matte", STACKLESS, 0)  # the stackless walk has no counting variant
    for scene in ("spheres", "shapes"):
        for c in (0, 1):
            trace(scene, AUTO, c)
    for scene in ("instanced", "two_level"):
        for c in (0, 1, 2):
            trace(scene, AUTO, c)
        for c in (0, 1):
            trace(scene, STACK, c)
    # 512 x 512 x 8 = 2^21 paths: the second bounce still holds more than 2^20 rays, so ray_order 0 sorts them
    out.append(dict(id="raysort-rand20k", kind="raysort", scene="rand20k"))
    assert len({c["id"] for c in out}) == len(out)
    return out


# ---- running one case ----
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _render(g, cam_fn, w, h, spp, integ, depth, **kw):
    film, st = g.render(cam_fn(w, h), w, h, spp, integrator=integ, max_depth=depth, seed=7, **kw)
    return dict(film=_sha(film), rays_closest=int(st["rays_closest"]), rays_shadow=int(st["rays_shadow"]),
                camera_samples=int(st["camera_samples"]))


class SceneCache:
    """Device scenes by name, built on first use and closed together."""

    def __init__(self, ctx):
        self.ctx, self.built = ctx, {}

    def get(self, name):
        if name not in self.built:
            sc, cam_fn = SCENES[name]()
            self.built[name] = (pbrt_hip.Scene(self.ctx, sc), cam_fn)
        return self.built[name]

    def close(self):
        for g, _ in self.built.values():
            g.close()
        self.built = {}


def run_case(ctx, cache, case):
    """What the fixture stores for `case`, computed by the loaded library. Leaves the context at TRAVERSAL_AUTO, counting off."""
    g, cam_fn = cache.get(case["scene"])
    if case["kind"] == "shade":
        return _render(g, cam_fn, case["width"], case["height"], SPP, INTEGRATORS[case["integrator"]], DEPTH, **case["kw"])
    if case["kind"] == "raysort":
        return {f"ray_order{ro}": _render(g, cam_fn, 512, 512, 8, PATH, 4, ray_order=ro) for ro in (0, 1)}
    res = dict(wide_records=g.wide_records()[0] > 0)
    try:
        ctx.set_traversal(case["traversal"])
        ctx.set_counting(case["counting"])
        ctx.counters(reset=True)
        ctx.wide_counters(reset=True)

        def counted():
            c, wc = ctx.counters(reset=True), ctx.wide_counters(reset=True)
            if case["counting"] == 1:
                return dict(node_tests=c["node_tests"], prim_tests=c["prim_tests"])
            if case["counting"] == 2 and case["wide"]:
                return dict(records=wc["records"], triangles=wc["triangles"])
            return None

        res["render"] = _render(g, cam_fn, W, H, SPP, PATH, DEPTH)
        res["render_counters"] = counted()
        centre, extent = RAY_BOX[case["scene"]]
        rays = scenes.random_rays(N_RAYS, 17, origin_extent=extent)
        rays["o"] += np.float32(centre)
        rays["t_max"][::7] = np.float32(0.5 * extent)
        hits = g.intersect(rays)
        res["hits"] = _sha(hits)
        res["n_hit"] = int(np.count_nonzero(hits["prim_id"] >= 0))
        res["intersect_counters"] = counted()
        res["occluded"] = _sha(g.intersect_p(rays))
        res["intersect_p_counters"] = counted()
    finally:
        ctx.set_traversal(AUTO)
        ctx.set_counting(0)
    return res


def main():
    ctx = pbrt_hip.Context(0)
    cache = SceneCache(ctx)
    recorded, excluded = {}, []
    for case in cases():
        a, b = run_case(ctx, cache, case), run_case(ctx, cache, case)
        if a != b:
            excluded.append(case["id"])
            print("NOT REPRODUCIBLE, excluded:", case["id"], a, b)
            continue
        recorded[case["id"]] = a
        print(case["id"], json.dumps(a))
    cache.close()
    ctx.close()
    all_cases = cases()
    assert len(excluded) * 20 <= len(all_cases), ("more than 5 % of the cases are not reproducible", excluded)
    for f in FEATURES:
        for integ in INTEGRATORS:
            assert any(c["kind"] == "shade" and c["feature"] == f and c["integrator"] == integ and c["id"] in recorded for c in all_cases), (f, integ)
    with open(FIXTURE, "w") as fh:
        json.dump(dict(cases=recorded, excluded=excluded), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(recorded)} cases written to {FIXTURE}, {len(excluded)} excluded")


if __name__ == "__main__":
    main()
