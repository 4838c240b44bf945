"""Moving instances on the GPU, second pass: the path's time across bounces, rows under scale and shear at the shaded hit, deep
top-level trees and the counting builds, the ends of the time range, the render driver and the material levels of the moving
shading builds, against the float64 model (tests/motion_model.py) through the cases of tests/motion_cases.py, which
tests/test_motion_cases_model.py holds to the model without a GPU.

Allowances that are measured, not chosen (as test_gpu_motion.py::test_hits_against_the_model): the same rays are first traced
through STATIC instances frozen at the model's matrices, per time; the worst error of that path against the model is the
baseline and the moving path is allowed 4 times it. Each test prints both figures; its docstring records them.

pbrt_hip_scene_set_shading_data takes one mesh for the whole scene and the two-level creation calls have no per-object normals,
so no smooth-normal object is part of the Lambert case.
"""
import numpy as np
import pytest

import closed_forms_samplers as cs
import motion_cases as mc
import pbrt_hip
from pbrt_hip import scenes

pytestmark = pytest.mark.gpu

N = mc.N_RAYS
KEYS = np.arange(N, dtype=np.uint64) + 1
INTEGRATORS = {"path": pbrt_hip.INTEGRATOR_PATH, "whitted": pbrt_hip.INTEGRATOR_WHITTED, "direct": pbrt_hip.INTEGRATOR_DIRECT,
               "ao": pbrt_hip.INTEGRATOR_AO}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_root(*scenes_):
    r = [s.tlas_nodes[0] for s in scenes_]
    return all(np.array_equal(x["bmin"], r[0]["bmin"]) and np.array_equal(x["bmax"], r[0]["bmax"]) for x in r[1:])


def create(hip_ctx, scene):
    g = pbrt_hip.Scene(hip_ctx, scene)
    if "set_roughness" in scene:
        row, u, v = scene["set_roughness"]
        g.set_material_roughness(row, u, v, remap=False)
    return g


def per_time_frozen(hip_ctx, instances, objects, rays, build, call, out):
    """`call(scene, rays)` on static instances frozen at the model's matrices, one scene per time, gathered into `out`"""
    for t in np.unique(rays["time"]):
        g = create(hip_ctx, build(mc.frozen(instances, objects, t)))
        sel = rays["time"] == t
        out[sel] = call(g, rays[sel], sel)
        g.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. time stays with its path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def path_time(hip_ctx):
    case = mc.path_time_case()
    g = {k: pbrt_hip.Scene(hip_ctx, case[k]) for k in ("moving", "covers", "away")}
    yield case, g
    for s in g.values():
        s.close()


@pytest.mark.parametrize("name", ["path", "whitted", "direct"])
def test_time_stays_with_its_path(path_time, name):
    """Specular chains (a mirror, two mirrors, a glass pane with its reflect and transmit branches) that end on an emitter or on a
    black quad sliding in front of it, 4096 rays of four classes interleaved over 8 times. Every ray's radiance equals, bit for
    bit, that of the static scene the model picks for it: the occluder covering its chain at the ray's own time, or out of the way.
    A continuation ray that carried another time (another path's, the start, none) sees the quad elsewhere."""
    case, g = path_time
    assert same_root(*g.values())
    rays, cls, keep, covered = case["rays"], case["cls"], case["keep"], case["covered"]
    kw = dict(integrator=INTEGRATORS[name], max_depth=4, light_strategy=0 if name == "direct" else 1)
    got, covers, away = (g[k].li(rays, KEYS, **kw)[0] for k in ("moving", "covers", "away"))
    expect = np.where(covered[:, None], covers, away)
    differ = (bits(covers) != bits(away)).any(axis=1)
    wrong = keep & (bits(got) != bits(expect)).any(axis=1)
    print(f"{name}: {wrong.sum()} of {keep.sum()} rays differ from their static scene; the two static scenes differ on {differ.sum()}")
    # the comparison can tell: a chain that reaches the emitter carries light, one that ends on the quad none of it
    assert (away[cls == 0] == 0.0).all() and (got[cls == 0] == 0.0).all()
    for k in (1, 2):
        assert differ[cls == k].all() and (away[cls == k] > 0.0).all()
    if name == "path":       # the pane: one branch per path, chosen by the stream; the reflect branch does not see the quad
        assert 0.5 < differ[cls == 3].mean() < 1.0
    else:                    # both branches: the reflect branch's light is there with and without the quad
        assert differ[cls == 3].all() and (covers[cls == 3] > 0.0).all()
        switched = keep & (cls == 3) & (covered != case["covered_at_start"])
        assert switched.sum() >= 2 * mc.MIN_SWITCHED
    assert not wrong.any(), np.flatnonzero(wrong)[:10]


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows under scale and shear at the shaded hit
# ---------------------------------------------------------------------------------------------------------------------
def test_lamberts_law_under_scale_and_shear(hip_ctx):
    """Matte instances under a distant light: the normal through (M(t)^-1)^T of the interpolated matrix, on a box and a quad that
    are turned, scaled along other axes than their own and turned again, and on a sheared box. The allowance is
    test_gpu_motion.py's NORMAL_TOL times cond_2 of M(t)'s linear part. Measured on gfx950 (MI355X): worst deviation 2.028e-07
    over 1250 lit hits (the smallest allowance is 2.4e-04)."""
    case = mc.lambert_case()
    rays, m = case["rays"], case["m"]
    light = (scenes.distant_light(mc.ROW_WI, (mc.LIGHT_L,) * 3),)
    g = pbrt_hip.Scene(hip_ctx, mc.row_scene(mc.ROW_INSTANCES, True, light))
    rgb, _ = g.li(rays, KEYS, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    hits = g.intersect(rays)
    g.close()
    mc.check_ids("scaled and sheared instances", hits, m)
    keep = ~m["unsure"]
    got = rgb.astype(np.float64) * (np.pi / (mc.KD * mc.LIGHT_L))
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 1], got[:, 2])
    assert (rgb[keep & ~m["hit"]] == 0.0).all()
    dev = np.abs(got[:, 0] - case["expect"])
    lit = keep & (case["expect"] > 0.05)
    print(f"scale and shear: {lit.sum()} lit hits, worst deviation {dev[keep].max():.3e}, worst deviation / allowance {(dev / case['tol'])[keep].max():.3e}")
    assert lit.sum() > 800
    assert np.all(dev[keep] <= case["tol"][keep])


@pytest.mark.parametrize("name", list(mc.ANISO_ROWS))
def test_anisotropic_rows_under_scale_and_shear(hip_ctx, name):
    """An anisotropic metal row (alphas 0.15, 0.6) and an anisotropic Disney row on the same instances under a point light,
    direct lighting, one bounce: f(wo, wi) I |n . wi| / r^2 with wo and wi in the model's frame (n through (M^-1)^T, dpdu through
    M). Rays whose model value is below 1e-3 in every channel are left out; the error is relative, per channel.
    Measured on gfx950 (MI355X), worst relative error: metal, 1198 rays kept: static baseline 2.364840e-06, moving path
    4.055898e-06 (allowed 9.459360e-06); Disney, 1153 rays kept: static baseline 2.961105e-06, moving path 3.504698e-06 (allowed
    1.184442e-05)."""
    case = mc.aniso_case(name)
    rays, ref, keep = case["rays"], case["ref"], case["keep"]
    light = (scenes.point_light(mc.ROW_LIGHT_P, mc.ROW_LIGHT_I),)
    kw = dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    base = per_time_frozen(hip_ctx, mc.ROW_INSTANCES, mc.OBJECTS, rays, lambda inst: mc.row_scene(inst, False, light, name),
                           lambda g, r, sel: g.li(r, KEYS[sel], **kw)[0], np.zeros((N, 3), np.float32))
    g = create(hip_ctx, mc.row_scene(mc.ROW_INSTANCES, True, light, name))
    got, _ = g.li(rays, KEYS, **kw)
    g.close()
    e_base, e_got = mc.aniso_error(base, ref, keep), mc.aniso_error(got, ref, keep)
    print(f"{name}: {keep.sum()} rays kept; worst relative error: static baseline {e_base.max():.6e}, moving path {e_got.max():.6e} "
          f"(allowed {4 * e_base.max():.6e}; recorded baseline {mc.ANISO_BASELINE_RECORDED[name]:.1e})")
    assert keep.sum() >= mc.MIN_KEPT
    assert (got[keep].max(axis=1) > 0.0).all()
    assert e_got.max() <= 4 * e_base.max()
    assert e_base.max() <= mc.ANISO_BASELINE_RECORDED[name]     # what the CPU test's sensitivity checks take as the allowance


def test_shadow_rays_start_on_the_scaled_box(hip_ctx):
    """The scaled, turning box just above a static matte plane under a low distant light. A point of the plane is dark exactly
    while the ray from it towards the light meets the box at the ray's time (the model's brute force); a lit face of the box is
    not in its own shadow and follows Lambert's law: the shadow ray leaves from p + the offset of p_error, both through the
    interpolated o2w."""
    case = mc.shadow_start_case()
    rays, keep = case["rays"], case["keep"]
    g = pbrt_hip.Scene(hip_ctx, mc.stand_scene())
    rgb, _ = g.li(rays, KEYS, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    g.close()
    assert 1.0 - keep.mean() <= mc.MAX_EXCLUDED
    dark, lit_plane = keep & case["dark"], keep & case["on_plane"] & ~case["dark"]
    assert (rgb[dark] == 0.0).all(), (rgb[dark] != 0.0).any(axis=1).sum()
    assert np.allclose(rgb[lit_plane].astype(np.float64), mc.KD / np.pi * mc.LIGHT_L * mc.STAND_WI[2], rtol=1e-5, atol=0.0)
    box = keep & case["on_box"]
    got = rgb[:, 1].astype(np.float64) * (np.pi / (mc.KD * mc.LIGHT_L))
    lit = box & (case["lambert"] > 0.05)
    print(f"box on the plane: {dark.sum()} dark and {lit_plane.sum()} lit points, {lit.sum()} lit hits on the box, "
          f"worst deviation / allowance {(np.abs(got - case['lambert'])[box] / case['tol'][box]).max():.3e}")
    assert (got[lit] > 0.0).all()                                   # none in its own shadow
    assert np.all(np.abs(got - case["lambert"])[box] <= case["tol"][box])


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth, counting and the bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", [2, 1])
def test_sixty_four_instances_against_brute_force(hip_ctx, n_objects):
    """64 overlapping instances (negated quaternions, the normalised-lerp branch, changing non-uniform scale, static ones among
    them), a top-level tree of five levels or more; two objects and world triangles (the kernels' INST = 2) or one box (INST = 1).
    Hit ids, instance ids and any-hit equal the model's brute force over all triangles; t within 4 times the static-frozen
    baseline; the counting builds give the same records bit for bit.
    Measured on gfx950 (MI355X), worst relative error of t: INST = 2: static baseline 1.681690e-06, moving path 1.280483e-06
    (allowed 6.726759e-06), hits by kind 530 / 591 / 509 / 391 / 1914; INST = 1: static baseline 3.916577e-06, moving path
    3.916577e-06 (allowed 1.566631e-05), hits by kind 430 / 484 / 533 / 523 / 1962."""
    case = mc.depth_case(n_objects)
    inst, objects, rays, m = case["instances"], case["objects"], case["rays"], case["m"]
    build = lambda instances, moving=False: mc.make_scene(instances, world=case["world"], moving=moving, objects=objects)   # noqa: E731
    base = per_time_frozen(hip_ctx, inst, objects, rays, build, lambda g, r, sel: g.intersect(r), np.zeros(N, dtype=scenes.HIT_DTYPE))
    _, base_rel = mc.check_ids("static instances at the interpolated matrices", base, m)
    g = pbrt_hip.Scene(hip_ctx, build(inst, True))
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    hip_ctx.set_counting(1)
    try:
        hip_ctx.counters(reset=True)
        counted, counted_any = g.intersect(rays), g.intersect_p(rays)
        counters = hip_ctx.counters(reset=True)
    finally:
        hip_ctx.set_counting(0)
    g.close()
    sel, rel = mc.check_ids("moving instances", hits, m)
    kinds = case["kinds"][m["inst"][sel]]
    print(f"INST = {n_objects}: worst relative error of t: static baseline {base_rel.max():.6e}, moving path {rel.max():.6e} "
          f"(allowed {4 * base_rel.max():.6e}); hits by kind {[int((kinds == k).sum()) for k in range(5)]}; counters {counters}")
    for k in range(3):
        assert (kinds == k).sum() >= mc.MIN_KIND_HITS, mc.KINDS[k]
    assert rel.max() <= 4 * base_rel.max()
    keep = ~m["unsure"]
    assert np.array_equal(anyhit.astype(bool)[keep], m["hit"][keep])
    # the counting builds
    assert np.array_equal(counted.view(np.uint8), hits.view(np.uint8))
    assert np.array_equal(counted_any, anyhit)
    assert counters["rays"] > 0 and counters["node_tests"] > 0 and counters["prim_tests"] > 0 and counters.get("inst_tests", 0) > 0


@pytest.mark.parametrize("n_objects", [2, 1])
def test_li_under_counting_is_li(hip_ctx, n_objects):
    """The counting builds of the wavefront's own traversal kernel (k_trace_moving<true, INST>, which only li and render launch;
    intersect and intersect_p above go through k_intersect_batch_moving): on the 64-instance scenes, with matte, glass and mirror
    instances under the sun and a dim sky, the radiance of all four integrators with set_counting(1) equals the radiance with
    counting off bit for bit, and the counters are not zero."""
    case = mc.depth_case(n_objects)
    lights = mc.SUN + ((scenes.LIGHT_INFINITE, (0.2, 0.25, 0.3), -1, 0, 1),)
    rows = np.where(np.arange(64) % 4 == 3, -1, np.arange(64) % 3)          # matte, glass, mirror, the object's own (matte)
    g = pbrt_hip.Scene(hip_ctx, mc.make_scene(case["instances"], world=case["world"], lights=lights, objects=case["objects"], instance_material=rows))
    assert g.motions["animated"].sum() == 56
    rays = case["rays"]
    try:
        for name, integrator in INTEGRATORS.items():
            kw = dict(integrator=integrator, max_depth=4, ao_samples=4, light_strategy=0 if name == "direct" else 1)
            plain, st = g.li(rays, KEYS, **kw)
            hip_ctx.set_counting(1)
            hip_ctx.counters(reset=True)
            counted, st_c = g.li(rays, KEYS, **kw)
            counters = hip_ctx.counters(reset=True)
            hip_ctx.set_counting(0)
            print(f"INST = {n_objects}, {name}: {len(np.unique(plain, axis=0))} different radiances, counters {counters}")
            assert np.array_equal(bits(counted), bits(plain)), name
            assert (st_c["rays_closest"], st_c["rays_shadow"]) == (st["rays_closest"], st["rays_shadow"]), name
            assert counters["rays"] > 0 and counters["node_tests"] > 0 and counters["prim_tests"] > 0 and counters.get("inst_tests", 0) > 0, name
            # no trivial result: the paths do meet the instances (AO with 4 samples takes few values: k / 4 of pi and its roundings)
            assert len(np.unique(plain, axis=0)) > (10 if name == "ao" else 500), name
    finally:
        hip_ctx.set_counting(0)
        g.close()


def test_counters_of_an_all_static_scene_are_the_old_scenes(hip_ctx):
    case = mc.depth_case(2)
    static = [(k, m0, None) for k, m0, _ in case["instances"]]
    rays = case["rays"]
    res = []
    hip_ctx.set_counting(1)
    try:
        for moving in (False, True):
            g = pbrt_hip.Scene(hip_ctx, mc.make_scene(static, world=case["world"], moving=moving))
            hip_ctx.counters(reset=True)
            res.append((g.intersect(rays), g.intersect_p(rays), hip_ctx.counters(reset=True)))
            g.close()
    finally:
        hip_ctx.set_counting(0)
    assert np.array_equal(res[0][0].view(np.uint8), res[1][0].view(np.uint8)) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] and res[0][2]["node_tests"] > 0 and res[0][2].get("inst_tests", 0) > 0, (res[0][2], res[1][2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the ends of the range
# ---------------------------------------------------------------------------------------------------------------------
def test_the_ends_of_the_time_range(hip_ctx):
    """Rays at exactly start_time and end_time and at the floats next to them. At and before the start: the static scene at the
    start rows, bit for bit, hits and the radiance of all four integrators; at and after the end: the static scene that holds
    the end matrix and its inverse (computed in double, rounded once). Just inside either end: the model's ids, t within 4
    times the static-frozen baseline (no jump).
    Measured on gfx950 (MI355X), 556 hits just inside: static baseline 7.977691e-07, moving path 8.993966e-07 (allowed
    3.191077e-06)."""
    times = mc.end_times()
    rays = mc.rays_at(mc.CENTRES, 91, times)
    g = {k: pbrt_hip.Scene(hip_ctx, mc.end_scene(k)) for k in ("moving", "start", "end")}
    assert same_root(*g.values())
    assert g["moving"].motions["animated"].sum() == 4
    at_start, at_end = rays["time"] <= times[1], rays["time"] >= times[4]
    inside = ~at_start & ~at_end
    assert at_start.sum() > 1000 and at_end.sum() > 1000 and inside.sum() > 1000
    hits = {k: s.intersect(rays) for k, s in g.items()}
    occl = {k: s.intersect_p(rays) for k, s in g.items()}
    for sel, k in ((at_start, "start"), (at_end, "end")):
        assert np.array_equal(hits["moving"][sel].view(np.uint8), hits[k][sel].view(np.uint8)), k
        assert np.array_equal(occl["moving"][sel], occl[k][sel]), k
        assert (hits[k]["instance_id"][sel] >= 0).sum() > 300
    # the end is not the start: the two static scenes differ on the rays that meet a moving instance
    assert (hits["start"]["t"] != hits["end"]["t"]).sum() > 500
    for name, integrator in INTEGRATORS.items():
        kw = dict(integrator=integrator, max_depth=3, ao_samples=4, light_strategy=0 if name == "direct" else 1)
        li = {k: s.li(rays, KEYS, **kw)[0] for k, s in g.items()}
        for sel, k in ((at_start, "start"), (at_end, "end")):
            assert np.array_equal(bits(li["moving"][sel]), bits(li[k][sel])), (name, k)
        assert li["moving"].max() > 0.0 and (bits(li["start"]) != bits(li["end"])).any(axis=1).sum() > 200, name
    for s in g.values():
        s.close()
    # just inside: the instances alone (the model knows nothing else), as test_gpu_motion.py::test_hits_against_the_model
    near = rays[inside]
    m = mc.model_hits(mc.FIVE, near)
    base = per_time_frozen(hip_ctx, mc.FIVE, mc.OBJECTS, near, lambda inst: mc.make_scene(inst, moving=False),
                           lambda s, r, sel: s.intersect(r), np.zeros(len(near), dtype=scenes.HIT_DTYPE))
    alone = pbrt_hip.Scene(hip_ctx, mc.make_scene(mc.FIVE))
    inner = alone.intersect(near)
    alone.close()
    _, base_rel = mc.check_ids("static instances just inside the ends", base, m)
    sel, rel = mc.check_ids("moving instances just inside the ends", inner, m)
    print(f"just inside the ends: {sel.sum()} hits, worst relative error of t: static baseline {base_rel.max():.6e}, moving path "
          f"{rel.max():.6e} (allowed {4 * base_rel.max():.6e})")
    assert sel.sum() > 500 and rel.max() <= 4 * base_rel.max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the render driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blur(hip_ctx):
    g = pbrt_hip.Scene(hip_ctx, mc.blur_scene())
    yield g, scenes.orthographic_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 2.0, mc.RES, mc.RES)
    g.close()


BLUR_KW = dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0, seed=3)


def test_tile_shares_of_a_moving_scene_add_up(blur):
    g, cam = blur
    whole, _ = g.render(cam, mc.RES, mc.RES, 16, **BLUR_KW)
    assert pbrt_hip.film_to_rgb(whole).max() > 0.0
    for order in (0, 1):
        parts = [g.render(cam, mc.RES, mc.RES, 16, tile_rank=r, tile_world=2, tile_order=order, **BLUR_KW)[0] for r in (0, 1)]
        assert all(p[..., 3].max() > 0.0 for p in parts)                         # each rank has tiles of its own
        assert not ((parts[0][..., 3] > 0.0) & (parts[1][..., 3] > 0.0)).any()   # ... and no pixel twice
        assert np.array_equal(bits(parts[0] + parts[1]), bits(whole)), order


def test_li_on_camera_rays_reproduces_the_render_of_a_moving_scene(blur):
    """as test_gpu_li.py::test_li_on_camera_rays_reproduces_render_bit_for_bit, with an open shutter: camera_rays hands the
    rays' times on, li traces every ray at its own"""
    g, cam = blur
    w = h = mc.RES
    spp = 16
    film, st = g.render(cam, w, h, spp, **BLUR_KW)
    rays, keys, pfilm, pix = g.camera_rays(cam, w, h, spp, seed=3)
    valid = pix[:, 0] >= 0
    assert valid.sum() == w * h * spp
    assert len(np.unique(rays["time"][valid])) > 0.9 * valid.sum() and rays["time"][valid].min() >= 0.0 and rays["time"][valid].max() < 1.0
    x, y, s = (pix[valid, k].astype(np.int64) for k in range(3))
    rgb, st_li = g.li(rays[valid], keys[valid], integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0, draws_before_li=5)
    assert st_li["rays_closest"] + st_li["rays_shadow"] == st["rays_closest"] + st["rays_shadow"]
    f32 = np.float32
    acc = np.zeros((h, w, 3), dtype=np.float32)
    order = np.lexsort((s, x, y))
    assert np.array_equal(np.floor(pfilm[valid]).astype(np.int64), np.stack([x, y], axis=1))
    for k in range(spp):            # the k-th sample of every pixel at once: per pixel the additions stay in sample order
        sel = order[k::spp]
        assert np.array_equal(s[sel], np.full(len(sel), k))
        acc[y[sel], x[sel]] += rgb[sel]
    xyz = np.stack([f32(0.412453) * acc[..., 0] + f32(0.357580) * acc[..., 1] + f32(0.180423) * acc[..., 2],
                    f32(0.212671) * acc[..., 0] + f32(0.715160) * acc[..., 1] + f32(0.072169) * acc[..., 2],
                    f32(0.019334) * acc[..., 0] + f32(0.119193) * acc[..., 1] + f32(0.950227) * acc[..., 2]], axis=-1)
    assert np.array_equal(film[..., 3], np.full((h, w), spp, dtype=np.float32))
    assert xyz.astype(np.float32).tobytes() == np.ascontiguousarray(film[..., :3]).tobytes()
    # the film is blurred: pixels that the quad covers for a part of the shutter only
    part = (acc[..., 1] > 0.0) & (acc[..., 1] < acc[..., 1].max() * 0.99)
    assert part.sum() > 500


def _times(g, cam, spp, sampler, seed=0):
    rays, _, _, pix = g.camera_rays(cam, 16, 16, spp, seed=seed, sampler=sampler)
    ok = pix[:, 0] >= 0
    return rays["time"][ok], pix[ok]


def test_camera_rays_return_the_samplers_first_1d_draw_as_the_time(blur):
    """ray.time = lerp(u, shutter_open, shutter_close) with u the sampler's first 1D draw (sampler.rs:66-73). With the shutter
    [0, 1] the lerp is exact and the time is the draw: one per stratum per pixel for the stratified sampler (the centres,
    un-jittered), one per interval of 1 / n for the (0, 2) sampler, the scrambled radical inverse in base 5 of the sample's index
    for the Halton sampler (its third dimension), under one digit permutation. Another shutter maps the same draws; a shutter of
    no length gives shutter_open. The issue asks for exactly shutter_open at every such shutter; the reference's lerp,
    (1 - u) a + u a, which the device evaluates as written, gives exactly a only where its two products are exact (a = 0 or a
    power of two: held exactly for 0, 1 and 4). For a = 0.75 the products round, so the test departs from the issue's wording
    there: the times are held to the float32 formula bit for bit and to 0.75 within one ulp."""
    g, _ = blur
    cam = scenes.orthographic_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 2.0, 16, 16)
    assert cam["shutter_open"] == 0.0 and cam["shutter_close"] == 1.0
    # stratified: nx * ny strata of the 1D dimension per pixel
    for nx, ny in ((4, 4), (3, 5)):
        n = nx * ny
        t, pix = _times(g, cam, n, ("stratified", nx, ny, True, 3), seed=5)
        assert len(t) == 256 * n
        cs.check_unit_interval(t)
        orders = set()
        for py in range(16):
            for px in range(16):
                sel = (pix[:, 0] == px) & (pix[:, 1] == py)
                u = t[sel][np.argsort(pix[sel, 2])]
                cs.check_one_per_interval(u, n)
                orders.add(tuple(np.floor(u.astype(np.float64) * n).astype(int)))
        assert len(orders) > 200                     # shuffled pixel by pixel
        t, pix = _times(g, cam, n, ("stratified", nx, ny, False, 3), seed=1)
        centres = np.minimum((np.arange(n, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(n)), cs.ONE_MINUS_EPSILON)
        sel = (pix[:, 0] == 7) & (pix[:, 1] == 3)
        assert sorted(t[sel].tolist()) == sorted(centres.tolist())
    # (0, 2): van der Corput under a random digit scramble
    n = 16
    t, pix = _times(g, cam, n, ("zerotwo", 3), seed=3)
    assert len(t) == 256 * n
    cs.check_unit_interval(t)
    tables = set()
    for py in range(16):
        for px in range(16):
            sel = (pix[:, 0] == px) & (pix[:, 1] == py)
            u = t[sel][np.argsort(pix[sel, 2])]
            cs.check_one_per_interval(u, n)
            tables.add(u.tobytes())
    assert len(tables) > 240                         # each pixel under its own scramble
    # Halton
    spp = 4
    t, pix = _times(g, cam, spp, ("halton",))
    _, idx = cs.halton_camera_samples(16, 16, spp)
    fits = mc.halton_time_permutation(idx[pix[:, 1], pix[:, 0], pix[:, 2]], t.astype(np.float64))
    assert len(fits) == 1, fits
    # another shutter: the same draws, mapped; no length: shutter_open
    random_u, pix_u = _times(g, cam, 4, None, seed=9)
    cs.check_unit_interval(random_u)
    assert len(np.unique(random_u)) > 1000
    cam2 = cam.copy()
    cam2["shutter_open"], cam2["shutter_close"] = 0.25, 1.75
    t2, pix2 = _times(g, cam2, 4, None, seed=9)
    assert np.array_equal(pix_u, pix2)
    back = (t2.astype(np.float64) - 0.25) / 1.5
    assert np.abs(back - random_u).max() <= 2 ** -23 and t2.min() >= 0.25 and t2.max() <= 1.75
    want = (np.float32(1.0) - random_u) * np.float32(0.25) + random_u * np.float32(1.75)
    assert np.array_equal(bits(t2), bits(want.astype(np.float32)))
    # lerp(u, a, a) = (1 - u) a + u a is exactly a for every u where a is a power of two (or 0); elsewhere the two products round
    for a, exact in ((1.0, True), (0.0, True), (4.0, True), (0.75, False)):
        cam2["shutter_close"] = cam2["shutter_open"] = a
        t3, _ = _times(g, cam2, 4, None, seed=9)
        if exact:
            assert (t3 == np.float32(a)).all(), a
        assert np.array_equal(bits(t3), bits(((np.float32(1.0) - random_u) * np.float32(a) + random_u * np.float32(a)).astype(np.float32))), a
        assert np.abs(t3.astype(np.float64) - a).max() <= 2.0 ** -23 * a, a


# ---------------------------------------------------------------------------------------------------------------------
# 6. material levels through the moving builds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3])
def test_material_levels_through_the_moving_builds(hip_ctx, level):
    """An all-static scene created through the moving entry point shades with the moving builds (the level-3 BSDF set); the old
    scene with a plastic and a metal row takes k_shade<., 1>, with set_material rows on top k_shade<., 2>, with a Disney row
    k_shade<., 3>. The films of all four integrators are the same bit for bit."""
    old_scene, new_scene = mc.level_scenes(level)
    old, new = pbrt_hip.Scene(hip_ctx, old_scene), pbrt_hip.Scene(hip_ctx, new_scene)
    assert new.motions is not None and not new.motions["animated"].any()
    cam = scenes.perspective_camera((1.0, -7.0, 4.0), (0, 0, 0), (0, 0, 1), 50.0, 48, 48)
    for name, integrator in INTEGRATORS.items():
        kw = dict(integrator=integrator, max_depth=4, ao_samples=4, light_strategy=0 if name == "direct" else 1)
        a, _ = old.render(cam, 48, 48, 4, **kw)
        b, _ = new.render(cam, 48, 48, 4, **kw)
        differ = (bits(a) != bits(b)).any(axis=-1)
        print(f"level {level}, {name}: {differ.sum()} of {differ.size} pixels differ, largest difference {np.abs(a - b).max():.3e}")
        assert not differ.any(), (level, name)
        assert pbrt_hip.film_to_rgb(a).max() > 0.0
    old.close()
    new.close()
