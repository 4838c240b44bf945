"""Moving instances on the GPU (pbrt_hip_scene_create_two_level_moving): hits, normals, shadow rays and motion blur against
the float64 model of tests/motion_model.py and against closed forms.

Objects: a two-triangle quad and a 12-triangle box; 5 instances; 4096 rays.

Tolerance of t in test_hits_against_the_model: measured, not chosen. The same rays are first traced through STATIC instances
whose matrices are the model's interpolated ones rounded to float (the kernels every two-level scene has always used); their
worst relative error in t against the model is the baseline, and the moving path (which adds the float32 roundings of compose and
invert) is allowed 4 times that. On gfx950 (MI355X): baseline 1.226936e-06, moving path 1.226936e-06 (the worst ray is one that
meets a stored matrix on both paths; over the hits that went through the interpolation: baseline 9.253821e-07, moving path 8.987490e-07).
"""
import numpy as np
import pytest

import motion_model as mm
import pbrt_hip
from pbrt_hip import scenes

pytestmark = pytest.mark.gpu

# the scenes' parts and helpers live in tests/motion_cases.py, which test_gpu_motion_paths.py shares
from motion_cases import (BLUR_SHIFT, BLUR_START, BOX, CENTRES, FIVE, FLOOR, KD, LIGHT_L, N_RAYS, NORMAL_TOL, QUAD, RES, SPP, SUN, T0, T1,  # noqa: F401
                          blur_scene, check_ids, make_scene, model_hits, model_instances, rays_at, rot, some_times, tr)


# ---------------------------------------------------------------------------------------------------------------------
# a scene in which nothing moves is the old scene
# ---------------------------------------------------------------------------------------------------------------------

def test_all_static_scene_is_the_old_scene(hip_ctx):
    static = [(k, m0, None) for k, m0, _ in FIVE]
    old = pbrt_hip.Scene(hip_ctx, make_scene(static, world=FLOOR, lights=SUN, moving=False))
    new = pbrt_hip.Scene(hip_ctx, make_scene(static, world=FLOOR, lights=SUN))       # through pbrt_hip_scene_create_two_level_moving
    assert new.motions is not None and not new.motions["animated"].any()
    assert old.wide_records() == new.wide_records()
    rays = rays_at(CENTRES, 1, some_times(2))
    assert np.array_equal(old.intersect(rays).view(np.uint8), new.intersect(rays).view(np.uint8))
    assert np.array_equal(old.intersect_p(rays), new.intersect_p(rays))
    cam = scenes.perspective_camera((1.0, -7.0, 4.0), (0, 0, 0), (0, 0, 1), 50.0, 48, 48)
    for integrator in (pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO):
        a, _ = old.render(cam, 48, 48, 4, integrator=integrator, max_depth=3, ao_samples=4)
        b, _ = new.render(cam, 48, 48, 4, integrator=integrator, max_depth=3, ao_samples=4)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), integrator
        assert pbrt_hip.film_to_rgb(a).max() > 0.0
    old.close()
    new.close()


def test_static_instance_beside_a_moving_one(hip_ctx):
    """Only instance 1 moves; the hits on the others are those of the scene without it, bit for bit."""
    one = [(k, m0, m1 if i == 1 else None) for i, (k, m0, m1) in enumerate(FIVE)]
    rest = [e for i, e in enumerate(one) if i != 1]
    moving = pbrt_hip.Scene(hip_ctx, make_scene(one))
    static = pbrt_hip.Scene(hip_ctx, make_scene(rest, moving=False))
    assert moving.wide_records() == (-1, "scene with moving instances")
    rays = rays_at(CENTRES, 3, some_times(4))
    a, b = moving.intersect(rays), static.intersect(rays)
    moving.close()
    static.close()
    sel = (a["instance_id"] >= 0) & (a["instance_id"] != 1)
    assert sel.sum() > 500 and (a["instance_id"] == 1).sum() > 100
    renumbered = np.where(a["instance_id"] > 1, a["instance_id"] - 1, a["instance_id"])
    assert np.array_equal(renumbered[sel], b["instance_id"][sel])
    for k in ("t", "b0", "b1", "b2"):
        assert np.array_equal(a[k][sel].view(np.uint32), b[k][sel].view(np.uint32)), k
    assert np.array_equal(a["prim_id"][sel], b["prim_id"][sel])


# ---------------------------------------------------------------------------------------------------------------------
# exact interpolation
# ---------------------------------------------------------------------------------------------------------------------
def test_translation_by_powers_of_two_is_exact(hip_ctx):
    """Translated from (-1, 0.5, 0.25) to (1, 1.5, 0.75) over [0, 2]: at time 1 every product and sum of the interpolation is
    exact, and the result is a static instance at (0, 1, 0.5) bit for bit. Fails if the time does not reach the kernel (the
    instance would stand at its start) or if compose / invert round anywhere."""
    box_at = lambda v: (1, tr(*v), None)
    others = [(0, tr(-2, 0, 0), None), (1, tr(2, 0, 0), None)]
    scene_m = make_scene([(1, tr(-1, 0.5, 0.25), tr(1, 1.5, 0.75))] + others)
    scene_m["instance_motion"] = {0: scenes.instance_motion(tr(1, 1.5, 0.75), 0.0, 2.0)}
    moving = pbrt_hip.Scene(hip_ctx, scene_m)
    static = pbrt_hip.Scene(hip_ctx, make_scene([box_at((0, 1, 0.5))] + others, moving=False))
    rays = rays_at(np.array([[0, 1, 0.5], [-1, 0.5, 0.25], [-2, 0, 0], [2, 0, 0]], dtype=np.float64), 5, [1.0])
    a, b = moving.intersect(rays), static.intersect(rays)
    ap, bp = moving.intersect_p(rays), static.intersect_p(rays)
    moving.close()
    static.close()
    assert (a["instance_id"] == 0).sum() > 500
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(ap, bp)


def test_exact_interpolation_renders_the_static_film(hip_ctx):
    """The same translation with the shutter held at time 1 (lerp(u, 1, 1) is exactly 1 for every u): the film of every integrator
    is the film of the static scene, bit for bit, through the moving builds of the traversal and shading kernels. The moving box is
    glass and a static one a mirror, above a matte floor under a distant light and a dim sky: continuation, MIS, shadow, specular
    recursion (with the unwind to the transmit branch) and AO rays all have to meet the box where time 1 puts it. Two small
    triangles far out give both scenes the same world bound (a moving instance's is its motion bound, as in the reference, and the
    distant light, the sky and the light distribution read the scene's bounding sphere)."""
    far = np.array([[-9, -9, -9], [-9, -8.9, -9], [-8.9, -9, -9], [9, 9, 9], [9, 8.9, 9], [8.9, 9, 9]], dtype=np.float32)
    world = dict(positions=np.concatenate([FLOOR["positions"], far]), indices=np.concatenate([FLOOR["indices"], [[4, 5, 6], [7, 8, 9]]]).astype(np.int32),
                 tri_material=np.zeros(4, np.int32), tri_light=np.full(4, -1, np.int32))
    others = [(0, tr(-2, 0, 0) @ rot((1, 0, 0), 30), None), (1, tr(2, 0, 0), None)]
    lights = SUN + ((scenes.LIGHT_INFINITE, (0.2, 0.25, 0.3), -1, 0, 1),)
    scene_m = make_scene([(1, tr(-1, 0.5, 0.25), tr(1, 1.5, 0.75))] + others, world=world, lights=lights, instance_material=[1, -1, 2])
    scene_m["instance_motion"] = {0: scenes.instance_motion(tr(1, 1.5, 0.75), 0.0, 2.0)}
    moving = pbrt_hip.Scene(hip_ctx, scene_m)
    static = pbrt_hip.Scene(hip_ctx, make_scene([(1, tr(0, 1, 0.5), None)] + others, world=world, lights=lights, moving=False,
                                                instance_material=[1, -1, 2]))
    assert np.array_equal(moving.tlas_nodes[0]["bmin"], static.tlas_nodes[0]["bmin"]) and np.array_equal(moving.tlas_nodes[0]["bmax"], static.tlas_nodes[0]["bmax"])
    cam = scenes.perspective_camera((1.0, -7.0, 4.0), (0, 0, 0), (0, 0, 1), 50.0, 48, 48)
    cam["shutter_open"] = cam["shutter_close"] = 1.0
    at_start = cam.copy()
    at_start["shutter_open"] = at_start["shutter_close"] = 0.0
    for integrator in (pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO):
        kw = dict(integrator=integrator, max_depth=4, ao_samples=4, light_strategy=0 if integrator == pbrt_hip.INTEGRATOR_DIRECT else 1)
        a, _ = moving.render(cam, 48, 48, 4, **kw)
        b, _ = static.render(cam, 48, 48, 4, **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), integrator
        c, _ = moving.render(at_start, 48, 48, 4, **kw)     # ... and the box is somewhere else at time 0
        assert not np.array_equal(a.view(np.uint32), c.view(np.uint32)), integrator
    moving.close()
    static.close()


# ---------------------------------------------------------------------------------------------------------------------
# hits against the model
# ---------------------------------------------------------------------------------------------------------------------
def test_hits_against_the_model(hip_ctx):
    times = some_times(6)
    rays = rays_at(CENTRES, 7, times)
    m = model_hits(FIVE, rays)
    # baseline: per time, static instances at the model's interpolated matrices rounded to float
    base_hits = np.zeros(N_RAYS, dtype=scenes.HIT_DTYPE)
    for t in times:
        frozen = [(k, mo.interpolate(np.float64(t)), None) for (k, _, _), (mo, _, _) in zip(FIVE, model_instances(FIVE))]
        g = pbrt_hip.Scene(hip_ctx, make_scene(frozen, moving=False))
        sel = rays["time"] == t
        base_hits[sel] = g.intersect(rays[sel])
        g.close()
    _, base_rel = check_ids("static instances at the interpolated matrices", base_hits, m)
    g = pbrt_hip.Scene(hip_ctx, make_scene(FIVE))
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    g.close()
    sel, rel = check_ids("moving instances", hits, m)
    for i in range(5):
        assert (m["inst"][sel] == i).sum() > 200, i
    print(f"worst relative error of t: static baseline {base_rel.max():.6e}, moving path {rel.max():.6e} (allowed {4 * base_rel.max():.6e})")
    # ... and over the hits that did go through the interpolation: an animated instance at a time strictly inside (T0, T1)
    inner = (m["inst"][sel] != 4) & (rays["time"][sel] > T0) & (rays["time"][sel] < T1)
    print(f"    of these, {inner.sum()} interpolated hits: static baseline {base_rel[inner].max():.6e}, moving path {rel[inner].max():.6e}")
    assert inner.sum() > 800
    assert rel.max() <= 4 * base_rel.max()
    keep = ~m["unsure"]
    assert np.array_equal(anyhit.astype(bool)[keep], m["hit"][keep])


# ---------------------------------------------------------------------------------------------------------------------
# normals: Lambert's law on a rotating box
# ---------------------------------------------------------------------------------------------------------------------
def test_normals_of_a_rotating_box(hip_ctx):
    spin = [(0, rot((0.2, 0.1, 1.0), 0), rot((0.2, 0.1, 1.0), 120))]   # of the one object (BOX,): the INST = 1 kernels
    wi = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    g = pbrt_hip.Scene(hip_ctx, make_scene(spin, lights=(scenes.distant_light(wi, (LIGHT_L, LIGHT_L, LIGHT_L)),), objects=(BOX,)))
    rays = rays_at(np.zeros((1, 3)), 8, some_times(9), spread=0.35)
    rgb, _ = g.li(rays, np.arange(N_RAYS, dtype=np.uint64) + 1, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    g.close()
    m = model_hits(spin, rays, objects=(BOX,))
    motion, pos, idx = model_instances(spin, objects=(BOX,))[0]
    expect = np.zeros(N_RAYS)
    for t in np.unique(rays["time"]):
        tris = mm.world_triangles(motion, pos, idx, np.float64(t))
        nrm = np.cross(tris[:, 0] - tris[:, 2], tris[:, 1] - tris[:, 2])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        sel = m["hit"] & (rays["time"] == t)
        n = nrm[m["prim"][sel]]
        n = np.where(((n * -rays["d"][sel].astype(np.float64)).sum(axis=1) < 0)[:, None], -n, n)   # towards the viewer
        expect[sel] = np.maximum(0.0, n @ wi)
    keep = ~m["unsure"]
    assert 1.0 - keep.mean() <= 0.02 and (keep & m["hit"]).sum() > 2000
    got = rgb.astype(np.float64) * (np.pi / (KD * LIGHT_L))
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 1], got[:, 2])
    assert (rgb[keep & ~m["hit"]] == 0.0).all()
    worst = np.abs(got[keep, 0] - expect[keep]).max()
    lit = keep & (expect > 0.05)
    print(f"rotating box: {lit.sum()} lit hits over {len(np.unique(rays['time']))} times, worst deviation {worst:.3e} (allowed {NORMAL_TOL:.3e})")
    assert lit.sum() > 800 and len(np.unique(np.round(expect[lit], 3))) > 8   # many different normals: the box does turn
    assert worst <= NORMAL_TOL


# ---------------------------------------------------------------------------------------------------------------------
# shadow rays carry the time
# ---------------------------------------------------------------------------------------------------------------------
def test_shadow_of_a_moving_occluder(hip_ctx):
    """A unit quad at z = 1 slides from x = -1 to x = 1 above the static world-space plane z = 0; the light is straight above. A
    point of the plane is dark exactly while the quad's footprint at the ray's time covers it."""
    plane = dict(FLOOR, positions=FLOOR["positions"] * np.float32([1, 1, 0]))
    slide = [(0, tr(-1, 0, 1), tr(1, 0, 1))]
    g = pbrt_hip.Scene(hip_ctx, make_scene(slide, world=plane, lights=(scenes.distant_light((0, 0, 1.0), (LIGHT_L, LIGHT_L, LIGHT_L)),)))
    rng = np.random.default_rng(10)
    times = some_times(11)
    rays = np.zeros(N_RAYS, dtype=scenes.RAY_DTYPE)
    rays["o"] = np.column_stack([rng.uniform(-2, 2, N_RAYS), rng.uniform(-1, 1, N_RAYS), np.full(N_RAYS, 0.5)])
    rays["d"] = (0.1, 0.05, -1.0)
    rays["t_max"] = np.inf
    rays["time"] = times[rng.integers(0, len(times), N_RAYS)]
    rgb, _ = g.li(rays, np.arange(N_RAYS, dtype=np.uint64) + 1, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    g.close()
    p = rays["o"].astype(np.float64) + 0.5 * rays["d"].astype(np.float64)     # where the ray meets z = 0
    u = np.clip((rays["time"].astype(np.float64) - T0) / (T1 - T0), 0.0, 1.0)
    dx, dy = np.abs(p[:, 0] - (-1.0 + 2.0 * u)), np.abs(p[:, 1])
    inside = (dx < 0.5) & (dy < 0.5)
    edge = (np.abs(dx - 0.5) < 1e-3) & (dy < 0.5 + 1e-3) | (np.abs(dy - 0.5) < 1e-3) & (dx < 0.5 + 1e-3)
    keep = ~edge
    assert 1.0 - keep.mean() <= 0.02
    lit_value = KD / np.pi * LIGHT_L
    assert (inside & keep).sum() > 300 and (~inside & keep).sum() > 1500
    # both sides of the switch at the SAME point of the plane: shadowed at one time, lit at another
    moved = inside & keep & (np.abs(p[:, 0] - (-1.0)) > 0.5)    # would be lit if every ray saw the quad at its start
    assert moved.sum() > 100
    assert (rgb[inside & keep] == 0.0).all()
    assert np.allclose(rgb[~inside & keep].astype(np.float64), lit_value, rtol=1e-5, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# motion blur: the coverage trapezoid
# ---------------------------------------------------------------------------------------------------------------------
def pixel_edges(cam):
    """world x of the RES + 1 column edges and world y of the row edges (orthographic: raster -> camera -> world is affine)"""
    m = cam["camera_to_world"].astype(np.float64).reshape(4, 4) @ cam["raster_to_camera"].astype(np.float64).reshape(4, 4)
    e = np.arange(RES + 1, dtype=np.float64)
    xs = m[0, 0] * e + m[0, 3]
    ys = m[1, 1] * e + m[1, 3]
    assert m[0, 1] == 0 and m[1, 0] == 0
    return xs, ys


def overlap(edges, lo, hi):
    """fraction of every interval between consecutive edges that lies in [lo, hi]"""
    a, b = np.minimum(edges[:-1], edges[1:]), np.maximum(edges[:-1], edges[1:])
    return np.clip(np.minimum(b, hi) - np.maximum(a, lo), 0.0, None) / (b - a)


def test_motion_blur_is_the_coverage_trapezoid(hip_ctx):
    cam = scenes.orthographic_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 2.0, RES, RES)
    g = pbrt_hip.Scene(hip_ctx, blur_scene())
    kw = dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0, seed=3)
    film, _ = g.render(cam, RES, RES, SPP, **kw)
    still = cam.copy()
    still["shutter_close"] = still["shutter_open"]
    film_still, _ = g.render(still, RES, RES, SPP, **kw)
    g.close()
    R = KD / np.pi * LIGHT_L
    xs, ys = pixel_edges(cam)
    x0, y0 = BLUR_START[0], BLUR_START[1]
    # ---- shutter_close == shutter_open: the sharp quad at its start position ----
    rgb = pbrt_hip.film_to_rgb(film_still)[:, :, 1].astype(np.float64)
    cover = overlap(ys, y0 - 0.5, y0 + 0.5)[:, None] * overlap(xs, x0 - 0.5, x0 + 0.5)[None, :]
    assert (cover == 1.0).sum() > 150 and (cover == 0.0).sum() > 3000
    assert np.allclose(rgb[cover == 1.0], R, rtol=1e-4, atol=0.0)
    assert (rgb[cover == 0.0] == 0.0).all()
    # ---- the open shutter: column means against the trapezoid, 5 sigma of RES * SPP independent time draws ----
    rgb = pbrt_hip.film_to_rgb(film)[:, :, 1].astype(np.float64)
    col = rgb.mean(axis=0) / R
    rows = overlap(ys, y0 - 0.5, y0 + 0.5).mean()          # the part of a column's height the quad's y range covers
    sub = (np.arange(2048) + 0.5) / 2048
    expect = np.zeros(RES)
    for c in range(RES):
        x = xs[c] + (xs[c + 1] - xs[c]) * sub
        # fraction of u in [0, 1] with |x - (x0 + shift u)| <= 0.5
        lo, hi = (x - 0.5 - x0) / BLUR_SHIFT, (x + 0.5 - x0) / BLUR_SHIFT
        expect[c] = rows * np.clip(np.minimum(hi, 1.0) - np.maximum(lo, 0.0), 0.0, None).mean()
    sigma = np.sqrt(expect * (1.0 - expect) / (RES * SPP))
    print(f"motion blur: largest column mean {col.max():.4f} (expected {expect.max():.4f}), worst deviation / sigma "
          f"{np.max(np.abs(col - expect)[sigma > 0] / sigma[sigma > 0]):.2f}")
    assert expect.max() > 0.15 and (expect == 0).sum() > 10
    assert (col[expect == 0] == 0.0).all()
    assert np.all(np.abs(col - expect) <= 5 * sigma + 1e-6)   # 1e-6: the midpoint rule above
    # ... and it is not the sharp film
    assert np.abs(col - pbrt_hip.film_to_rgb(film_still)[:, :, 1].mean(axis=0) / R).max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# refusals: each leaves the context usable
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx):
    scene = make_scene(FIVE)
    static_tree = pbrt_hip.build_general_two_level(make_scene(FIVE, moving=False))
    with pytest.raises(pbrt_hip.PbrtHipError, match="motion bound"):
        pbrt_hip.Scene(hip_ctx, scene, bvh=static_tree)
    bad = make_scene(FIVE)
    bad["instance_motion"][2] = scenes.instance_motion(np.diag([1.0, 1.0, 0.0, 1.0]), T0, T1)
    with pytest.raises(pbrt_hip.PbrtHipError, match="moving instance 2: a singular matrix"):
        pbrt_hip.Scene(hip_ctx, bad, bvh=pbrt_hip.build_general_two_level(scene))
    bad["instance_motion"][2] = scenes.instance_motion(FIVE[2][2], T1, T0)
    with pytest.raises(pbrt_hip.PbrtHipError, match="moving instance 2: end_time <= start_time"):
        pbrt_hip.Scene(hip_ctx, bad, bvh=pbrt_hip.build_general_two_level(scene))
    with_map = make_scene(FIVE, lights=(scenes.goniometric_light(np.eye(4), (1.0, 1.0, 1.0)),))
    with pytest.raises(pbrt_hip.PbrtHipError, match="projection or goniometric"):
        pbrt_hip.Scene(hip_ctx, with_map)
    g = pbrt_hip.Scene(hip_ctx, scene)
    assert g.wide_records() == (-1, "scene with moving instances")
    with pytest.raises(pbrt_hip.PbrtHipError, match="moving instances take no lobe rows"):
        g.set_lobe_material(0, scenes.uber())
    rays = rays_at(CENTRES, 12, some_times(13))
    before = g.intersect(rays)
    hip_ctx.set_traversal(pbrt_hip.TRAVERSAL_STACKLESS)
    try:
        with pytest.raises(pbrt_hip.PbrtHipError, match="STACKLESS"):
            g.intersect(rays)
    finally:
        hip_ctx.set_traversal(pbrt_hip.TRAVERSAL_AUTO)
    assert np.array_equal(before.view(np.uint8), g.intersect(rays).view(np.uint8))   # the context and the scene still work
    g.close()
