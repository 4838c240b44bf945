"""The Curve shape on the device (pbrt_hip_scene_create_with_curves): Scene.intersect / intersect_p against the float64 model of
curve_model.py on the shared cases, the tree against the model's loop over all curves, the coverage of an orthographic view, the
closed-form shading of a cylinder-type strip through three integrators, a curve's shadow, old scenes bit for bit through the new
entry point, plastic and Disney rows on a curve, the refusals, and examples/render_fur_patch.cpp against this binding.

Tolerance of t, u and v against the model: four times the spread of the model's own float32 run against its float64 run over the
same cases (curve_cases.case_spread, the largest over the 18 cases), as measured on the CPU by this file at import:
    spread  t 3.04e-06  u 1.70e-06  v 3.11e-04      tolerance  t 1.21e-05  u 6.79e-06  v 1.25e-03
(test_tolerances_are_the_measured_spread prints the figures of the run at hand).

test_gpu_curve_edges.py holds the hit test at the inputs these cases do not reach (each with a margin and a tolerance of its own)
and curves among other primitives; test_gpu_curve_shading.py holds the surface on every case, the orientation flag, and the
integrators and lights beyond point and distant ones."""
import re
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import curve_cases as cc
import curve_model as cm
from test_cpp_example import _build

pytestmark = pytest.mark.gpu

FAR_TRIANGLE = dict(positions=np.array([[50.0, 50.0, 50.0], [50.001, 50.0, 50.0], [50.0, 50.001, 50.0]], dtype=np.float32),
                    indices=np.array([[0, 1, 2]], dtype=np.int32))  # a scene needs a triangle: a speck far from everything
GREY = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
SPREAD_FACTOR = 4.0


def curve_scene(curve_records, materials=None, lights=(), extra=None, shapes=None):
    geo = extra or dict(FAR_TRIANGLE, tri_material=np.zeros(1, dtype=np.int32), tri_light=np.full(1, -1, dtype=np.int32))
    sc = dict(positions=geo["positions"], indices=geo["indices"], tri_material=geo["tri_material"], tri_light=geo["tri_light"],
              materials=materials if materials is not None else scenes._materials([GREY]), lights=scenes._lights(list(lights)),
              curves=scenes.curves(*curve_records) if isinstance(curve_records, (list, tuple)) else curve_records)
    if shapes is not None:
        sc["shapes"] = shapes
    return sc


def as_rays(o, d, t_max=np.inf):
    rays = np.zeros(len(o), dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_max"] = o, d, t_max
    return rays


_tolerance = {}


def tolerance():
    """SPREAD_FACTOR times the model's float32-against-float64 spread, the largest over the cases (computed once, on the CPU)"""
    if not _tolerance:
        spreads = [cc.case_spread(*case) for case in cc.CASES]
        for k in ("t", "u", "v"):
            _tolerance[k] = SPREAD_FACTOR * max(s[k] for s in spreads)
            _tolerance["spread_" + k] = max(s[k] for s in spreads)
    return _tolerance


def test_tolerances_are_the_measured_spread():
    tol = tolerance()
    print("float32 / float64 spread of the model: t %.2e u %.2e v %.2e; tolerance t %.2e u %.2e v %.2e" % (
        tol["spread_t"], tol["spread_u"], tol["spread_v"], tol["t"], tol["u"], tol["v"]))
    assert 0 < tol["t"] < 1e-3 and 0 < tol["u"] < 1e-3 and 0 < tol["v"] < 1e-1


# ---------------------------------------------------------------------------------------------------------------------
# 1. hits against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: "-".join(c))
def test_hits_against_the_model(hip_ctx, case):
    curves, (o, d, t_max), m64, _ = cc.case_model(*case)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves))
    assert g.wide_records() == (-1, "scene with curves")
    rays = as_rays(o, d, t_max)
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    g.close()
    keep = m64["margin"] >= cc.MARGIN
    assert 1.0 - keep.mean() <= cc.MAX_LEFT_OUT
    dev_hit = hits["prim_id"] >= 1          # curve j is primitive n_tris + j
    assert ((hits["prim_id"] >= -1) & (hits["prim_id"] <= len(curves))).all()
    both = keep & dev_hit & m64["hit"]
    tol = tolerance()
    err = {k: np.abs(hits[f][both].astype(np.float64) - m64[k][both]) for k, f in (("t", "t"), ("u", "b0"), ("v", "b1"))}
    print("-".join(case), "hits %.3f left out %.4f worst t %.2e u %.2e v %.2e (allowed %.2e %.2e %.2e)" % (
        m64["hit"].mean(), 1.0 - keep.mean(), err["t"].max(), err["u"].max(), err["v"].max(), tol["t"], tol["u"], tol["v"]))
    assert np.array_equal(dev_hit[keep], m64["hit"][keep]), np.flatnonzero(keep & (dev_hit != m64["hit"]))[:5]
    assert both.sum() > 400
    assert np.array_equal(hits["prim_id"][both] - 1, m64["prim"][both])
    assert (hits["b2"][dev_hit] == 0).all()
    for k in ("t", "u", "v"):
        assert err[k].max() <= tol[k], (k, err[k].max(), tol[k])
    # Curve::intersect_p stops at the first leaf that hits: the same verdict on every ray
    assert np.array_equal(anyhit.astype(bool), dev_hit)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the tree against brute force
# ---------------------------------------------------------------------------------------------------------------------
def test_tree_of_overlapping_curves_against_the_loop_over_all(hip_ctx):
    rng = np.random.default_rng(77)
    recs = []
    for j in range(64):
        p0 = rng.uniform(-0.5, 0.5, 3)
        cp = p0 + np.cumsum(np.vstack([np.zeros(3), rng.uniform(-0.4, 0.4, (3, 3))]), axis=0)
        kind = ("flat", "cylinder", "ribbon")[j % 3]
        recs.append(scenes.curve(cp, rng.uniform(0.03, 0.08), rng.uniform(0.01, 0.05), type=kind,
                                 normals=rng.normal(size=(2, 3)) if kind == "ribbon" else None, split_depth=0))
    curves = scenes.curves(*recs)
    n = 8192
    target = rng.uniform(-0.6, 0.6, (n, 3))
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    o = (target + 2.5 * away).astype(np.float32)
    d = (-away * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    m = cm.intersect_many(curves, o, d)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves), max_prims_in_node=4)
    hits = g.intersect(as_rays(o, d))
    assert len(g.nodes) > 16
    g.close()
    # a ray is left out where any curve's decision is close, or where two curves' hits lie closer than the tolerance of t
    keep = m["margin"] >= cc.MARGIN
    dev_hit = hits["prim_id"] >= 1
    assert keep.mean() > 0.9 and m["hit"].mean() > 0.3
    assert np.array_equal(dev_hit[keep], m["hit"][keep])
    both = keep & dev_hit
    second = np.full(n, np.inf)
    for j, rec in enumerate(curves):
        r = cm.intersect(rec, o, d)
        other = r["hit"] & (m["prim"] != j)
        second = np.where(other, np.minimum(second, r["t"]), second)
    clear = both & (second > m["t"] + 10 * tolerance()["t"])
    assert clear.sum() > 0.9 * both.sum()
    assert np.array_equal(hits["prim_id"][clear] - 1, m["prim"][clear])
    assert np.abs(hits["t"][clear] - m["t"][clear]).max() <= tolerance()["t"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. coverage and the closed-form shading of a strip that spans the film
# ---------------------------------------------------------------------------------------------------------------------
STRIP_W, KD, SUN = 0.5, 0.6, 2.0
STRIP_CP = np.array([(-3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (3.0, 0.0, 0.0)])


def strip_view(hip_ctx, kind):
    """an orthographic camera on +z looking down at a straight curve along x that spans the 2 x 2 film window; the sun behind
    the camera. Returns (scene, camera rays, their stream keys, device hits)."""
    mats = scenes._materials([(scenes.MAT_MATTE, (KD, KD, KD), (0, 0, 0), 1.0)])
    sc = curve_scene([scenes.curve(STRIP_CP, STRIP_W, STRIP_W, type=kind, split_depth=1)], materials=mats,
                     lights=[scenes.distant_light((0.0, 0.0, 1.0), (SUN, SUN, SUN))])
    g = pbrt_hip.Scene(hip_ctx, sc)
    cam = scenes.orthographic_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 32, 32)
    rays, keys, _, _ = g.camera_rays(cam, 32, 32, 16, seed=4)
    return g, rays, keys, g.intersect(rays)


def test_coverage_of_a_flat_strip(hip_ctx):
    g, rays, _, hits = strip_view(hip_ctx, "flat")
    g.close()
    n = len(rays)
    frac, want = (hits["prim_id"] >= 1).mean(), STRIP_W / 2.0
    sigma = np.sqrt(want * (1 - want) / n)
    print(f"coverage {frac:.5f} against {want:.5f}, sigma {sigma:.5f}, n {n}")
    assert n == 32 * 32 * 16 and abs(frac - want) <= 5 * sigma
    h = hits["prim_id"] >= 1
    np.testing.assert_allclose(hits["t"][h], 5.0, atol=1e-4)
    np.testing.assert_allclose(np.abs(hits["b1"][h] - 0.5), np.abs(rays["o"][h, 1]) / STRIP_W, atol=1e-4)


@pytest.mark.parametrize("integrator", ["path", "direct", "whitted"])
def test_cylinder_strip_radiance_closed_form(hip_ctx, integrator):
    """theta = lerp(v, -90, 90) degrees is linear in v and v is uniform over the strip under an orthographic view, so the mean of
    |cos theta| over the strip is 2 / pi and the mean radiance Kd / pi * E * 2 / pi with E the sun's normal irradiance. Every lit
    sample also shows that the shadow ray leaving the curve (offset by p_error = 2 hit_width) does not hit the curve itself: a
    self-shadowed sample would be black."""
    g, rays, keys, hits = strip_view(hip_ctx, "cylinder")
    which = dict(path=pbrt_hip.INTEGRATOR_PATH, direct=pbrt_hip.INTEGRATOR_DIRECT, whitted=pbrt_hip.INTEGRATOR_WHITTED)[integrator]
    rgb, _ = g.li(rays, keys, integrator=which, max_depth=1)
    g.close()
    h = hits["prim_id"] >= 1
    assert h.sum() > 3000 and np.isfinite(rgb).all() and (rgb[~h] == 0).all()
    per_ray = rgb[h, 0].astype(np.float64)
    want_each = KD / np.pi * SUN * np.abs(np.cos(np.radians(-90.0 + 180.0 * hits["b1"][h].astype(np.float64))))
    np.testing.assert_allclose(per_ray, want_each, rtol=2e-3, atol=2e-4)  # the same law ray by ray, v from the hit record
    want = KD / np.pi * SUN * 2.0 / np.pi
    sigma = KD / np.pi * SUN * np.sqrt(0.5 - 4.0 / np.pi ** 2) / np.sqrt(h.sum())
    print(f"{integrator}: mean {per_ray.mean():.5f} against {want:.5f}, sigma {sigma:.5f}")
    assert abs(per_ray.mean() - want) <= 5 * sigma


# ---------------------------------------------------------------------------------------------------------------------
# 5. shadows
# ---------------------------------------------------------------------------------------------------------------------
def test_a_curves_shadow_on_a_plane_follows_the_model(hip_ctx):
    """the plane z = 0 under a point light, a bent flat curve between them: a plane point is lit iff the model's intersect_p
    lets the shadow ray (from the point, offset along the normal as spawn_ray does it, to the light) through"""
    half = 4.0
    plane = dict(positions=np.array([(-half, -half, 0), (half, -half, 0), (half, half, 0), (-half, half, 0)], dtype=np.float32),
                 indices=np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    cp = np.array([(-0.8, 0.1, 0.6), (-0.2, 0.5, 0.8), (0.3, -0.4, 0.5), (0.9, 0.0, 0.7)])
    curves = scenes.curve(cp, 0.12, 0.06, type="flat", split_depth=1)
    p_light = np.array([0.2, 1.5, 2.5])
    sc = curve_scene(curves, extra=plane, lights=[scenes.point_light(tuple(p_light), (10.0, 10.0, 10.0))])
    g = pbrt_hip.Scene(hip_ctx, sc)
    rng = np.random.default_rng(5)
    n = 6000
    # points in the shadow's neighbourhood: the curve's points projected from the light onto the plane, jittered
    u = rng.uniform(0, 1, n)[:, None]
    on_curve = (1 - u) ** 3 * cp[0] + 3 * u * (1 - u) ** 2 * cp[1] + 3 * u * u * (1 - u) * cp[2] + u ** 3 * cp[3]
    s = p_light[2] / (p_light[2] - on_curve[:, 2:3])
    ground = p_light + (on_curve - p_light) * s + np.concatenate([rng.uniform(-0.25, 0.25, (n, 2)), np.zeros((n, 1))], axis=1)
    ground[:, 2] = 0.0
    o = (ground + np.array([0.0, -3.0, 4.0])).astype(np.float32)  # looked at from the side the shadow falls to
    d = (ground - o).astype(np.float32)
    rays = as_rays(o, d)
    first = g.intersect(rays)
    rgb, _ = g.li(rays, np.arange(n, dtype=np.uint64), integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1)
    g.close()
    on_plane = (first["prim_id"] >= 0) & (first["prim_id"] < 2)
    assert on_plane.mean() > 0.8
    p = o.astype(np.float64) + d.astype(np.float64) * first["t"][:, None].astype(np.float64)
    to_light = p_light - p
    m = cm.intersect_many(curves, p + np.array([0.0, 0.0, 1e-4]), to_light, 1.0 - 1e-4)
    keep = on_plane & (m["margin"] >= 0.02)   # the plane point itself carries the primary ray's rounding: a wider band than MARGIN
    lit = rgb[:, 0] > 0
    print(f"shadow: on the plane {on_plane.mean():.3f}, kept {keep.mean():.3f}, in shadow {m['hit'][keep].mean():.3f}")
    assert keep.mean() > 0.7 and 0.1 < m["hit"][keep].mean() < 0.9
    assert np.array_equal(lit[keep], ~m["hit"][keep])


@pytest.mark.parametrize("kind", ["flat", "cylinder"])
def test_a_shadow_ray_leaving_a_bent_curve_does_not_hit_it_where_it_starts(hip_ctx, kind):
    """a bent curve alone under an oblique sun: a hit reflects Kd / pi * E * |wi . n| when wi and wo lie on one side of n and
    nothing when they do not, unless ANOTHER part of the curve stands in the way, which the model decides from the origin
    spawn_ray gives the shadow ray (p moved along n by |n| . p_error, p_error = 2 hit_width through the transform). A curve that
    caught its own shadow ray at the start would be black where the model says lit."""
    curves, (o, d, t_max), m64, _ = cc.case_model(kind, "bent", "rigid")
    sun_dir = np.array([0.5, 0.3, 0.8]) / np.linalg.norm([0.5, 0.3, 0.8])
    mats = scenes._materials([(scenes.MAT_MATTE, (KD, KD, KD), (0, 0, 0), 1.0)])
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=mats, lights=[scenes.distant_light(tuple(sun_dir), (SUN, SUN, SUN))]))
    rays = as_rays(o, d, t_max)
    rgb, _ = g.li(rays, np.arange(len(o), dtype=np.uint64), integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1)
    g.close()
    n, p, width = np.zeros((len(o), 3)), np.zeros((len(o), 3)), np.zeros(len(o))
    for j, rec in enumerate(curves):
        r = cm.intersect(rec, o, d, t_max)
        mine = m64["hit"] & (m64["prim"] == j)
        n[mine], p[mine], width[mine] = r["n"][mine], r["p"][mine], r["width"][mine]
    h = m64["hit"] & (m64["margin"] >= 0.05)
    wo = -d.astype(np.float64) / np.linalg.norm(d, axis=1, keepdims=True)
    cos_i, cos_o = n @ sun_dir, (n * wo).sum(-1)
    lin = np.abs(cc.transform("rigid")[:3, :3])
    p_err = 2 * width[:, None] * lin.sum(1)[None, :]
    start = p + n * np.sign(cos_i)[:, None] * (np.abs(n) * p_err).sum(-1, keepdims=True)
    blocked = cm.intersect_many(curves, start[h], np.broadcast_to(sun_dir, (h.sum(), 3)))
    sure = blocked["margin"] >= 0.05
    want = np.where((cos_i[h] * cos_o[h] > 0) & ~blocked["hit"], KD / np.pi * SUN * np.abs(cos_i[h]), 0.0)
    lit = want > 0
    print(f"{kind}: {h.sum()} hits, {sure.mean():.3f} of them clear of a decision, lit {lit[sure].mean():.3f}, blocked by the curve {blocked['hit'][sure].mean():.3f}")
    assert sure.mean() > 0.8 and lit[sure].mean() > 0.2
    np.testing.assert_allclose(rgb[h, 0][sure], want[sure], rtol=5e-3, atol=2e-4)


def test_the_binding_refuses_curves_where_no_entry_point_takes_them(hip_ctx):
    rec = scenes.curve(cc.STRAIGHT, 0.1, 0.1, split_depth=0)
    base = curve_scene(rec)
    for extra in (dict(instances=np.zeros(1, scenes.INSTANCE_DTYPE)), dict(objects=[])):
        with pytest.raises(pbrt_hip.PbrtHipError, match="one-level scenes"):
            pbrt_hip.Scene(hip_ctx, dict(base, **extra))
    with pytest.raises(pbrt_hip.PbrtHipError, match="one-level scenes"):
        pbrt_hip.Scene(hip_ctx, base, device_build=True)
    # an empty array and no shapes: the scene it was without the key
    plain = dict(base, curves=scenes.curves())
    a, b = pbrt_hip.Scene(hip_ctx, plain), pbrt_hip.Scene(hip_ctx, {k: v for k, v in plain.items() if k != "curves"})
    assert a.wide_records() == b.wide_records() and a.wide_records()[0] >= 0
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. old scenes unchanged
# ---------------------------------------------------------------------------------------------------------------------
def test_a_scene_without_curves_through_the_new_entry_is_bit_for_bit_the_old_one(hip_ctx):
    base = scenes.mixed_materials_scene(n_tris=64)
    shapes = scenes.shapes(scenes.sphere_shape(0.3, to_world=np.array([[1, 0, 0, 0.2], [0, 1, 0, 0.1], [0, 0, 1, -0.1], [0, 0, 0, 1.0]]), material=1),
                           scenes.cylinder(0.15, -0.4, 0.4, material=2), scenes.disk(0.3, 0.4, material=0))
    old = dict(base, shapes=shapes)
    new = dict(old, curves=scenes.curves())
    ga, gb = pbrt_hip.Scene(hip_ctx, old), pbrt_hip.Scene(hip_ctx, new)
    assert ga.nodes.tobytes() == gb.nodes.tobytes() and gb.wide_records() == (-1, "scene with shapes")
    rays = scenes.random_rays(8192, 11, origin_extent=1.5)
    assert ga.intersect(rays).tobytes() == gb.intersect(rays).tobytes()
    assert np.array_equal(ga.intersect_p(rays), gb.intersect_p(rays))
    cam = scenes.perspective_camera((0.0, 0.3, 3.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 32, 32)
    for integrator in (pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO):
        fa, _ = ga.render(cam, 32, 32, 8, integrator=integrator, max_depth=4, seed=3, ao_samples=4)
        fb, _ = gb.render(cam, 32, 32, 8, integrator=integrator, max_depth=4, seed=3, ao_samples=4)
        assert fa[..., :3].mean() > 0.001 and fa.tobytes() == fb.tobytes(), integrator
    ga.close()
    gb.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. materials on a curve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", ["plastic", "disney"])
def test_glossy_rows_on_a_curve_follow_bsdf_query(hip_ctx, material):
    """one ray onto a flat curve under a point light: L = f(wo, wi) I |cos theta_i| / r^2 with f from bsdf_query in the shading
    frame the model's n and dpdu span (make_frame: ss = normalize(dpdu), ts = ns x ss)"""
    mats = scenes._materials([scenes.plastic((0.4, 0.3, 0.2), (0.5, 0.5, 0.5), 0.2) if material == "plastic" else GREY])
    rec = scenes.curve(cc.BENT, 0.3, 0.2, type="flat", to_world=cc.transform("rigid"), split_depth=0)
    p_light, intensity = np.array([0.5, 0.4, 3.0]), np.array([6.0, 5.0, 4.0])
    g = pbrt_hip.Scene(hip_ctx, curve_scene(rec, materials=mats, lights=[scenes.point_light(tuple(p_light), tuple(intensity))]))
    if material == "disney":
        g.set_disney_material(0, scenes.disney((0.5, 0.4, 0.3), metallic=0.3, roughness=0.4, sheen=0.5, clearcoat=0.5))
    m = cc.transform("rigid")
    u = 0.31  # a point of the curve away from the junctions of its leaves, and the ray a little off its axis
    mid = ((1 - u) ** 3 * cc.BENT[0] + 3 * u * (1 - u) ** 2 * cc.BENT[1] + 3 * u * u * (1 - u) * cc.BENT[2] + u ** 3 * cc.BENT[3]
           + np.array([0.02, 0.03, 0.0])) @ m[:3, :3].T + m[:3, 3]
    o = (mid + np.array([0.3, -0.2, 2.0])).astype(np.float32)[None, :]
    d = (mid - o[0]).astype(np.float32)[None, :]
    r = cm.intersect(rec[0], o, d)
    assert r["hit"][0] and r["margin"][0] > 0.05
    rgb, _ = g.li(as_rays(o, d), np.zeros(1, np.uint64), integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1)
    film, _ = g.render(scenes.perspective_camera(tuple(o[0]), tuple(mid), (0.0, 1.0, 0.0), 30.0, 16, 16), 16, 16, 4, max_depth=3, seed=1)
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    n, ss = r["n"][0], r["dpdu"][0] / np.linalg.norm(r["dpdu"][0])
    ts = np.cross(n, ss)
    to_local = lambda w: np.array([w @ ss, w @ ts, w @ n])
    wo = -d[0].astype(np.float64) / np.linalg.norm(d[0])
    wi = p_light - r["p"][0]
    dist2 = wi @ wi
    wi = wi / np.sqrt(dist2)
    q = g.bsdf_query(0, to_local(wo)[None, :], to_local(wi)[None, :], np.zeros((1, 2)))
    g.close()
    want = q["f"][0].astype(np.float64) * intensity * abs(wi @ n) / dist2
    print(material, "L", rgb[0], "want", want)
    assert (want > 0).all()
    np.testing.assert_allclose(rgb[0], want, rtol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _bad(field, value, kind="flat"):
    rec = scenes.curve(cc.BENT, 0.05, 0.02, type=kind, normals=[(0, 0, 1), (0, 1, 0)] if kind == "ribbon" else None, split_depth=0)
    rec[field] = value
    return rec


REFUSALS = [
    ("unknown type", lambda: _bad("type", 3), "unknown curve type"),
    ("negative type", lambda: _bad("type", -1), "unknown curve type"),
    ("nan control point", lambda: _bad("cp", np.full((4, 3), np.nan)), "control points must be finite"),
    ("infinite control point", lambda: _bad("cp", np.full((4, 3), np.inf)), "control points must be finite"),
    ("negative width", lambda: _bad("width1", -0.01), "widths must be finite and not negative"),
    ("both widths zero", lambda: scenes.curve(cc.BENT, 0.0, 0.0, split_depth=0), "must not both be zero"),
    ("u_min == u_max", lambda: _bad("u_max", 0.0), "u range"),
    ("u_max > 1", lambda: _bad("u_max", 1.5), "u range"),
    ("u_min < 0", lambda: _bad("u_min", -0.5), "u range"),
    ("zero ribbon normal", lambda: _bad("n0", (0, 0, 0), "ribbon"), "normals must not be zero"),
    ("opposite ribbon normals", lambda: _bad("n1", (0, 0, -2), "ribbon"), "n0 == -n1"),
    ("material out of range", lambda: _bad("material", 7), "curve material out of range"),
]


@pytest.mark.parametrize("name,make,why", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_context_usable(hip_ctx, name, make, why):
    with pytest.raises(pbrt_hip.PbrtHipError, match=re.escape(why)):
        pbrt_hip.Scene(hip_ctx, curve_scene(make()))
    good = scenes.curve(cc.STRAIGHT, 0.1, 0.1, split_depth=0)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(good))
    assert g.intersect(as_rays(np.array([[0.6, 0.0, 2.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32)))["prim_id"][0] == 1
    g.close()


def test_a_light_on_a_curve_and_what_shape_scenes_refuse(hip_ctx):
    good = scenes.curve(cc.STRAIGHT, 0.1, 0.1, split_depth=0)
    with pytest.raises(pbrt_hip.PbrtHipError, match="a curve cannot carry an area light"):
        pbrt_hip.Scene(hip_ctx, curve_scene(good, lights=[(scenes.LIGHT_DIFFUSE_AREA, (1.0, 1.0, 1.0), 1, 0, 1)]))
    with pytest.raises(pbrt_hip.PbrtHipError, match="shape radius must be positive"):  # whatever _with_shapes refuses
        bad_shape = scenes.sphere_shape(0.3)
        bad_shape["radius"] = -0.3
        pbrt_hip.Scene(hip_ctx, curve_scene(good, shapes=bad_shape))
    g = pbrt_hip.Scene(hip_ctx, curve_scene(good, shapes=scenes.shapes(scenes.sphere_shape(0.2, to_world=np.array(
        [[1, 0, 0, 0.0], [0, 1, 0, 1.0], [0, 0, 1, 0.0], [0, 0, 0, 1.0]])))))
    # primitives: the speck 0, the sphere 1, the curve 2
    hits = g.intersect(as_rays(np.array([[0.6, 0.0, 2.0], [0.0, 1.0, 2.0]], np.float32), np.array([[0.0, 0.0, -1.0]] * 2, np.float32)))
    assert list(hits["prim_id"]) == [2, 1]
    assert g.intersect_p(as_rays(np.array([[0.6, 0.0, 2.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32)))[0] == 1
    g.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the C++ example
# ---------------------------------------------------------------------------------------------------------------------
def _fur_patch():
    """the scene of examples/render_fur_patch.cpp, array for array (the same 31-bit generator, in float32)"""
    state = [12345]

    def unit():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7FFFFFFF
        return np.float32(state[0] >> 7) / np.float32(16777216.0)

    f = np.float32
    side, recs = 16, []
    for i in range(side):
        for j in range(side):
            x = f(-0.9) + f(1.8) * (f(i) + unit()) / f(side)
            z = f(-0.9) + f(1.8) * (f(j) + unit()) / f(side)
            bx = f(0.3) * (unit() - f(0.5))
            bz = f(0.3) * (unit() - f(0.5))
            h = f(0.4) + f(0.3) * unit()
            cp = np.array([(x, f(0), z), (x + f(0.2) * bx, f(0.4) * h, z + f(0.2) * bz), (x + bx, f(0.8) * h, z + bz),
                           (x + f(2.0) * bx, h, z + f(2.0) * bz)], dtype=np.float32)
            recs.append(scenes.curve(cp, 0.03, 0.005, type="cylinder", material=1, split_depth=1))
    quad = dict(positions=np.array([(-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1)], dtype=np.float32),
                indices=np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    mats = scenes._materials([(scenes.MAT_MATTE, (0.6, 0.5, 0.4), (0, 0, 0), 1.0), (scenes.MAT_MATTE, (0.35, 0.2, 0.1), (0, 0, 0), 1.0)])
    sun = scenes.distant_light((0.3, 1.0, -0.2), (3.0, 3.0, 3.0))
    ln = np.sqrt(f(0.3) * f(0.3) + f(1.0) + f(0.2) * f(0.2))
    sun["pos"] = (f(0.3) / ln, f(1.0) / ln, f(-0.2) / ln)
    return curve_scene(scenes.curves(*recs), materials=mats, lights=[sun], extra=quad)


def test_cpp_fur_patch_renders_what_the_python_binding_renders(tmp_path, hip_ctx):
    W = H = 32
    raw = tmp_path / "film.raw"
    r = subprocess.run([_build(tmp_path, "render_fur_patch.cpp"), str(raw), str(W), str(H)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"fur patch: 512 curve segments, (\d+) camera samples, (\d+) closest-hit \+ (\d+) shadow rays", r.stdout)
    assert m and int(m.group(1)) == W * H * 16, r.stdout
    g = pbrt_hip.Scene(hip_ctx, _fur_patch())
    film, st = g.render(scenes.perspective_camera((0.0, 1.6, -2.6), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 40.0, W, H), W, H, 16, max_depth=3, seed=7,
                        light_strategy=2)  # PathIntegrator::new's default: "spatial"
    g.close()
    assert (st["camera_samples"], st["rays_closest"], st["rays_shadow"]) == tuple(int(m.group(k)) for k in (1, 2, 3))
    assert film[..., :3].mean() > 0.01
    assert raw.read_bytes() == film.tobytes()
