"""The surface make_surface_curve builds and the integrators and lights a curve had not met, on the device against the float64
model (curve_model.py, curve_cases.py, bxdf_model.py, microfacet_model.py):

  a. the Lambert probe of test_gpu_curves.py's shadow test on all 18 shared cases and on the thin, hair, taper and placed edge
     cases: a ribbon's normal, every normal under scale, a mirror and reverse_orientation, p_error through the case's transform,
     and the traversal's hit (with the rays' finite t_max) against make_surface_curve's second run of the hit test without one,
     whose fallback surface (n = wo) this law tells apart;
  b. kCurveFlipNormal: a rough-glass row, which is not symmetric under n -> -n, under a point light before and behind the curve,
     for {rigid, mirrored} x {reverse_orientation 0, 1} and scaled, f from bxdf_model.py in the model's frame; and dpdu through
     vec(w, dpdu) under scale with an anisotropic metal row. test_curve_model.py shows on the CPU that a reversed normal (a frame
     turned by 90 degrees) moves the expected value by more than ten times the tolerance on 0.58-1.0 (0.75-0.99) of the rays;
  c. k_shade_direct<AO, kDirectCurves>, a constant environment through both integrators and every light strategy, a mesh emitter
     against Lambert's polygon formula, and specular glass.

Measured on the CPU (the model alone): the probe keeps 786-1534 hits of a shared case with 0.999 or more of them clear of a
decision and 0.47-0.52 lit, and 299-835 of an edge case; the orientation cases keep 162-231 of 256 rays, all with an open way to
the light, 0.44-1.0 of them with f > 0. The environment's 5 sigma is 0.0185-0.0197 of Kd Le at 4096 hits, the emitter's 0.010
(direct) and 0.017 (path) of the mean at 3379 kept hits.

Where this departs from the issue, because the model or the algorithm does not bear it out:
  - the probe leaves out hair-cylinder and placed_far-cylinder, and on the other edge cases the rays the model's own float32 run
    does not decide (UNDECIDED, lambert_probe);
  - the strip faces a plane 2 below it, not 0.5, and only the flat type's value is 0 there
    (test_ambient_occlusion_under_a_strip_that_faces_a_plane);
  - a sample through specular glass on a strip is Le when it reflects and Le (eta_i / eta_t)^2 when it refracts
    (test_specular_glass_on_a_strip)."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import bxdf_model as bm
import curve_cases as cc
from curve_cases import GLASS, GLOSSY_RTOL, METAL
import curve_model as cm
import microfacet_model as mm
from test_gpu_curves import KD, STRIP_CP, STRIP_W, SUN, as_rays, curve_scene

pytestmark = pytest.mark.gpu

PATH, DIRECT, AO = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_AO
MATTE = scenes._materials([(scenes.MAT_MATTE, (KD, KD, KD), (0, 0, 0), 1.0)])
SUN_DIR = np.array([0.5, 0.3, 0.8]) / np.linalg.norm([0.5, 0.3, 0.8])


# ---------------------------------------------------------------------------------------------------------------------
# a. the Lambert probe
# ---------------------------------------------------------------------------------------------------------------------
def lambert_probe(hip_ctx, label, curves, o, d, t_max, m64, m32=None):
    """a curve alone under an oblique sun: a hit reflects Kd / pi * E * |wi . n| when wi and wo lie on one side of the model's n
    and nothing is in the way (which the model decides from where spawn_ray starts the shadow ray), otherwise nothing. The
    margins (0.05 of hit_width on the hit and on the shadow ray) and the tolerances are those of
    test_gpu_curves.py::test_a_shadow_ray_leaving_a_bent_curve_does_not_hit_it_where_it_starts.
    m32 (the edge cases): the model's float32 run. A ray is then kept only where that run's own normal gives the float64 value
    within a quarter of the allowance (the device is allowed SPREAD_FACTOR = 4 times the model's own spread, as for t, u and v),
    and of the hits at least 0.8 must remain."""
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=MATTE, lights=[scenes.distant_light(tuple(SUN_DIR), (SUN, SUN, SUN))]))
    rgb, _ = g.li(as_rays(o, d, t_max), np.arange(len(o), dtype=np.uint64), integrator=DIRECT, max_depth=1)
    g.close()
    assert np.isfinite(rgb).all()
    surf = cc.surface_of(curves, o, d, t_max, m64)
    h = m64["hit"] & (m64["margin"] >= 0.05)
    wo = -d.astype(np.float64) / np.linalg.norm(d, axis=1, keepdims=True)
    cos_i, cos_o = surf["n"][h] @ SUN_DIR, (surf["n"][h] * wo[h]).sum(-1)
    blocked = cc.leaving(curves, surf, h, np.broadcast_to(SUN_DIR, (h.sum(), 3)))
    sure = blocked["margin"] >= 0.05
    want = np.where((cos_i * cos_o > 0) & ~blocked["hit"], KD / np.pi * SUN * np.abs(cos_i), 0.0)
    allowance = 2e-4 + 5e-3 * np.abs(want)
    if m32 is not None:
        n32 = np.zeros((len(o), 3))
        for j, rec in enumerate(curves):
            mine = h & m32["hit"] & (m32["prim"] == j) & (m64["prim"] == j)
            if mine.any():
                n32[mine] = cm.intersect(rec, o[mine], d[mine], t_max[mine], np.float32)["n"]
        own = np.abs(KD / np.pi * SUN * np.abs(n32[h] @ SUN_DIR) - KD / np.pi * SUN * np.abs(cos_i))
        print(f"{label}: the float32 model's own error over the allowance: worst {(own / allowance).max():.2f}, "
              f"over a quarter of it on {(own > allowance / 4).mean():.4f} of the hits")
        sure &= own <= allowance / 4
    lit = want > 0
    got = rgb[h, 0].astype(np.float64)
    worst = np.abs(got[sure] - want[sure]) / allowance[sure]
    print(f"{label}: {h.sum()} hits, {sure.mean():.3f} of them clear of a decision, lit {lit[sure].mean():.3f}, blocked by the curve "
          f"{blocked['hit'][sure].mean():.3f}, worst error over allowance {worst.max():.3f}")
    assert sure.mean() > 0.8 and lit[sure].mean() > 0.2
    np.testing.assert_allclose(got[sure], want[sure], rtol=5e-3, atol=2e-4)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: "-".join(c))
def test_lambert_probe_on_the_shared_cases(hip_ctx, case):
    curves, (o, d, t_max), m64, _ = cc.case_model(*case)
    lambert_probe(hip_ctx, "-".join(case), curves, o, d, t_max, m64)


# A cylinder-type curve's normal reads v. Where v itself is not decided in float32 (its spread is 0.017-0.15 of the strip on the
# hair and 0.007-0.04 moved far from the origin; the clamp's is not compared either), the model's own float32 run misses this
# probe's allowance on 0.23 and 0.21 of the hits, by up to 17 times: those two cases cannot be held to it.
UNDECIDED = {("hair", "cylinder"), ("placed_far", "cylinder")}
PROBED_EDGES = [c for c in cc.EDGE_CASES if c[0] in ("thin", "hair", "taper", "placed_far", "placed_small", "placed_large") and c not in UNDECIDED]


@pytest.mark.parametrize("case", PROBED_EDGES, ids=lambda c: "-".join(c))
def test_lambert_probe_on_edge_cases(hip_ctx, case):
    curves, (o, d, t_max), m64, m32, _ = cc.edge_model(*case)
    lambert_probe(hip_ctx, "-".join(case), curves, o, d, t_max, m64, m32)


# ---------------------------------------------------------------------------------------------------------------------
# b. the orientation flag and dpdu
# ---------------------------------------------------------------------------------------------------------------------
def point_light_check(hip_ctx, label, kind, xform, reverse, set_row, f_of, lights, materials=None):
    curves, (o, d), _, surf, where = cc.orient_case(kind, xform, reverse)
    for light in lights:
        keep, clear = cc.orient_kept(kind, xform, reverse, light)
        g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=materials, lights=[scenes.point_light(tuple(where[light]), cc.ORIENT_INTENSITY)]))
        set_row(g)
        rgb, _ = g.li(as_rays(o, d), np.arange(len(o), dtype=np.uint64), integrator=DIRECT, max_depth=1)
        g.close()
        want = cc.point_light_radiance(surf, keep, d, where[light], cc.ORIENT_INTENSITY, f_of) * clear[:, None]
        got = rgb[keep].astype(np.float64)
        scale = np.abs(want).max()
        worst = np.abs(got - want) / (GLOSSY_RTOL * np.abs(want) + 1e-6 * scale)
        print(f"{label} light {light}: kept {len(keep)}, nonzero {(want > 0).all(-1).mean():.3f}, largest {scale:.3g}, "
              f"worst error over allowance {worst.max():.3f}")
        assert len(keep) >= 128 and (want > 0).all(-1).mean() > 0.3 and np.isfinite(rgb).all()
        # rtol as test_gpu_curves.py's glossy rows; atol, a millionth of the largest value, for the rays whose f is 0
        np.testing.assert_allclose(got, want, rtol=GLOSSY_RTOL, atol=1e-6 * scale)


@pytest.mark.parametrize("xform,reverse", cc.ORIENTATIONS, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", cc.TYPES)
def test_rough_glass_tells_the_side_of_the_normal(hip_ctx, kind, xform, reverse):
    """L = f(wo, wi) I |wi . n| / r^2 with f of rough glass (Kr = Kt = 1, eta 1.5, roughness 0.3) in the frame ss =
    normalize(dpdu), ts = n x ss with the model's n: reflection past the critical angle and transmission both depend on which
    side n calls outside, so kCurveFlipNormal inverted fails this on most rays (test_curve_model.py measures how many)."""
    model = bm.rough_glass(GLASS["kr"], GLASS["kt"], GLASS["eta"], GLASS["roughness"])
    desc = scenes.rough_glass(GLASS["kr"], GLASS["kt"], GLASS["eta"], GLASS["roughness"])
    point_light_check(hip_ctx, f"{kind} {xform} reverse {int(reverse)}", kind, xform, reverse, lambda g: g.set_material(0, desc),
                      lambda wo, wi: bm.bsdf_f(model, wo, wi), ("front", "behind"))


@pytest.mark.parametrize("kind", cc.TYPES)
def test_anisotropic_metal_holds_dpdu_under_scale(hip_ctx, kind):
    """a metal row with alphas from roughness 0.05 along dpdu and 0.4 across it, under the scaled transform and the front light:
    vec(w, dpdu) wrong by a quarter turn moves the value on 0.75-0.99 of the rays (test_curve_model.py)"""
    model = mm.Material.metal(METAL["eta"], METAL["k"], METAL["u_roughness"], METAL["v_roughness"])
    mats = scenes._materials([scenes.metal(METAL["eta"], METAL["k"], METAL["u_roughness"])])
    point_light_check(hip_ctx, f"{kind} scaled metal", kind, "scaled", False,
                      lambda g: g.set_material_roughness(0, METAL["u_roughness"], METAL["v_roughness"]),
                      lambda wo, wi: mm.bsdf_f(model, wo, wi), ("front",), materials=mats)


# ---------------------------------------------------------------------------------------------------------------------
# c. integrators and lights
# ---------------------------------------------------------------------------------------------------------------------
def straight_strip(kind, material=0):
    normals = [(0.0, 0.0, 1.0), (0.0, 1.0, 1.0)] if kind == "ribbon" else None
    return scenes.curve(STRIP_CP, STRIP_W, STRIP_W, type=kind, normals=normals, material=material, split_depth=1)


def rays_onto_the_strip(n, seed, z_from=5.0, half=0.12):
    """parallel rays along -z (from below: +z) onto the middle of the strip: every one hits, the ribbon's narrowed width too"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-half, half, n), np.full(n, z_from)], -1).astype(np.float32)
    d = np.broadcast_to(np.array([0.0, 0.0, -1.0 if z_from > 0 else 1.0], np.float32), (n, 3))
    return o, d


@pytest.mark.parametrize("kind", cc.TYPES)
def test_ambient_occlusion_on_a_strip(hip_ctx, kind):
    """k_shade_direct<AO> in the build for curves. A straight strip alone, seen through strip_view's camera: no ray that leaves
    it into its normal's hemisphere meets it again (the model finds none among 4096 cosine-distributed ones), so with
    cos_sample every hit gives pi (1e-4 on the mean as test_ambient_occlusion_closed_forms, and no sample below it), every miss
    0, and 16 shadow rays per hit."""
    g = pbrt_hip.Scene(hip_ctx, curve_scene([straight_strip(kind)], materials=MATTE))
    cam = scenes.orthographic_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 32, 32)
    rays, keys, _, _ = g.camera_rays(cam, 32, 32, 16, seed=4)
    hits = g.intersect(rays)["prim_id"] >= 1
    rgb, st = g.li(rays, keys, integrator=AO, ao_samples=16, light_strategy=1)
    g.close()
    print(f"{kind}: {hits.sum()} hits of {len(rays)}, mean over the hits {rgb[hits].mean():.6f}, least {rgb[hits].min():.6f}, shadow rays {st['rays_shadow']}")
    assert hits.sum() > 3000 and (rgb[~hits] == 0).all()
    assert abs(rgb[hits].mean() - np.pi) < 1e-4 and rgb[hits].min() > np.pi - 1e-4
    assert st["rays_shadow"] == 16 * hits.sum()


def share_past_a_square(half, h):
    """the cosine-weighted share of the hemisphere about the axis of a square of side 2 half, seen from the distance h on that
    axis, that passes the square: 1 - the form factor of a point to a parallel rectangle, four corner rectangles
    (1 / 2 pi) [X / sqrt(1 + X^2) atan(Y / sqrt(1 + X^2)) + Y / sqrt(1 + Y^2) atan(X / sqrt(1 + Y^2))] with X = Y = half / h"""
    x = half / h
    s = np.sqrt(1 + x * x)
    return 1.0 - 4.0 / (2.0 * np.pi) * 2.0 * (x / s) * np.arctan(x / s)


@pytest.mark.parametrize("kind", cc.TYPES)
def test_ambient_occlusion_under_a_strip_that_faces_a_plane(hip_ctx, kind):
    """the strip 2 above a plane 200 wide, seen from between the two: the normal, turned to the viewer, leans towards the plane.
    (2 and not the issue's 0.5: spawn_ray starts a ray |n| . p_error = 2 hit_width (|n_x| + |n_y| + |n_z|), 1 to 1.42 here, off
    the surface, which at 0.5 would be beyond the plane.) The flat type's normal faces the plane squarely: every sample is
    occluded but the share that passes the plane's edge, at most share_past_a_square(100, 1) = 8.2e-5 (the rays start 0.58 to 1
    above the plane and within 1 of its axis, which moves the share by less than a hundredth of itself). The cylinder type's
    normal is turned about the axis by theta = lerp(v, -90, 90) degrees and the ribbon's by its n_hit, and the cosine-weighted
    share of a hemisphere above the plane's horizon is (1 - cos theta) / 2: the mean of value - pi (1 - |n_z|) / 2 is 0 within 5
    sigma and that share, sigma being at most 0.004 of pi."""
    half, gap = 100.0, 2.0
    plane = dict(positions=np.array([(-half, -half, -gap), (half, -half, -gap), (half, half, -gap), (-half, half, -gap)], dtype=np.float32),
                 indices=np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    curves = straight_strip(kind)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=MATTE, extra=plane))
    o, d = rays_onto_the_strip(4096, 21, z_from=-0.25)
    rays = as_rays(o, d)
    prim = g.intersect(rays)["prim_id"]
    rgb, st = g.li(rays, np.arange(len(o), dtype=np.uint64) * 5 + 1, integrator=AO, ao_samples=16, light_strategy=1)
    g.close()
    assert (prim >= 2).all() and st["rays_shadow"] == 16 * len(o)
    value = rgb[:, 0].astype(np.float64)
    share = share_past_a_square(half, 1.0)
    if kind == "flat":
        n_samples = 16 * len(o)
        allowed = np.pi * (share + 5 * np.sqrt(share / n_samples))
        print(f"{kind}: mean {value.mean():.3e}, share that passes the plane {share:.3e}, allowed mean {allowed:.3e}")
        assert share < 1e-4 and value.mean() <= allowed
    else:
        m = cm.intersect_many(curves, o, d)
        n_z = np.abs(cc.surface_of(curves, o, d, np.inf, m)["n"][:, 2])
        diff = value - np.pi * (1.0 - n_z) / 2.0
        sigma = diff.std(ddof=1) / np.sqrt(len(diff))
        print(f"{kind}: mean value {value.mean():.4f}, mean difference from the model {diff.mean():.5f}, sigma {sigma:.5f}")
        assert value.mean() > 0.05 and sigma <= 0.004 * np.pi and abs(diff.mean()) <= 5 * sigma + np.pi * share


ENV_LE = 0.8


@pytest.mark.parametrize("integrator,strategy", [(PATH, 0), (PATH, 1), (PATH, 2), (DIRECT, 0), (DIRECT, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", cc.TYPES)
def test_a_strip_under_a_constant_environment(hip_ctx, kind, integrator, strategy):
    """estimate_direct's light- and BSDF-sampled halves with MIS against an infinite light, started on a curve: matte Kd under
    a constant Le, depth 1. Nothing stands in the way of a ray that leaves a straight strip, so every hit expects Kd Le."""
    g = pbrt_hip.Scene(hip_ctx, curve_scene([straight_strip(kind)], materials=MATTE, lights=[(scenes.LIGHT_INFINITE, (ENV_LE,) * 3, -1, 0, 1)]))
    o, d = rays_onto_the_strip(4096, 31)
    rays = as_rays(o, d)
    assert (g.intersect(rays)["prim_id"] >= 1).all()
    rgb, _ = g.li(rays, np.arange(len(o), dtype=np.uint64) * 3 + 2, integrator=integrator, max_depth=1, light_strategy=strategy)
    g.close()
    value = rgb[:, 0].astype(np.float64)
    want = KD * ENV_LE
    sigma = value.std(ddof=1) / np.sqrt(len(value))
    print(f"{kind} integrator {integrator} strategy {strategy}: mean {value.mean():.5f} against {want:.5f}, sigma {sigma:.5f}, 5 sigma / value {5 * sigma / want:.4f}")
    assert np.isfinite(rgb).all() and 5 * sigma / want <= 0.02
    assert abs(value.mean() - want) <= 5 * sigma


def polygon_irradiance(p, n, verts, L):
    """Lambert's formula: E = L / 2 * sum_i gamma_i (n . Gamma_i) over the edges of a polygon wholly above the horizon of n, gamma_i
    the angle the edge subtends at p and Gamma_i the unit normal of the plane through p and the edge"""
    v = verts[None, :, :] - p[:, None, :]
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    total = np.zeros(len(p))
    for i in range(verts.shape[0]):
        a, b = v[:, i], v[:, (i + 1) % verts.shape[0]]
        gamma = np.arccos(np.clip((a * b).sum(-1), -1, 1))
        c = np.cross(a, b)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        total += gamma * (c * n).sum(-1)
    return L / 2.0 * np.abs(total)


@pytest.mark.parametrize("integrator", [DIRECT, PATH], ids=["direct", "path"])
def test_a_strip_under_a_mesh_emitter(hip_ctx, integrator):
    """a shadow ray (and estimate_direct's BSDF-sampled ray) from a curve towards an area light: a one-sided quad emitter facing
    down, 3 above a straight cylinder-type strip. The hits kept are those whose normal (the model's, turned to the viewer) has
    the whole quad at least 0.1 above its horizon; there L = Kd / pi * E(p, n) with E by Lambert's polygon formula."""
    L_e = 5.0
    quad = np.array([(-1.0, -1.0, 3.0), (-1.0, 1.0, 3.0), (1.0, 1.0, 3.0), (1.0, -1.0, 3.0)])   # normalize(dp02 x dp12) = -z
    mesh = dict(positions=quad.astype(np.float32), indices=np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32),
                tri_material=np.zeros(2, np.int32), tri_light=np.array([0, 1], np.int32))
    curves = straight_strip("cylinder")
    lights = [(scenes.LIGHT_DIFFUSE_AREA, (L_e,) * 3, 0, 0, 1), (scenes.LIGHT_DIFFUSE_AREA, (L_e,) * 3, 1, 0, 1)]
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=MATTE, lights=lights, extra=mesh))
    o, d = rays_onto_the_strip(4096, 41, z_from=2.0, half=0.24)
    rays = as_rays(o, d)
    assert (g.intersect(rays)["prim_id"] >= 2).all()
    rgb, _ = g.li(rays, np.arange(len(o), dtype=np.uint64) * 7 + 3, integrator=integrator, max_depth=1, light_strategy=0)
    g.close()
    m = cm.intersect_many(curves, o, d)
    surf = cc.surface_of(curves, o, d, np.inf, m)
    n = surf["n"] * np.sign(surf["n"][:, 2:3])   # to the viewer's side (+z), where the emitter is
    above = ((quad[None, :, :] - surf["p"][:, None, :]) * n[:, None, :]).sum(-1).min(1)
    keep = m["hit"] & (m["margin"] >= 0.05) & (above > 0.1)
    want = KD / np.pi * polygon_irradiance(surf["p"][keep], n[keep], quad, L_e)
    diff = rgb[keep, 0].astype(np.float64) - want
    sigma = diff.std(ddof=1) / np.sqrt(keep.sum())
    print(f"integrator {integrator}: kept {keep.sum()} of {len(o)}, mean expected {want.mean():.5f}, mean difference {diff.mean():.6f}, "
          f"sigma {sigma:.6f}, 5 sigma / value {5 * sigma / want.mean():.4f}")
    assert keep.sum() > 1500 and np.isfinite(rgb).all() and 5 * sigma / want.mean() <= 0.02
    assert abs(diff.mean()) <= 5 * sigma


@pytest.mark.parametrize("kind", ["flat", "ribbon"])
def test_specular_glass_on_a_strip(hip_ctx, kind):
    """Kr = Kt = 1, eta 1.5 on a straight strip under a constant environment, the path integrator at max_depth 4 without
    roulette. A strip is one interface, not a slab: a sample that misses or reflects returns Le, and one that refracts returns
    Le (eta_i / eta_t)^2 (TransportMode::Radiance), eta_i on the side of the model's normal the ray comes from; nothing else, so
    the issue's "every sample equals Le" holds for the reflected ones only. Every continuation ray escapes: a closest-hit ray per
    camera sample and one more per hit, and one that met the curve where it starts would add to that."""
    le, eta = 0.7, 1.5
    mats = scenes._materials([(scenes.MAT_GLASS, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), eta)])
    curves = straight_strip(kind)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves, materials=mats, lights=[(scenes.LIGHT_INFINITE, (le,) * 3, -1, 0, 1)]))
    cam = scenes.orthographic_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 32, 32)
    rays, keys, _, _ = g.camera_rays(cam, 32, 32, 16, seed=9)
    hits = g.intersect(rays)["prim_id"] >= 1
    rgb, st = g.li(rays, keys, integrator=PATH, max_depth=4, rr_threshold=0.0)
    g.close()
    o, d = rays["o"], rays["d"]
    m = cm.intersect_many(curves, o, d)
    surf = cc.surface_of(curves, o, d, np.inf, m)
    outside = (surf["n"] * -d).sum(-1) > 0   # the ray arrives on the side the normal points to: it enters
    refracted = le * np.where(outside, 1.0 / eta ** 2, eta ** 2)
    value = rgb[:, 0].astype(np.float64)
    is_le, is_refracted = np.isclose(value, le, rtol=1e-5, atol=0), np.isclose(value, refracted, rtol=1e-5, atol=0)
    print(f"{kind}: {hits.sum()} hits, reflected {is_le[hits].mean():.4f}, refracted {is_refracted[hits].mean():.4f}, closest-hit rays {st['rays_closest']}")
    sure = m["margin"] >= cc.MARGIN
    assert hits.sum() > 3000 and np.array_equal(hits[sure], m["hit"][sure]) and sure.mean() > 0.99 and is_le[~hits].all()
    assert (is_le | is_refracted)[hits].all() and 0.01 < is_le[hits].mean() < 0.2   # R = 0.04 at normal incidence
    assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 0] == rgb[:, 2]).all()
    assert st["rays_closest"] == len(rays) + hits.sum()
