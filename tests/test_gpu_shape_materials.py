"""Glossy, specular and Disney materials on the quadric shapes (k_shade_shapes, k_shade_direct<., 3 + kDirectShapes>), held to the
float64 models: the tangent frame of make_surface_shape through anisotropic lobes under a point light, on every shape, transform
and sweep; reflection about a curved, transformed surface under an image environment map; a lossless glass sphere whose paths
continue into the body; the glossy furnace on convex bodies (bsdf_sample_f's to_world on a shape's frame); shape lights seen by a
lobe narrow enough for the BSDF-sampled branch of estimate_direct to carry the estimate; the ray down a disk's axis; and the
films of the older levels, unchanged by a shape nothing sees. Cases, references and allowances: shape_material_cases.py, held on
the CPU by test_shape_material_model.py."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import quadric_model as qm
import shape_material_cases as smc
from test_quadric_model import TRANSFORMS
from test_gpu_shapes import (N_FACTOR, NORMAL_PROBE_SPHERE_PATH_WORST, as_rays, floor_quad, shape_scene)

pytestmark = pytest.mark.gpu
PATH, DIRECT, WHITTED, AO = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO
NAMES = {PATH: "path", DIRECT: "direct", WHITTED: "whitted"}


def open_scene(hip_ctx, rec, row, lights):
    sc, after = smc.material_scene(rec, row, lights)
    scene = pbrt_hip.Scene(hip_ctx, sc)
    after(scene)
    return scene


# ---- 2.1 the point-light closed form on every shape ----
@pytest.mark.parametrize("case", smc.POINT_CASES, ids=smc.POINT_IDS)
def test_point_light_closed_form_on_shapes(hip_ctx, case):
    """test_gpu_lobe_materials.py::test_point_light_closed_form on a shape: Li = f(wo_l, wi_l) I |ns . wi| / r^2 with the local
    directions through the model's frame (qm.surface_frame) at the model's hit point, by the path integrator at depth 1, direct
    lighting and Whitted, light_strategy 0. A point light and one surface interaction: no random number reaches the result.
    Per-ray allowance, derived: the device's hit point is within T_TOL t of the model's along the ray (test_gpu_shapes.py), so
    the model is evaluated at t (1 +- T_TOL) and the larger change taken; to that the plane test's rtol 1e-4, the same BSDF code
    with no curvature. That the anisotropic rows tell a wrong frame from the right one at this allowance is
    test_shape_material_model.py::test_point_light_cases_keep_enough_rays_and_can_fail."""
    name, rec, row_name, _ = case
    shape, row = qm.from_record(rec[0]), smc.ROWS[row_name]
    light, o, d = smc.point_setup(case)
    c = smc.point_light_case(shape, row, light, o, d, wrong_frames=True)
    keep = c["keep"]
    assert keep.sum() >= smc.MIN_KEPT
    scene = open_scene(hip_ctx, rec, row, [scenes.point_light(tuple(light), tuple(smc.LIGHT_I))])
    rays, keys = as_rays(o, d), np.arange(len(o), dtype=np.uint64) * 7919 + 3
    got = {integ: scene.li(rays, keys, integrator=integ, max_depth=1, light_strategy=0)[0].astype(np.float64) for integ in NAMES}
    scene.close()
    worst = {}
    for integ, rgb in got.items():
        ratio = np.abs(rgb[keep] - c["ref"][keep]) / c["allow"][keep]
        worst[NAMES[integ]] = float(ratio.max())
    print(f"{name}: kept {keep.sum()} of {len(o)}, worst error over allowance {worst}")
    for integ, rgb in got.items():
        assert np.isfinite(rgb).all(), (name, NAMES[integ])
        bad = (np.abs(rgb - c["ref"]) > c["allow"]).any(axis=1) & keep
        assert not bad.any(), (name, NAMES[integ], worst[NAMES[integ]], np.flatnonzero(bad)[:5], rgb[bad][:2], c["ref"][bad][:2])


# ---- 2.2 the reflection direction ----
@pytest.mark.parametrize("name,rec", smc.MIRROR_CASES, ids=[c[0] for c in smc.MIRROR_CASES])
def test_mirror_reflects_the_environment_map(hip_ctx, name, rec):
    """A mirror (Kr = 0.9, 0.8, 0.7) on a sphere (under "scaled": an ellipsoid), a cylinder and a disk whose only light is an
    image environment map under a generic light_to_world: where the reflected ray misses the shape (by the model; always so on a
    convex body's outside) Li = Kr le(reflect(d, n)), by the path integrator at depth 2 and by Whitted's and direct lighting's
    specular branch at depth 2. reflect() reads the normal with twice Lambert's sensitivity. Allowance as in the point-light test:
    the model's hit moved by T_TOL t, plus 1e-4 relative."""
    shape = qm.from_record(rec[0])
    o, d = smc.select_rays(shape)
    c = smc.mirror_case(shape, o, d)
    keep = c["keep"]
    assert keep.sum() >= smc.MIN_KEPT
    scene = open_scene(hip_ctx, rec, smc.MIRROR_ROW, [(scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1)])
    scene.set_environment_map(0, smc.ENV_MAP, smc.ENV_TO_WORLD)
    rays, keys = as_rays(o, d), np.arange(len(o), dtype=np.uint64) * 7919 + 3
    got = {integ: scene.li(rays, keys, integrator=integ, max_depth=2, light_strategy=0)[0].astype(np.float64) for integ in NAMES}
    scene.close()
    worst = {NAMES[i]: float((np.abs(rgb[keep] - c["ref"][keep]) / c["allow"][keep]).max()) for i, rgb in got.items()}
    print(f"{name}: kept {keep.sum()} of {len(o)}, worst error over allowance {worst}")
    for integ, rgb in got.items():
        bad = (np.abs(rgb - c["ref"]) > c["allow"]).any(axis=1) & keep
        assert not bad.any(), (name, NAMES[integ], worst[NAMES[integ]], np.flatnonzero(bad)[:5], rgb[bad][:2], c["ref"][bad][:2])


# ---- 2.3 the lossless glass sphere ----
def glass_samples(hip_ctx, to_world):
    rec = scenes.sphere_shape(0.8, to_world=to_world)
    shape = qm.from_record(rec[0])
    o, d = smc.select_rays(shape, n=smc.GLASS_RAYS)
    row = dict(row=(scenes.MAT_GLASS, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), smc.GLASS_ETA), desc=None, roughness=None)
    scene = open_scene(hip_ctx, rec, row, [(scenes.LIGHT_INFINITE, smc.GLASS_LE, -1, 0, 1)])
    n = smc.GLASS_RAYS * smc.GLASS_KEYS
    rgb, _ = scene.li(np.repeat(as_rays(o, d), smc.GLASS_KEYS), np.arange(n, dtype=np.uint64) * 31 + 11, integrator=PATH,
                      max_depth=smc.GLASS_DEPTH, rr_threshold=0.0)
    scene.close()
    return shape, o, d, rgb.astype(np.float64).reshape(smc.GLASS_RAYS, smc.GLASS_KEYS, 3)


def two_values(rgb, name):
    """every sample is 0 or Le; returns the mask of the nonzero ones. rtol 2e-5: the project holds one pass through a surface to
    1e-6 (test_gpu_lobe_materials.py::test_exact_pass_through); a path here multiplies up to twelve f |cos| / pdf factors and the
    eta^2 pair of entering and leaving, so 12 x 1e-6 = 1.2e-5, rounded up to one digit."""
    le = np.asarray(smc.GLASS_LE)
    zero = (rgb == 0.0).all(axis=-1)
    rel = np.abs(rgb[~zero] / le - 1.0)
    print(f"{name}: {zero.mean():.5f} of the samples are 0, the others are off Le by at most {rel.max():.3g} (allowed {smc.GLASS_RTOL})")
    assert np.isfinite(rgb).all() and (rel <= smc.GLASS_RTOL).all(), (name, rel.max())
    return ~zero


@pytest.fixture(scope="module")
def glass_sphere_worst_zero_share():
    return {}


@pytest.mark.parametrize("place", list(smc.GLASS_PLACES))
def test_lossless_glass_sphere(hip_ctx, place, glass_sphere_worst_zero_share):
    """Kr = Kt = 1, eta 1.5, a constant environment Le, the path integrator at max_depth D = 12 without roulette (rr_threshold 0),
    200 rays x 64 samples. Every sample is 0 (the path is still inside after D vertices) or Le: a continuation ray that starts on
    the wrong side of the surface, or misses the far wall, gives another value or another share of zeros.
    Bounce accounting (wf_path.h, shade_bounce): `bounces` counts the scatterings done; a vertex scatters while bounces < max_depth
    and an escaped ray adds Le after a specular bounce whatever its count. So the D scatterings happen at the first hit (bounces
    0) and at the internal hits 1 .. D - 1; a path still inside at internal hit D ends with 0. A chord of a sphere meets it at
    the same angle at both ends, so every vertex reflects with the first hit's R = fr_dielectric(cos theta): the share of
    samples that return Le is 1 - (1 - R) R^(D - 1), the issue's form without adjustment
    (test_shape_material_model.py::test_glass_sphere_share_against_a_simulation). Per ray within 4 binomial sigma (+ 1e-12:
    where the share is 1 to rounding, sigma is 0 and every sample must be Le)."""
    shape, o, d, rgb = glass_samples(hip_ctx, smc.GLASS_PLACES[place])
    lit = two_values(rgb, place)
    share, skip = smc.glass_sphere_share(shape, o, d)
    assert skip.mean() <= 0.05
    got = lit.mean(axis=1)
    sigma = np.sqrt(share * (1.0 - share) / smc.GLASS_KEYS)
    dev = np.abs(got - share)[~skip]
    k = np.argmax(dev - 4.0 * sigma[~skip])
    print(f"{place}: expected share of Le from {share[~skip].min():.4f} to {share[~skip].max():.6f}, observed from {got[~skip].min():.4f}; "
          f"worst ray: observed {got[~skip][k]:.4f} expected {share[~skip][k]:.4f} sigma {sigma[~skip][k]:.4f}")
    glass_sphere_worst_zero_share[place] = float((1.0 - got[~skip]).max())
    assert (dev <= 4.0 * sigma[~skip] + 1e-12).all(), (place, got[~skip][k], share[~skip][k], sigma[~skip][k])


def test_lossless_glass_ellipsoid(hip_ctx, glass_sphere_worst_zero_share):
    """the same on the ellipsoid ("scaled"): every sample 0 or Le, and the share of zeros over all samples below the worst ray's
    of the spheres"""
    if not glass_sphere_worst_zero_share:
        for place in smc.GLASS_PLACES:
            shape, o, d, rgb = glass_samples(hip_ctx, smc.GLASS_PLACES[place])
            skip = smc.glass_sphere_share(shape, o, d)[1]
            glass_sphere_worst_zero_share[place] = float((rgb == 0.0).all(axis=-1).mean(axis=1)[~skip].max())
    _, _, _, rgb = glass_samples(hip_ctx, TRANSFORMS["scaled"])
    lit = two_values(rgb, "ellipsoid")
    worst = max(glass_sphere_worst_zero_share.values())
    print(f"ellipsoid: share of zeros {1.0 - lit.mean():.5f}, the spheres' worst ray {worst:.5f}")
    assert 1.0 - lit.mean() < worst


# ---- 2.4 the glossy furnace on convex bodies ----
@pytest.fixture(scope="module")
def furnace_references():
    return {}


@pytest.mark.parametrize("integrator", [PATH, DIRECT], ids=["path", "direct"])
@pytest.mark.parametrize("row_name", smc.FURNACE_ROWS)
@pytest.mark.parametrize("body", list(smc.FURNACE_BODIES))
def test_glossy_furnace_on_convex_bodies(hip_ctx, furnace_references, body, row_name, integrator):
    """The level-1 plastic, level-2 substrate and level-3 Disney rows of the point-light test on the ellipsoid, the cylinder's
    outside and the disk under a constant environment Le: 12 model-chosen rays x 4096 samples each through Scene.li, path and
    direct lighting at depth 1. Li = Le albedo(wo_local), wo_local through the model's frame; the hemisphere about the viewer-side
    normal is free of the shape (test_furnace_rays_see_a_free_hemisphere). Acceptance as the project's furnace tests:
    |mean - ref| < 4 se + 1e-4 ref with the model's quadrature error below se / 4."""
    rec = smc.FURNACE_BODIES[body]
    shape, row = qm.from_record(rec[0]), smc.ROWS[row_name]
    o, d = smc.furnace_rays(shape, body.split("-")[0])
    if (body, row_name) not in furnace_references:
        furnace_references[(body, row_name)] = smc.furnace_albedo(shape, row, o, d)
    albedo, err = furnace_references[(body, row_name)]
    le = np.asarray(smc.FURNACE_LE)
    scene = open_scene(hip_ctx, rec, row, [(scenes.LIGHT_INFINITE, smc.FURNACE_LE, -1, 0, 1)])
    n = smc.FURNACE_RAYS * smc.FURNACE_KEYS
    rgb, _ = scene.li(np.repeat(as_rays(o, d), smc.FURNACE_KEYS), np.arange(n, dtype=np.uint64) * 17 + 5, integrator=integrator, max_depth=1,
                      light_strategy=0)
    scene.close()
    v = rgb.astype(np.float64).reshape(smc.FURNACE_RAYS, smc.FURNACE_KEYS, 3)
    mean, se = v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(smc.FURNACE_KEYS)
    ref = le * albedo
    print(f"{body} {row_name} {NAMES[integrator]}: green mean {mean[:, 1]} ref {ref[:, 1]} se {se[:, 1]} quadrature error {(le * err)[:, 1]}; "
          f"worst |mean - ref| / (4 se + 1e-4 ref) {np.max(np.abs(mean - ref) / (4 * se + 1e-4 * ref)):.3f}")
    assert np.isfinite(v).all()
    assert np.all(le * err < se / 4 + 1e-12), (le * err, se)
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-4 * ref), (mean, ref, se)


# ---- 2.5 a shape light seen by a narrow lobe ----
NARROW_ESTIMATORS = {"path-all": dict(integrator=PATH, max_depth=1, light_strategy=0), "path-one": dict(integrator=PATH, max_depth=1, light_strategy=1),
                     "direct-all": dict(integrator=DIRECT, max_depth=1, light_strategy=0), "direct-one": dict(integrator=DIRECT, max_depth=1, light_strategy=1)}


@pytest.mark.parametrize("light", smc.NARROW_LIGHTS)
def test_shape_light_seen_by_a_narrow_lobe(hip_ctx, light):
    """A plastic plane (Ks 0.6, Kd 0, alpha 0.05 set directly) under the disk light, the inward-emitting cylinder light and the
    rotated sphere light (R / d = 0.5) of test_gpu_shapes.py's closed forms; each of 8 plane points is seen from the mirror image
    of the direction to a point of the emitter, so the lobe sits on the emitter and the BSDF-sampled branch of estimate_direct,
    weighted with shape_light_pdf, carries the estimate: by the model (the integral of f cos times the power heuristic's weight
    with the model's pdfs over that of f cos) 0.83 to 0.89 of it under the disk, 0.97 under the cylinder, 0.78 to 0.81 under the
    sphere (test_narrow_lobe_reference_is_carried_by_the_bsdf_branch asserts > 0.5). 8192 samples per point; reference: the
    quadrature qm.bsdf_patch_radiance_by_quadrature with its halving error; acceptance 4 se + that error."""
    setup = smc.narrow_setup(light)
    ref, err, share = smc.narrow_reference(light)
    o, d = smc.narrow_rays(setup)
    sc = shape_scene([setup["rec"]], materials=scenes._materials([smc.NARROW_ROW["row"], (scenes.MAT_NONE, (0, 0, 0), (0, 0, 0), 1.0)]),
                     lights=[(scenes.LIGHT_DIFFUSE_AREA, (smc.NARROW_LE,) * 3, 2, setup["two_sided"], 1)], extra=floor_quad(20.0, setup["y"]))
    scene = pbrt_hip.Scene(hip_ctx, sc)
    scene.set_material_roughness(0, *smc.NARROW_ROW["roughness"][:2], remap=False)
    n = smc.NARROW_POINTS * smc.NARROW_KEYS
    rays, keys = np.repeat(as_rays(o, d), smc.NARROW_KEYS), np.arange(n, dtype=np.uint64) * 13 + 7
    got = {name: scene.li(rays, keys, **kw)[0].astype(np.float64).reshape(smc.NARROW_POINTS, smc.NARROW_KEYS, 3) for name, kw in NARROW_ESTIMATORS.items()}
    scene.close()
    print(f"{light}: BSDF-branch share by the model {share}")
    for name, v in got.items():
        mean, se = v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(smc.NARROW_KEYS)
        print(f"{light} {name}: green mean {mean[:, 1]} ref {ref[:, 1]} se {se[:, 1]} quadrature error {err[:, 1]}; "
              f"worst |mean - ref| / (4 se + error) {np.max(np.abs(mean - ref) / (4 * se + err)):.3f}")
    for name, v in got.items():
        mean, se = v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(smc.NARROW_KEYS)
        assert np.isfinite(v).all() and (mean > 0.0).all(), name
        assert np.all(np.abs(mean - ref) <= 4 * se + err), (light, name, mean, ref, se)


# ---- 2.6 the disk's axis ----
AXIS_RHO, AXIS_L = 0.5, 3.0


@pytest.mark.parametrize("place", ["identity", "scaled"])
def test_a_ray_down_the_disks_axis(hip_ctx, place):
    """Rays exactly along the object z axis of a full disk without a hole, from both sides, under one distant light on either
    side in turn: Li is the Lambert closed form at the centre (rho / pi L |n . w| on the light's side, exactly 0 on the other), to
    test_normals_through_lamberts_law's tolerance, where the reference's dpdv = p (r_i - r) / |p| is 0 / 0 and the sample used
    to be lost as a NaN. And under the AO integrator, which builds its hemisphere on dpdu: finite, and the
    value of a ray beside the axis."""
    rec = scenes.disk(0.1, 1.0, to_world=TRANSFORMS[place])
    shape = qm.from_record(rec[0])
    m = shape["o2w"]
    centre, axis = m[:3, :3] @ [0.0, 0.0, shape["z_min"]] + m[:3, 3], m[:3, :3] @ [0.0, 0.0, 1.0]
    axis /= np.linalg.norm(axis)
    o = np.stack([centre + 2.0 * axis, centre - 2.0 * axis]).astype(np.float32)
    d = np.stack([-axis, axis]).astype(np.float32)
    model = qm.intersect(shape, o, d)
    assert model["hit"].all()
    tol = N_FACTOR * NORMAL_PROBE_SPHERE_PATH_WORST * np.linalg.cond(m[:3, :3], 2)
    w = np.array([0.3, 0.5, 0.81]) / np.linalg.norm([0.3, 0.5, 0.81])
    for sign in (1.0, -1.0):
        scene = pbrt_hip.Scene(hip_ctx, shape_scene([rec], lights=[scenes.distant_light(sign * w, (AXIS_L,) * 3)]))
        hits = scene.intersect(as_rays(o, d))
        assert (hits["prim_id"] == 1).all()
        for integ in (DIRECT, PATH):
            rgb, _ = scene.li(as_rays(o, d), np.arange(2, dtype=np.uint64) + 1, integrator=integ, max_depth=1, light_strategy=0)
            got = rgb.astype(np.float64) * (np.pi / (AXIS_RHO * AXIS_L))
            cos = model["n"] @ (sign * w)
            lit = ((model["n"] * -d.astype(np.float64)).sum(axis=1) * cos) > 0.0  # the light on the viewer's side
            expect = np.where(lit, np.abs(cos), 0.0)
            print(f"{place} light {sign:+.0f} {NAMES[integ]}: recovered |n . w| {got[:, 1]} expected {expect}, "
                  f"worst error over tolerance {np.abs(got - expect[:, None]).max() / tol:.3g}")
            assert np.isfinite(rgb).all() and lit.sum() == 1
            assert (got[~lit] == 0.0).all()
            assert np.abs(got - expect[:, None]).max() <= tol
        n_keys = 256
        off = o + (m[:3, :3] @ [0.05, 0.0, 0.0]).astype(np.float32)
        ao = {}
        for what, origins in (("axis", o), ("beside", off)):
            rgb, _ = scene.li(np.repeat(as_rays(origins, d), n_keys), np.arange(2 * n_keys, dtype=np.uint64) + 9, integrator=AO, ao_samples=16)
            assert np.isfinite(rgb).all(), what
            v = rgb[:, 1].astype(np.float64)
            ao[what] = (v.mean(), v.std(ddof=1) / np.sqrt(len(v)))
        scene.close()
        print(f"{place} AO: on the axis {ao['axis'][0]:.5f} +- {ao['axis'][1]:.5f}, beside it {ao['beside'][0]:.5f} +- {ao['beside'][1]:.5f}")
        assert ao["axis"][0] > 0.0
        assert abs(ao["axis"][0] - ao["beside"][0]) <= 4.0 * np.hypot(ao["axis"][1], ao["beside"][1]) + 1e-5 * ao["beside"][0]


# ---- 2.7 the SHP build leaves older films alone ----
def _older_scenes():
    from glossy_cases import _glossy_mixed
    from test_gpu_disney import _level2_mixed
    from test_gpu_lobe_materials import _disney_mixed
    return {"mixed": lambda: scenes.mixed_materials_scene(n_tris=3000), "glossy_mixed": _glossy_mixed, "level2_mixed": _level2_mixed,
            "disney_mixed": _disney_mixed}


# Where no path goes. The four scenes are one open cloud of triangles in [-1.08, 1.08]^3 under an emitter quad at y = 1.6
# (|x|, |z| <= 0.5) and an environment light, seen from (0, 0, 3.5): no wall closes anything off, so "unreachable" is a matter of
# measure. The speck must also stay inside the triangles' bounding box: the scene's bounds give the infinite light its radius, hence
# its power (pi r^2) in the light distribution, so a shape that moves them changes which light a path picks (a speck 1000 units away does: the
# path integrator then traces a fifth more rays). It sits in the empty corner beside the emitter, at (1, 1.55, -1): from any point
# of the cloud or the camera it subtends less than 3e-6 sr, 2e-7 of the sphere of directions, and a render of 64 x 64 x 4 paths to
# depth 5 traces some 5e4 rays, none of them aimed. The renders are deterministic: were the speck ever hit, the ray counts and
# the film would differ and the test would say so, every time.
SPECK_AT = (1.0, 1.55, -1.0)
SPECK = scenes.sphere_shape(1e-3, to_world=np.array([[1, 0, 0, SPECK_AT[0]], [0, 1, 0, SPECK_AT[1]], [0, 0, 1, SPECK_AT[2]], [0, 0, 0, 1.0]]), material=0)


@pytest.mark.parametrize("shade_order", [0, 1, 2])
@pytest.mark.parametrize("integrator", [PATH, DIRECT, WHITTED], ids=["path", "direct", "whitted"])
@pytest.mark.parametrize("base", ["mixed", "glossy_mixed", "level2_mixed", "disney_mixed"])
def test_unused_shape_leaves_old_films_bit_identical(hip_ctx, base, integrator, shade_order):
    """The scenes of test_unused_glossy_rows_..., test_unused_level2_rows_... and test_unused_disney_row_... (their builders,
    levels 0 to 3) with one shape nothing sees: k_shade_shapes and k_shade_direct<., 3 + kDirectShapes> render, bit for bit and
    with the same ray counts, what k_shade<., LEVEL> and k_shade_direct<., LEVEL> render without it, as the comment above
    k_shade_shapes says."""
    from test_gpu_lobe_materials import _render
    sc = _older_scenes()[base]()
    lo, hi = pbrt_hip.shape_world_bounds(SPECK)
    assert (lo[0] > sc["positions"].min(axis=0)).all() and (hi[0] < sc["positions"].max(axis=0)).all()  # the scene's bounds stay
    f0, s0 = _render(hip_ctx, sc, integrator, shade_order)
    f1, s1 = _render(hip_ctx, dict(sc, shapes=scenes.shapes(SPECK)), integrator, shade_order)
    assert np.isfinite(f0).all() and f0[..., :3].mean() > 0.01
    assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
