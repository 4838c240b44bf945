"""Disk, Cylinder and the general Sphere on the device (pbrt_hip_scene_create_with_shapes): the translated-sphere path pinned bit
for bit, intersection against the float64 model of quadric_model.py, any-hit against closest-hit, the surface normal and the
shadow rays' start through Lambert's law under six distant lights, the side a one-sided shape light emits to, the convex-body
furnace (also far from the origin, tiny and huge), the closed forms of disk, cylinder and sphere lights (partial cylinder, rotated
sphere, mirrored one-sided disk) with the estimators' mutual agreement, and the creation errors."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import quadric_model as qm
from test_quadric_model import TRANSFORMS, RECORDS, ORTHONORMAL_MIRROR, PROBE_AXES, PROBE_RAYS, probe_exclusion, translate, rot, scale

pytestmark = pytest.mark.gpu

# Tolerance of |t_dev - t_model| / t_model on rays the model does not flag `near`, measured and not chosen: the translated-sphere
# path that predates the shapes (scene["spheres"], unchanged by them) was run on the generator of this file (20 000 rays of
# qm.rays_at_unit_cube per sphere; radii 0.3, 0.65 and 1.0 at offsets inside the unit cube) against the same model; its worst
# relative error of t over the agreeing hits was SPHERE_PATH_WORST_REL_T. The shapes are allowed T_FACTOR times that: the cylinder
# runs the same interval quadratic with fewer terms and the disk is one division, so neither should be worse than the sphere; a
# general transform adds the rounding of nine more products to the ray, which the factor covers.
SPHERE_PATH_WORST_REL_T = 7.775233e-06  # gfx950 (MI355X), the same figure from the library before and after the shapes
T_FACTOR = 4.0
T_TOL = T_FACTOR * SPHERE_PATH_WORST_REL_T

FAR_TRIANGLE = dict(positions=np.array([[50.0, 50.0, 50.0], [50.001, 50.0, 50.0], [50.0, 50.001, 50.0]], dtype=np.float32),
                    indices=np.array([[0, 1, 2]], dtype=np.int32))  # a scene needs a triangle: a speck far from everything


def shape_scene(shape_records, materials=None, lights=(), extra=None):
    """The shapes beside the far speck (or `extra`: positions / indices / tri_material / tri_light of real triangles)."""
    geo = extra or dict(FAR_TRIANGLE, tri_material=np.zeros(1, dtype=np.int32), tri_light=np.full(1, -1, dtype=np.int32))
    return dict(positions=geo["positions"], indices=geo["indices"], tri_material=geo["tri_material"], tri_light=geo["tri_light"],
                materials=materials if materials is not None else scenes._materials([(scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)]),
                lights=scenes._lights(list(lights)), shapes=scenes.shapes(*shape_records))


def as_rays(o, d, t_max=np.inf):
    rays = np.zeros(len(o), dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_max"] = o, d, t_max
    return rays


# ---------------------------------------------------------------------------------------------------------------------
# 1. the old path pinned bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def spheres_both_ways(light_on_sphere=False):
    sc = scenes.mixed_materials_scene(n_tris=64)
    u = scenes.pcg32_float(13, 8 * 4).reshape(8, 4)
    sph = np.zeros((8, 8), dtype=np.float32)
    sph[:, :3], sph[:, 3], sph[:, 5] = u[:, :3] * 1.6 - 0.8, 0.03 + 0.25 * u[:, 3], -1
    sph[:, 4] = np.arange(8) % 3
    if light_on_sphere:
        n_prims_before = sc["indices"].shape[0]
        sc["lights"] = scenes._lights(list(sc["lights"]) + [(scenes.LIGHT_DIFFUSE_AREA, (9.0, 8.0, 7.0), n_prims_before + 2, 0, 1)])
        sph[2, 4], sph[2, 5] = 0, len(sc["lights"]) - 1
    a, b = dict(sc, spheres=sph), dict(sc)
    b["shapes"] = scenes.shapes(*[scenes.sphere_shape(float(s[3]), to_world=translate(*s[:3].astype(np.float64)), material=int(s[4]), light=int(s[5]))
                                  for s in sph])
    return a, b, sph


def test_translated_full_spheres_equal_the_sphere_path_bit_for_bit(hip_ctx):
    a, b, sph = spheres_both_ways()
    ga, gb = pbrt_hip.Scene(hip_ctx, a), pbrt_hip.Scene(hip_ctx, b)
    assert ga.nodes.tobytes() == gb.nodes.tobytes() and np.array_equal(ga.prim_order, gb.prim_order)
    assert gb.wide_records() == (-1, "scene with shapes")
    rays = scenes.random_rays(20_000, 31, origin_extent=1.5)
    rays["t_max"][:500] = 0.5
    inside = rays[:2000].copy()
    inside["o"] = sph[np.arange(2000) % 8, :3]  # from the centres: the second root is the hit
    rays = np.concatenate([rays, inside])
    ha, hb = ga.intersect(rays), gb.intersect(rays)
    assert (ha["prim_id"] >= a["indices"].shape[0]).sum() > 2000
    assert ha.tobytes() == hb.tobytes()
    assert np.array_equal(ga.intersect_p(rays), gb.intersect_p(rays))
    cam = scenes.perspective_camera((0.0, 0.3, 3.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 32, 32)
    for integrator in (pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT):
        fa, _ = ga.render(cam, 32, 32, 16, integrator=integrator, max_depth=5, seed=3)
        fb, _ = gb.render(cam, 32, 32, 16, integrator=integrator, max_depth=5, seed=3)
        assert fa[..., :3].mean() > 0.01 and fa.tobytes() == fb.tobytes(), integrator
    ga.close()
    gb.close()


def test_a_full_sphere_light_equals_the_sphere_path_bit_for_bit(hip_ctx):
    a, b, _ = spheres_both_ways(light_on_sphere=True)
    ga, gb = pbrt_hip.Scene(hip_ctx, a), pbrt_hip.Scene(hip_ctx, b)
    cam = scenes.perspective_camera((0.0, 0.3, 3.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 32, 32)
    for integrator, strategy in ((pbrt_hip.INTEGRATOR_PATH, 1), (pbrt_hip.INTEGRATOR_PATH, 2), (pbrt_hip.INTEGRATOR_DIRECT, 0)):
        fa, _ = ga.render(cam, 32, 32, 16, integrator=integrator, max_depth=5, seed=5, light_strategy=strategy)
        fb, _ = gb.render(cam, 32, 32, 16, integrator=integrator, max_depth=5, seed=5, light_strategy=strategy)
        assert fa[..., :3].mean() > 0.01 and fa.tobytes() == fb.tobytes(), (integrator, strategy)
    ga.close()
    gb.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. intersection against the model, any-hit against closest-hit
# ---------------------------------------------------------------------------------------------------------------------
def check_against_model(hip_ctx, name, rec, o, d, t_max=np.inf, min_hits=100):
    g = pbrt_hip.Scene(hip_ctx, shape_scene([rec]))
    rays = as_rays(o, d, t_max)
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    g.close()
    m = qm.intersect(qm.from_record(rec[0]), o, d, t_max)
    keep = ~m["near"]
    excluded = 1.0 - keep.mean()
    dev_hit = hits["prim_id"] == 1  # primitive n_tris + 0
    assert ((hits["prim_id"] == 1) | (hits["prim_id"] == -1)).all()
    both = keep & dev_hit & m["hit"]
    rel = np.abs(hits["t"][both].astype(np.float64) - m["t"][both]) / m["t"][both]
    p_dev = np.stack([hits["b0"], hits["b1"], hits["b2"]], axis=1)[both].astype(np.float64)
    p_err = np.abs(p_dev - m["p"][both]).max() if both.any() else 0.0
    print(f"{name}: hits {m['hit'].mean():.3f} excluded {excluded:.5f} worst rel t {rel.max() if both.any() else 0.0:.3e} "
          f"worst |p_dev - p_model| {p_err:.3e} (allowed rel t {T_TOL:.3e})")
    assert excluded <= 0.01, name
    assert np.array_equal(dev_hit[keep], m["hit"][keep]), (name, np.flatnonzero(keep & (dev_hit != m["hit"]))[:5])
    assert both.sum() >= min_hits, name
    assert not both.any() or rel.max() <= T_TOL, name
    # 3. Shape::intersect_p gives intersect's verdict on every ray (both run the same test; nothing is excluded)
    assert np.array_equal(anyhit.astype(bool), dev_hit), name
    return hits, m


@pytest.mark.parametrize("name,rec", RECORDS, ids=[r[0] for r in RECORDS])
def test_intersection_against_the_model(hip_ctx, name, rec):
    o, d = qm.rays_at_unit_cube(20_000, 5)
    check_against_model(hip_ctx, name, rec, o, d)


@pytest.mark.parametrize("kind", ["sphere", "cylinder"])
def test_rays_starting_inside_take_the_second_root(hip_ctx, kind):
    m = TRANSFORMS["scaled"]
    rec = scenes.sphere_shape(0.9, to_world=m) if kind == "sphere" else scenes.cylinder(0.8, -5.0, 5.0, to_world=m)
    rng = np.random.default_rng(9)
    o_obj = rng.uniform(-0.4, 0.4, size=(20_000, 3))
    o = (o_obj @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    d = rng.normal(size=(20_000, 3))
    d = (d / np.sqrt((d ** 2).sum(axis=1))[:, None]).astype(np.float32)
    hits, model = check_against_model(hip_ctx, f"{kind}-from-inside", rec, o, d)
    assert model["hit"].mean() > 0.9 and (hits["prim_id"] == 1).mean() > 0.9  # (a cylinder's rays along the axis leave through its ends)
    # ... and a t_max short of the far side finds nothing
    short = check_against_model(hip_ctx, f"{kind}-from-inside-short", rec, o[:4000], d[:4000], t_max=0.3, min_hits=0)[0]
    assert (short["prim_id"] == -1).mean() > 0.2


def test_closest_of_several_shapes_and_triangles(hip_ctx):
    """A capped cylinder, an ellipsoid and a ring beside real triangles: the closest hit is the model's."""
    recs = [scenes.cylinder(0.4, -0.5, 0.5, to_world=TRANSFORMS["rigid"]), scenes.disk(0.5, 0.4, to_world=TRANSFORMS["rigid"]),
            scenes.disk(-0.5, 0.4, to_world=TRANSFORMS["rigid"], reverse_orientation=True),
            scenes.sphere_shape(0.35, to_world=translate(-0.5, 0.4, 0.3) @ scale(1.0, 1.6, 0.7)),
            scenes.disk(0.0, 0.6, 0.3, 300.0, to_world=translate(0.4, -0.5, -0.3) @ rot((1, 1, 0), 50.0))]
    tri = scenes.random_triangles(64, seq=3, extent=1.0, size=0.2)
    extra = dict(positions=tri["positions"], indices=tri["indices"], tri_material=np.zeros(64, dtype=np.int32), tri_light=np.full(64, -1, dtype=np.int32))
    g = pbrt_hip.Scene(hip_ctx, shape_scene(recs, extra=extra))
    only_tris = pbrt_hip.Scene(hip_ctx, dict(tri, lights=scenes._lights([]), tri_light=np.full(64, -1, dtype=np.int32)))
    o, d = qm.rays_at_unit_cube(20_000, 17)
    rays = as_rays(o, d)
    hits, t_tri = g.intersect(rays), only_tris.intersect(rays)["t"].astype(np.float64)
    anyhit = g.intersect_p(rays)
    g.close()
    only_tris.close()
    best, best_t, near = qm.intersect_scene([qm.from_record(r[0]) for r in recs], o, d)
    near |= np.isfinite(t_tri) & np.isfinite(best_t) & (np.abs(t_tri - best_t) <= qm.REL * np.maximum(t_tri, best_t))
    expect = np.where(t_tri < best_t, -2, np.where(best >= 0, best + 64, -1))  # -2: some triangle
    got = np.where((hits["prim_id"] >= 0) & (hits["prim_id"] < 64), -2, hits["prim_id"])
    keep = ~near
    assert 1.0 - keep.mean() <= 0.01
    assert np.array_equal(got[keep], expect[keep])
    for k in range(len(recs)):
        assert (got[keep] == 64 + k).sum() > 50, k
    sel = keep & (got >= 64)
    rel = np.abs(hits["t"][sel].astype(np.float64) - best_t[sel]) / best_t[sel]
    assert rel.max() <= T_TOL
    assert np.array_equal(anyhit.astype(bool), hits["prim_id"] >= 0)


# ---------------------------------------------------------------------------------------------------------------------
# 3a. the normal, through Lambert's law
# ---------------------------------------------------------------------------------------------------------------------
# The shape, matte, under six distant lights along +-PROBE_AXES[:, k], pair k emitting in channel k alone: one surface interaction
# of direct lighting returns rho / pi * L * |n . a_k| in channel k (qm.lambert_probe), or exactly 0 where the shape shadows the
# light on the viewer's side. Delta lights under UniformSampleAll: no random number reaches the result. A wrong normal matrix
# (transposed, not inverted: invisible to a furnace), a wrong dpdv or a swapped cross product changes |n . a_k|; a shadow ray
# started on the wrong side of an open shape, or any-hit disagreeing with the model, changes which channels are 0.
#
# Tolerance of |rgb_k pi / (rho L) - expected_k| (a quantity in [0, 1]), measured and not chosen, as T_TOL above: the same probe on
# the translated-sphere path (scene["spheres"]; radii 0.3, 0.65 and 1.0 at the offsets below, the same 20 000 rays each) deviated
# from the model by at most NORMAL_PROBE_SPHERE_PATH_WORST. A shape is allowed N_FACTOR times that times the condition number
# of its transform's linear part: the inverse transpose and the renormalisation amplify an object-space error of the normal
# by at most cond_2, and the factor covers the extra products of a general matrix as T_FACTOR does.
NORMAL_PROBE_SPHERE_PATH_WORST = 4.9379e-05  # gfx950 (MI355X): 4.937854e-05 (r 0.3; 2.684e-05 at r 0.65, 1.007e-05 at r 1.0), rounded up
N_FACTOR = 4.0
PROBE_RHO, PROBE_L = 0.5, 3.0
PROBE_SPHERES = ((0.3, (0.3, -0.2, 0.4)), (0.65, (-0.2, 0.1, 0.15)), (1.0, (0.0, 0.0, 0.0)))  # radius, centre


def probe_lights():
    rows = []
    for k in range(3):
        colour = np.zeros(3)
        colour[k] = PROBE_L
        rows += [scenes.distant_light(sign * PROBE_AXES[:, k], colour) for sign in (1.0, -1.0)]
    return rows


def normal_probe(hip_ctx, name, sc, model_shape):
    """Runs the probe on the scene; returns (worst deviation over the channels, worst | |n| - 1 |, the model's probe, the
    recovered |n . a_k|) after asserting what does not depend on a tolerance: the exclusion caps, misses, and the exact zeros."""
    o, d = qm.rays_at_unit_cube(*PROBE_RAYS)
    g = pbrt_hip.Scene(hip_ctx, sc)
    rgb, _ = g.li(as_rays(o, d), np.arange(len(o), dtype=np.uint64) + 1, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0)
    g.close()
    got = rgb.astype(np.float64) * (np.pi / (PROBE_RHO * PROBE_L))
    m = qm.lambert_probe(model_shape, o, d, PROBE_AXES)
    keep = m["keep"]
    near, shadow_excluded = probe_exclusion(m)
    lit = keep & ~m["shadowed"].any(axis=1)
    worst = np.abs(got[keep] - m["expect"][keep]).max()
    worst_len = np.abs(np.sqrt((got[lit] ** 2).sum(axis=1)) - 1.0).max()
    on_shadowed = got[keep][m["shadowed"][keep]]
    print(f"{name}: kept {keep.sum()} of {m['hit'].sum()} hits (near {near:.5f} of the batch, shadow rule {shadow_excluded:.5f} of the rest), "
          f"shadowed channels {len(on_shadowed)}, worst deviation {worst:.3e}, worst | |n| - 1 | {worst_len:.3e}, "
          f"nonzero on shadowed {np.count_nonzero(on_shadowed)}")
    assert near <= 0.01 and shadow_excluded <= 0.01 and keep.sum() >= 1000, name
    assert (rgb[~m["hit"] & ~m["near"]] == 0.0).all(), name  # nothing else in the scene reflects
    assert (on_shadowed == 0.0).all(), (name, np.flatnonzero(on_shadowed)[:5])
    return worst, worst_len, m, got


def test_normal_probe_on_the_sphere_path_is_the_recorded_baseline(hip_ctx):
    worst = 0.0
    for radius, centre in PROBE_SPHERES:
        sc = shape_scene([], lights=probe_lights())
        del sc["shapes"]
        sc["spheres"] = np.array([[*centre, radius, 0, -1, 0, 0]], dtype=np.float32)
        dev, dev_len, m, _ = normal_probe(hip_ctx, f"sphere path r {radius}", sc, qm.make("sphere", radius, -radius, radius, o2w=translate(*centre)))
        assert not m["shadowed"][m["keep"]].any()
        worst = max(worst, dev, dev_len)
    print(f"sphere path: worst deviation of the normal probe {worst:.6e} (recorded {NORMAL_PROBE_SPHERE_PATH_WORST:.6e})")
    assert worst <= NORMAL_PROBE_SPHERE_PATH_WORST


@pytest.mark.parametrize("name,rec", RECORDS, ids=[r[0] for r in RECORDS])
def test_normals_through_lamberts_law(hip_ctx, name, rec):
    model_shape = qm.from_record(rec[0])
    cond = np.linalg.cond(model_shape["o2w"][:3, :3], 2)
    tol = N_FACTOR * NORMAL_PROBE_SPHERE_PATH_WORST * cond
    worst, worst_len, m, _ = normal_probe(hip_ctx, name, shape_scene([rec], lights=probe_lights()), model_shape)
    print(f"{name}: cond {cond:.3f}, allowed {tol:.3e}")
    if not name.startswith("disk") and not name.endswith("-360"):
        assert m["shadowed"][m["keep"]].any(axis=1).sum() > 300, name  # the open shapes do put hits in their own shadow
    assert worst <= tol, (name, worst, tol)
    assert worst_len <= tol, (name, worst_len, tol)


# ---------------------------------------------------------------------------------------------------------------------
# 3b. the side a one-sided shape light emits to
# ---------------------------------------------------------------------------------------------------------------------
EMITTERS = {
    "sphere": lambda **kw: scenes.sphere_shape(0.7, **kw),
    "cylinder": lambda **kw: scenes.cylinder(0.5, -0.6, 0.7, **kw),
    "disk": lambda **kw: scenes.disk(0.1, 0.9, **kw),
}
EMITTER_PLACES = {"rigid": TRANSFORMS["rigid"], "mirror": ORTHONORMAL_MIRROR}
BLACK_MATTE = [(scenes.MAT_MATTE, (0.0, 0.0, 0.0), (0, 0, 0), 1.0)]


@pytest.mark.parametrize("reverse", [False, True], ids=["as-made", "reversed"])
@pytest.mark.parametrize("place", list(EMITTER_PLACES))
@pytest.mark.parametrize("kind", list(EMITTERS))
def test_one_sided_light_emits_to_the_normals_side(hip_ctx, kind, place, reverse):
    """Emitted radiance alone (path integrator, no bounce) seen by a primary ray: LE where the model's normal (pbrt-v3's:
    flipped by reverse_orientation ^ swaps_handedness) faces the ray's origin, 0 on the other side, both exactly."""
    to_world = EMITTER_PLACES[place]
    rec = EMITTERS[kind](to_world=to_world, light=0, reverse_orientation=reverse)
    le = np.float32([LE, 0.5 * LE, 0.25 * LE])
    sc = shape_scene([rec], materials=scenes._materials(BLACK_MATTE), lights=[(scenes.LIGHT_DIFFUSE_AREA, tuple(le), 1, 0, 1)])
    o, d = qm.rays_at_unit_cube(20_000, 29)
    # a closed sphere shows rays from outside one side only: a tenth of the rays start inside the shape's hollow instead
    o_obj = np.random.default_rng(3).uniform(-0.2, 0.2, size=(2000, 3))
    o[:2000] = (o_obj @ to_world[:3, :3].T + to_world[:3, 3]).astype(np.float32)
    g = pbrt_hip.Scene(hip_ctx, sc)
    rgb, _ = g.li(as_rays(o, d), np.arange(len(o), dtype=np.uint64) + 5, integrator=pbrt_hip.INTEGRATOR_PATH, max_depth=0)
    g.close()
    m = qm.intersect(qm.from_record(rec[0]), o, d)
    cos = -(m["n"] * d.astype(np.float64)).sum(axis=1)
    sure = m["hit"] & ~m["near"] & (np.abs(cos) >= 1e-3)
    front, back = sure & (cos > 0.0), sure & (cos < 0.0)
    print(f"{kind} {place} reverse {reverse}: {front.sum()} rays on the emitting side, {back.sum()} on the other, "
          f"wrong on the emitting side {(rgb[front] != le).any(axis=1).sum()}, wrong on the other {(rgb[back] != 0.0).any(axis=1).sum()}")
    assert front.sum() >= 300 and back.sum() >= 300
    assert (rgb[front] == le).all()
    assert (rgb[back] == 0.0).all()
    assert (rgb[~m["hit"] & ~m["near"]] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. convex-body furnace
# ---------------------------------------------------------------------------------------------------------------------
def furnace(hip_ctx, rec, view_dir, up, half=1.0, spp=64, res=32, centre=(0.0, 0.0, 0.0)):
    """res x res parallel rays through the pixel centres of a [-half, half]^2 window about `centre` looking along view_dir
    from 4 * half away, spp Integrator::li samples each (direct lighting, constant environment Le = 1, matte 0.5). Returns
    per-pixel mean, standard error, and the mask of pixels the model puts at least one pixel inside the silhouette."""
    w = np.asarray(view_dir, dtype=np.float64)
    w /= np.linalg.norm(w)
    r = np.cross(np.asarray(up, dtype=np.float64), w)
    r /= np.linalg.norm(r)
    u = np.cross(w, r)
    c = (np.arange(res) + 0.5) / res * 2.0 * half - half
    px, py = np.meshgrid(c, c, indexing="xy")

    def origins(dx, dy):
        return (np.asarray(centre, dtype=np.float64) - 4.0 * half * w + (px.reshape(-1, 1) + dx) * r + (py.reshape(-1, 1) + dy) * u).astype(np.float32)

    d = np.tile(w.astype(np.float32), (res * res, 1))
    shape = qm.from_record(rec[0])
    step = 2.0 * half / res
    inside = np.ones(res * res, dtype=bool)
    for dx in (-step, 0.0, step):
        for dy in (-step, 0.0, step):
            m = qm.intersect(shape, origins(dx, dy), d)
            inside &= m["hit"] & ~m["near"]
    sc = shape_scene([rec], lights=[(scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1)])
    g = pbrt_hip.Scene(hip_ctx, sc)
    rays = np.repeat(as_rays(origins(0.0, 0.0), d), spp)
    rgb, _ = g.li(rays, np.arange(len(rays), dtype=np.uint64) + 1000, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=3, light_strategy=1)
    g.close()
    v = rgb[:, 1].astype(np.float64).reshape(res * res, spp)
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 1], rgb[:, 2])
    return v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(spp), inside


FURNACE = {
    "ellipsoid": (scenes.sphere_shape(0.9, to_world=rot((1, 2, 0.5), 35.0) @ scale(1.0, 0.6, 0.8)), (0.2, -0.3, -1.0), (0, 1, 0)),
    "ellipsoid-mirrored": (scenes.sphere_shape(0.9, to_world=rot((1, 2, 0.5), 35.0) @ scale(1.0, -0.6, 0.8)), (0.2, -0.3, -1.0), (0, 1, 0)),
    "disk-front": (scenes.disk(0.0, 0.95, to_world=rot((1, 0.3, 0), 30.0)), (0.0, 0.0, -1.0), (0, 1, 0)),
    "disk-back": (scenes.disk(0.0, 0.95, to_world=rot((1, 0.3, 0), 30.0)), (0.0, 0.0, 1.0), (0, 1, 0)),
    "disk-reversed": (scenes.disk(0.0, 0.95, to_world=rot((1, 0.3, 0), 30.0), reverse_orientation=True), (0.0, 0.0, -1.0), (0, 1, 0)),
    "cylinder-side-on": (scenes.cylinder(0.7, -3.0, 3.0, to_world=rot((0, 1, 0), 90.0) @ rot((0, 0, 1), 20.0)), (0.0, 0.1, -1.0), (0, 1, 0)),
    "cylinder-scaled": (scenes.cylinder(0.7, -3.0, 3.0, to_world=rot((0, 1, 0), 90.0) @ scale(1.0, 0.7, 1.0)), (0.0, 0.1, -1.0), (0, 1, 0)),
}


@pytest.mark.parametrize("name", list(FURNACE))
def test_convex_body_furnace(hip_ctx, name):
    rec, view, up = FURNACE[name]
    mean, se, inside = furnace(hip_ctx, rec, view, up)
    assert inside.sum() > 150, (name, inside.sum())
    dev = np.abs(mean[inside] - 0.5)
    print(f"{name}: {inside.sum()} pixels inside, worst |mean - 0.5| {dev.max():.4f}, worst in sigma {np.max(dev / np.maximum(se[inside], 1e-12)):.2f}, "
          f"darkest {mean[inside].min():.4f}")
    assert (dev <= 4.0 * se[inside] + 1e-6).all(), (name, np.flatnonzero(dev > 4.0 * se[inside] + 1e-6)[:8])


def placed(rec, m):
    """The record under m @ its own to_world."""
    return scenes._shape(int(rec[0]["type"]), rec[0]["radius"], rec[0]["z_min"], rec[0]["z_max"], rec[0]["inner_radius"], rec[0]["phi_max"],
                         m @ rec[0]["to_world"].astype(np.float64).reshape(4, 4), int(rec[0]["material"]), int(rec[0]["light"]),
                         bool(rec[0]["reverse_orientation"]))


# name -> (shape of FURNACE, the transform put in front of its own, the window's half size): p_error has to follow the
# translation (|p| ~ 600: the bound is 1e4 times the one at the origin) and the scale, and offset_ray_origin has to use it in
# world space; a shadow ray that starts inside the surface gives a dark pixel
FAR = translate(300.0, -200.0, 500.0)
FURNACE_PLACED = {
    "ellipsoid-far": ("ellipsoid", FAR, 1.0),
    "disk-far": ("disk-front", FAR, 1.0),
    "ellipsoid-tiny": ("ellipsoid", scale(0.01, 0.01, 0.01), 0.01),
    "ellipsoid-huge": ("ellipsoid", scale(50.0, 50.0, 50.0), 50.0),
}


@pytest.mark.parametrize("name", list(FURNACE_PLACED))
def test_convex_body_furnace_at_placement_extremes(hip_ctx, name):
    base, m, half = FURNACE_PLACED[name]
    rec, view, up = FURNACE[base]
    mean, se, inside = furnace(hip_ctx, placed(rec, m), view, up, half=half, centre=m[:3, 3])
    assert inside.sum() > 150, (name, inside.sum())
    dev = np.abs(mean[inside] - 0.5)
    print(f"{name}: {inside.sum()} pixels inside, worst |mean - 0.5| {dev.max():.4f}, worst in sigma {np.max(dev / np.maximum(se[inside], 1e-12)):.2f}, "
          f"darkest {mean[inside].min():.4f}")
    assert (dev <= 4.0 * se[inside] + 1e-6).all(), (name, np.flatnonzero(dev > 4.0 * se[inside] + 1e-6)[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 6. area lights: closed forms
# ---------------------------------------------------------------------------------------------------------------------
N_LI = 65_536
RHO, LE = 0.6, 5.0


def floor_quad(half, y=0.0):
    """Matte floor in the plane y = const whose geometric normal points to +y."""
    pos = np.array([[-half, y, -half], [-half, y, half], [half, y, half], [half, y, -half]], dtype=np.float32)
    return dict(positions=pos, indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), tri_material=np.zeros(2, dtype=np.int32),
                tri_light=np.full(2, -1, dtype=np.int32))


def li_mean(hip_ctx, sc, o, d, **kw):
    g = pbrt_hip.Scene(hip_ctx, sc)
    rays = np.repeat(as_rays(np.float32([o]), np.float32([d])), N_LI)
    rgb, _ = g.li(rays, np.arange(N_LI, dtype=np.uint64) + 77, **kw)
    g.close()
    v = rgb[:, 0].astype(np.float64)
    return v.mean(), v.std(ddof=1) / np.sqrt(N_LI)


@pytest.mark.parametrize("ratio", [1.0, 0.25])
@pytest.mark.parametrize("placed", ["axis", "rotated"])
def test_disk_light_closed_form(hip_ctx, ratio, placed):
    h = 1.2
    R = ratio * h
    # the disk's own normal is +z: turned to face down (-y) over the floor point p0; "rotated" also spins it about its axis
    # and moves the whole arrangement away from the origin
    p0 = np.array([0.0, 0.0, 0.0]) if placed == "axis" else np.array([0.3, 0.0, -0.2])
    spin = np.eye(4) if placed == "axis" else rot((0, 0, 1), 63.0)
    to_world = translate(p0[0], h, p0[2]) @ rot((1, 0, 0), 90.0) @ spin
    assert np.allclose(to_world[:3, :3] @ [0, 0, 1], [0, -1, 0])
    mats = scenes._materials([(scenes.MAT_MATTE, (RHO, RHO, RHO), (0, 0, 0), 1.0), (scenes.MAT_NONE, (0, 0, 0), (0, 0, 0), 1.0)])
    expect = qm.disk_light_floor_radiance(RHO, LE, R, h)
    eye = p0 + np.array([0.4, 0.9, 0.3])
    for reverse in (False, True):
        rec = scenes.disk(0.0, R, to_world=to_world, material=0, light=0, reverse_orientation=reverse)
        sc = shape_scene([rec], materials=mats, lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 2, 0, 1)], extra=floor_quad(20.0))
        mean, se = li_mean(hip_ctx, sc, eye, p0 - eye, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=2, light_strategy=1)
        print(f"disk light R/h {ratio} {placed} reverse {reverse}: {mean:.5f} +- {se:.5f}, closed form {expect:.5f}")
        if reverse:
            assert mean == 0.0  # a one-sided light facing away contributes exactly nothing
        else:
            assert abs(mean - expect) <= 4.0 * se


def test_cylinder_light_closed_form(hip_ctx):
    R, H = 0.8, 1.1
    # the cylinder emits inward (two_sided), its axis along world y; a small matte disk at its centre faces +y along the axis
    axis_up = rot((1, 0, 0), -90.0)  # object +z -> world +y
    assert np.allclose(axis_up[:3, :3] @ [0, 0, 1], [0, 1, 0])
    move = translate(0.2, -0.1, 0.3)
    mats = scenes._materials([(scenes.MAT_MATTE, (RHO, RHO, RHO), (0, 0, 0), 1.0), (scenes.MAT_NONE, (0, 0, 0), (0, 0, 0), 1.0)])
    recs = [scenes.cylinder(R, -H, H, to_world=move @ axis_up @ rot((0, 0, 1), 20.0), material=1, light=0),
            scenes.disk(0.0, 0.05, to_world=move @ axis_up @ translate(0.02, 0.01, 0.0), material=0)]  # (off centre: the ray must not
                                                                                                  # meet the disk where r = 0)
    sc = shape_scene(recs, materials=mats, lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 1, 1, 1)])
    expect = qm.cylinder_light_centre_radiance(RHO, LE, R, H)
    centre = move[:3, 3]
    eye = centre + np.array([0.1, 0.5, 0.15])  # inside the cylinder, above the patch
    est = {}
    for name, kw in (("path", dict(integrator=pbrt_hip.INTEGRATOR_PATH, max_depth=1, light_strategy=1)),
                     ("direct", dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=2, light_strategy=1))):
        est[name] = li_mean(hip_ctx, sc, eye, centre - eye, **kw)
        print(f"cylinder light, {name}: {est[name][0]:.5f} +- {est[name][1]:.5f}, closed form {expect:.5f}")
        assert abs(est[name][0] - expect) <= 4.0 * est[name][1], name
    assert abs(est["path"][0] - est["direct"][0]) <= 4.0 * np.hypot(est["path"][1], est["direct"][1])


EMITTER_MATS = [(scenes.MAT_MATTE, (RHO, RHO, RHO), (0, 0, 0), 1.0), (scenes.MAT_NONE, (0, 0, 0), (0, 0, 0), 1.0)]  # 0: floor / patch, 1: emitter
ESTIMATORS = {
    "direct-all": dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=2, light_strategy=0),
    "direct-one": dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=2, light_strategy=1),
    "path": dict(integrator=pbrt_hip.INTEGRATOR_PATH, max_depth=1, light_strategy=1),
}


@pytest.mark.parametrize("phi_max", [200.0, 90.0])
def test_partial_cylinder_light_closed_form(hip_ctx, phi_max):
    """test_cylinder_light_closed_form with the cylinder cut to a sweep: Cylinder::sample draws phi in [0, phi_max] and the
    area counts the same part, so the sector's share of the full cylinder's irradiance arrives (the patch's cosine does not
    depend on the azimuth)."""
    R, H = 0.8, 1.1
    axis_up = rot((1, 0, 0), -90.0)  # object +z -> world +y
    move = translate(0.2, -0.1, 0.3)
    recs = [scenes.cylinder(R, -H, H, phi_max=phi_max, to_world=move @ axis_up @ rot((0, 0, 1), 20.0), material=1, light=0),
            scenes.disk(0.0, 0.05, to_world=move @ axis_up @ translate(0.02, 0.01, 0.0), material=0)]
    sc = shape_scene(recs, materials=scenes._materials(EMITTER_MATS), lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 1, 1, 1)])
    expect = qm.partial_cylinder_light_centre_radiance(RHO, LE, R, H, np.radians(phi_max))
    centre = move[:3, 3]
    eye = centre + np.array([0.1, 0.5, 0.15])
    est = {}
    for name in ("path", "direct-one"):
        est[name] = li_mean(hip_ctx, sc, eye, centre - eye, **ESTIMATORS[name])
        print(f"cylinder light phi_max {phi_max}, {name}: {est[name][0]:.5f} +- {est[name][1]:.5f}, closed form {expect:.5f}")
        assert abs(est[name][0] - expect) <= 4.0 * est[name][1], name
    assert abs(est["path"][0] - est["direct-one"][0]) <= 4.0 * np.hypot(est["path"][1], est["direct-one"][1])


@pytest.mark.parametrize("ratio", [0.5, 0.1, 0.02])
def test_rotated_sphere_light_closed_form(hip_ctx, ratio):
    """A full sphere light under a rotation and a translation (Sphere::sample2's cone about object_to_world * (0, 0, 0)) above
    a floor point: Lo = rho L (R / d)^2. R / d = 0.02 takes the small-angle branch of the cone sampling (sin^2(theta_max) =
    0.0004 < 0.00068523; at 0.1 it is 0.01, still the general branch). That branch is pbrt's approximation and float32's limit,
    not an exact estimator: it draws sin^2(theta) uniformly (off the uniform cone by O(sin^2(theta_max))) and its pdf divides by
    1 - cos(theta_max) = 2e-4, formed from a float32 next to 1 (cos(theta_max) carries up to 1.5 * 2^-24: the rounding of
    1 - sin^2 halved by the root, and the root's own). Allowed there, beside 4 se: (sin^2(theta_max) + 1.5 * 2^-24 /
    (1 - cos(theta_max))) of the value, 8.5e-4 of it; a wrong centre or radius is off by a multiple of the value."""
    d = 1.5
    p0 = np.array([0.3, 0.0, -0.2])
    eye = p0 + np.array([0.8, 0.5, 0.4])
    R = ratio * d
    rec = scenes.sphere_shape(R, to_world=translate(p0[0], d, p0[2]) @ rot((1, 2, 3), 40.0), material=1, light=0)
    sc = shape_scene([rec], materials=scenes._materials(EMITTER_MATS), lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 2, 0, 1)],
                     extra=floor_quad(20.0))
    expect = qm.sphere_light_floor_radiance(RHO, LE, R, d)
    rounding = (ratio ** 2 + 1.5 * 2.0 ** -24 / (1.0 - np.sqrt(1.0 - ratio ** 2))) * expect if ratio == 0.02 else 0.0
    est = {}
    for name in ESTIMATORS:
        est[name] = li_mean(hip_ctx, sc, eye, p0 - eye, **ESTIMATORS[name])
        print(f"sphere light R/d {ratio}, {name}: {est[name][0]:.7f} +- {est[name][1]:.7f}, closed form {expect:.7f}")
        assert abs(est[name][0] - expect) <= 4.0 * est[name][1] + rounding, name
    assert abs(est["path"][0] - est["direct-one"][0]) <= 4.0 * np.hypot(est["path"][1], est["direct-one"][1]) + rounding


@pytest.mark.parametrize("reverse", [False, True], ids=["as-made", "reversed"])
def test_mirrored_one_sided_sphere_light(hip_ctx, reverse):
    """The sphere's cone sampling orients its normal by itself: under a mirror that keeps lengths the normal points inward
    (the light is dark from outside, exactly) unless reverse_orientation turns it outward again (the closed form)."""
    d, ratio = 1.5, 0.5
    p0 = np.array([0.3, 0.0, -0.2])
    eye = p0 + np.array([0.8, 0.5, 0.4])
    rec = scenes.sphere_shape(ratio * d, to_world=translate(p0[0], d, p0[2]) @ rot((1, 2, 3), 40.0) @ scale(1.0, -1.0, 1.0), material=1, light=0,
                              reverse_orientation=reverse)
    n = qm.intersect(qm.from_record(rec[0]), p0[None, :], np.array([[0.0, 1.0, 0.0]]))["n"][0]
    assert (n[1] < 0.0) == reverse  # outward at the sphere's lowest point is -y
    sc = shape_scene([rec], materials=scenes._materials(EMITTER_MATS), lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 2, 0, 1)],
                     extra=floor_quad(20.0))
    expect = qm.sphere_light_floor_radiance(RHO, LE, ratio * d, d) if reverse else 0.0
    for name in ESTIMATORS:
        mean, se = li_mean(hip_ctx, sc, eye, p0 - eye, **ESTIMATORS[name])
        print(f"mirrored sphere light reverse {reverse}, {name}: {mean:.6f} +- {se:.6f}, closed form {expect:.6f}")
        if reverse:
            assert abs(mean - expect) <= 4.0 * se, (name, mean, se, expect)
        else:
            assert mean == 0.0, (name, mean)


@pytest.mark.parametrize("reverse", [False, True], ids=["as-made", "reversed"])
def test_mirrored_one_sided_disk_light_closed_form(hip_ctx, reverse):
    """test_disk_light_closed_form under a mirror that keeps lengths. The emitting side is the normal's of
    test_one_sided_light_emits_to_the_normals_side (the model's: flipped by reverse_orientation ^ swaps_handedness): turned to
    the floor, light sampling and BSDF sampling must both see it emit (the closed form, by every estimator); turned away,
    neither may (exactly 0)."""
    h = R = 1.2
    p0 = np.array([0.3, 0.0, -0.2])
    eye = p0 + np.array([0.4, 0.9, 0.3])
    expect = qm.disk_light_floor_radiance(RHO, LE, R, h)
    seen = set()
    for turn in (90.0, -90.0):  # object +z to world -y, to world +y
        to_world = translate(p0[0], h, p0[2]) @ rot((1, 0, 0), turn) @ rot((0, 0, 1), 63.0) @ scale(1.0, -1.0, 1.0)
        rec = scenes.disk(0.0, R, to_world=to_world, material=1, light=0, reverse_orientation=reverse)
        n = qm.intersect(qm.from_record(rec[0]), p0[None, :], np.array([[0.0, 1.0, 0.0]]))["n"][0]
        assert abs(abs(n[1]) - 1.0) < 1e-6
        facing = n[1] < 0.0
        seen.add(facing)
        sc = shape_scene([rec], materials=scenes._materials(EMITTER_MATS), lights=[(scenes.LIGHT_DIFFUSE_AREA, (LE, LE, LE), 2, 0, 1)],
                         extra=floor_quad(20.0))
        for name in ESTIMATORS:
            mean, se = li_mean(hip_ctx, sc, eye, p0 - eye, **ESTIMATORS[name])
            print(f"mirrored disk light reverse {reverse} {'facing' if facing else 'facing away'}, {name}: {mean:.5f} +- {se:.5f}, "
                  f"closed form {expect if facing else 0.0:.5f}")
            if facing:
                assert abs(mean - expect) <= 4.0 * se, (name, mean, se, expect)
            else:
                assert mean == 0.0, (name, mean)
    assert seen == {True, False}


# ---------------------------------------------------------------------------------------------------------------------
# 7. creation errors
# ---------------------------------------------------------------------------------------------------------------------
def test_creation_refusals_leave_the_context_usable(hip_ctx):
    def bad(**changes):
        rec = scenes.cylinder(0.5, -0.5, 0.5) if changes.pop("_cyl", False) else scenes.disk(0.0, 0.5, 0.1)
        if changes.pop("_sphere", False):
            rec = scenes.sphere_shape(0.5, **changes.pop("_args"))
        for k, v in changes.items():
            rec[k] = v
        return rec

    area = [(scenes.LIGHT_DIFFUSE_AREA, (1.0, 1.0, 1.0), 1, 0, 1)]
    cases = {
        "zero radius": (bad(radius=0.0), ()),
        "negative radius": (bad(radius=-1.0), ()),
        "inner radius at the radius": (bad(inner_radius=0.5), ()),
        "negative inner radius": (bad(inner_radius=-0.1), ()),
        "flat cylinder": (bad(_cyl=True, z_min=0.25, z_max=0.25), ()),
        "zero sweep": (bad(phi_max=0.0), ()),
        "negative sweep": (bad(_cyl=True, phi_max=-90.0), ()),
        "material out of range": (bad(material=1), ()),
        "negative material": (bad(material=-1), ()),
        "light out of range": (bad(light=0), ()),
        "unknown type": (bad(type=3), ()),
        "sphere short in z with a light": (bad(_sphere=True, _args=dict(z_max=0.3, light=0)), area),
        "sphere short in phi with a light": (bad(_sphere=True, _args=dict(phi_max=270.0, light=0)), area),
        # Disk::sample covers the full disk (D87); Shape::area is the object-space area (D86)
        "annulus with a light": (bad(light=0), area),
        "disk sector with a light": (bad(inner_radius=0.0, phi_max=270.0, light=0), area),
        "scaled sphere with a light": (bad(_sphere=True, _args=dict(to_world=scale(2.0, 2.0, 2.0), light=0)), area),
        "stretched sphere with a light": (bad(_sphere=True, _args=dict(to_world=rot((1, 2, 3), 40.0) @ scale(1.0, 1.0, 1.01), light=0)), area),
        "sheared sphere with a light": (bad(_sphere=True, _args=dict(to_world=np.array([[1, 0.01, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]), light=0)), area),
    }
    says = {"annulus with a light": "partial disk", "disk sector with a light": "partial disk", "scaled sphere with a light": "scales or shears",
            "stretched sphere with a light": "scales or shears", "sheared sphere with a light": "scales or shears"}
    # the tree over a good record's bounds, so that every record reaches the creation call itself (the binding's own bounds call
    # refuses an unknown type before that)
    tri = FAR_TRIANGLE["positions"][FAR_TRIANGLE["indices"]]
    lo, hi = pbrt_hip.shape_world_bounds(scenes.disk(0.0, 0.5))
    tree = pbrt_hip.bvh_build_boxes(np.concatenate([tri.min(axis=1), lo]), np.concatenate([tri.max(axis=1), hi]))
    for name, (rec, lights) in cases.items():
        with pytest.raises(pbrt_hip.PbrtHipError) as e:
            pbrt_hip.Scene(hip_ctx, shape_scene([rec], lights=lights), bvh=tree)
        msg = str(e.value)
        assert "pbrt_hip_scene_create_with_shapes" in msg and len(msg.split(":", 1)[-1].strip()) > 0, (name, msg)
        assert says.get(name, "") in msg, (name, msg)
        assert not hip_ctx.is_lost(), name
    with pytest.raises(pbrt_hip.PbrtHipError):  # "spheres" and "shapes" in one scene
        pbrt_hip.Scene(hip_ctx, dict(shape_scene([scenes.disk(0.0, 0.5)]), spheres=np.array([[0, 0, 0, 1.0, 0, -1, 0, 0]], dtype=np.float32)))
    # the same shapes without the light are good, and so is a light under a mirror that keeps lengths
    for name in says:
        rec = cases[name][0].copy()
        rec["light"] = -1
        pbrt_hip.Scene(hip_ctx, shape_scene([rec])).close()
    pbrt_hip.Scene(hip_ctx, shape_scene([scenes.sphere_shape(0.5, to_world=ORTHONORMAL_MIRROR, light=0)], lights=area)).close()
    # the same context still creates and traces a good scene, and the other limits are reported
    g = pbrt_hip.Scene(hip_ctx, shape_scene([scenes.sphere_shape(0.5, light=0)], lights=area))
    hit = g.intersect(as_rays(np.float32([[0, 0, 3]]), np.float32([[0, 0, -1]])))
    assert hit["prim_id"][0] == 1 and abs(hit["t"][0] - 2.5) <= T_TOL * 2.5
    hip_ctx.set_traversal(pbrt_hip.TRAVERSAL_STACKLESS)
    try:
        with pytest.raises(pbrt_hip.PbrtHipError):
            g.intersect(as_rays(np.float32([[0, 0, 3]]), np.float32([[0, 0, -1]])))
    finally:
        hip_ctx.set_traversal(pbrt_hip.TRAVERSAL_AUTO)
    g.close()
