"""The float64 quadric model against itself, pbrt_hip_shape_world_bounds against the model and against the float32
corner-transform union, the share of rays the GPU tests' generator puts next to a decision boundary (of the hit test and of
the Lambert probe's shadow rays), and the area lights' closed forms against a quadrature. No GPU."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import quadric_model as qm


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


TRANSFORMS = {
    "identity": np.eye(4),
    "rigid": translate(0.2, -0.1, 0.15) @ rot((1, 2, 3), 40.0),
    "scaled": translate(-0.1, 0.1, 0.0) @ rot((0, 1, 1), 25.0) @ scale(1.0, 0.6, 1.4),
    "mirrored": translate(0.1, 0.0, -0.1) @ rot((1, 0, 1), 70.0) @ scale(1.0, -0.8, 1.1),
}

# a mirror that neither scales nor shears (TRANSFORMS["mirrored"] also scales): swaps handedness, keeps lengths and areas
ORTHONORMAL_MIRROR = translate(0.15, -0.1, 0.2) @ rot((2, 1, -1), 65.0) @ scale(1.0, -1.0, 1.0)
# the Lambert probe's light axes: a generic rotation keeps every light off every object axis of every transform above
PROBE_AXES = rot((3, -1, 2), 57.0)[:3, :3]
PROBE_RAYS = (20_000, 23)  # qm.rays_at_unit_cube(*PROBE_RAYS)


def shape_records():
    """The shapes of the GPU tests: every type, radius in [0.3, 1], phi_max in {360, 270, 135}, mixed z ranges, inner radius 0 / 0.4 r."""
    recs = []
    for name, m in TRANSFORMS.items():
        for phi in (360.0, 270.0, 135.0):
            recs.append((f"sphere-{name}-{phi:g}", scenes.sphere_shape(0.8, -0.8 if phi == 360.0 else -0.5, 0.8 if phi != 135.0 else 0.3, phi, m)))
            recs.append((f"cylinder-{name}-{phi:g}", scenes.cylinder(0.5 if phi != 270.0 else 0.3, -0.6, 0.7 if phi != 135.0 else 0.2, phi, m)))
            recs.append((f"disk-{name}-{phi:g}", scenes.disk(0.1, 1.0 if phi == 360.0 else 0.7, 0.0 if phi != 270.0 else 0.28, phi, m)))
    return recs


RECORDS = shape_records()


@pytest.mark.parametrize("name,rec", RECORDS[:9] + RECORDS[18:27], ids=[r[0] for r in RECORDS[:9] + RECORDS[18:27]])
def test_hit_points_satisfy_the_implicit_equations(name, rec):
    s = qm.from_record(rec[0])
    o, d = qm.rays_at_unit_cube(4000, 11)
    r = qm.intersect(s, o, d)
    assert r["hit"].sum() > 50
    p = r["p"][r["hit"]]
    assert np.abs(qm.implicit_residual(s, p)).max() < 1e-12
    # the object-space point is where the ray is at t
    w2o = np.linalg.inv(s["o2w"])
    oo = o.astype(np.float64) @ w2o[:3, :3].T + w2o[:3, 3]
    dd = d.astype(np.float64) @ w2o[:3, :3].T
    along = oo[r["hit"]] + dd[r["hit"]] * r["t"][r["hit"]][:, None]
    assert np.abs(along - p).max() < 1e-9
    # inside the cut: z range, sweep, radii
    assert (r["phi"][r["hit"]] <= s["phi_max"] + 1e-12).all()
    assert (p[:, 2] >= s["z_min"] - 1e-12).all() and (p[:, 2] <= s["z_max"] + 1e-12).all()
    # unit normal, perpendicular to the surface: against a finite difference of the parametrisation through the transform
    n = r["n"][r["hit"]]
    assert np.abs(np.sqrt((n ** 2).sum(axis=1)) - 1.0).max() < 1e-12


@pytest.mark.parametrize("name,rec", RECORDS, ids=[r[0] for r in RECORDS])
def test_tangent_frame_against_the_parametrisation(name, rec):
    """surface_frame at the hits of the GPU tests' rays, held by finite differences of surface_points through o2w (partial
    sweeps, mirrored and scaled transforms included), not by its own formula: ss is parallel to dp/du and points the same way;
    ss is perpendicular to ns; (ss, ts, ns) is right-handed, det = +1, under every transform, because ts = ns x ss makes it so
    whatever the matrix's determinant. What the handedness swap and reverse_orientation change is the normal: ns = +(dp/du x
    dp/dv) / |...| of the world-space surface unless reverse_orientation is set, the mirror or not (pbrt-v3 flips n by
    reverse ^ swaps, and the world-space cross product itself turns over under a mirror), so ts points along the part of dp/dv
    perpendicular to ss, or against it when reversed. The anisotropic lobes cannot see that sign: Trowbridge-Reitz D and Lambda
    read cos^2 phi and sin^2 phi of the local directions alone, which are even in the ts component."""
    s = qm.from_record(rec[0])
    o, d = qm.rays_at_unit_cube(4000, 11)
    r = qm.intersect(s, o, d)
    hit = r["hit"]
    assert hit.sum() > 50
    fr = qm.surface_frame(s, r)
    ss, ts, ns = fr["ss"][hit], fr["ts"][hit], fr["ns"][hit]
    # the parameters of the hit points, by inverting the parametrisation
    p = r["p"][hit]
    u = r["phi"][hit] / s["phi_max"]
    if s["type"] == "disk":
        v = (np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - s["inner_radius"]) / (s["radius"] - s["inner_radius"])
    else:
        v = (p[:, 2] - s["z_min"]) / (s["z_max"] - s["z_min"])
    assert np.abs(qm.surface_points(s, u, v) - p).max() < 1e-9
    h = 1e-6
    lin = s["o2w"][:3, :3]
    du = (qm.surface_points(s, u + h, v) - qm.surface_points(s, u - h, v)) / (2 * h) @ lin.T
    dv = (qm.surface_points(s, u, v + h) - qm.surface_points(s, u, v - h)) / (2 * h) @ lin.T
    du_len = np.sqrt((du ** 2).sum(axis=1))
    assert np.abs(np.cross(ss, du / du_len[:, None])).max() < 1e-8 and ((ss * du).sum(axis=1) > 0.0).all()
    assert np.abs(fr["dpdu"][hit] - du).max() < 1e-8 * max(1.0, du_len.max())  # and its length: phi_max is in it
    assert np.abs((ss * ns).sum(axis=1)).max() < 1e-12
    assert np.abs(np.sqrt((ss ** 2).sum(axis=1)) - 1.0).max() < 1e-12 and np.abs(np.sqrt((ts ** 2).sum(axis=1)) - 1.0).max() < 1e-12
    assert np.abs(np.linalg.det(np.stack([ss, ts, ns], axis=1)) - 1.0).max() < 1e-12
    cross = np.cross(du, dv)
    sign = -1.0 if s["reverse"] else 1.0
    if s["type"] == "disk":
        sign = -sign  # surface_points runs the disk's v from the inner radius outward, Disk::intersect's from the radius inward
    assert (sign * (ns * cross).sum(axis=1) > 0.0).all() and (sign * (ts * dv).sum(axis=1) > 0.0).all()
    # to_local: the coordinates rebuild the vector
    w = np.random.default_rng(3).normal(size=ss.shape)
    l = qm.to_local(dict(ss=ss, ts=ts, ns=ns), w)
    assert np.abs(l[:, :1] * ss + l[:, 1:2] * ts + l[:, 2:] * ns - w).max() < 1e-12


def test_reversed_orientation_turns_the_frame_over():
    for name in ("rigid", "mirrored"):
        a, b = (qm.from_record(scenes.cylinder(0.5, -0.6, 0.7, 270.0, TRANSFORMS[name], reverse_orientation=rev)[0]) for rev in (False, True))
        o, d = qm.rays_at_unit_cube(2000, 11)
        ra, rb = qm.intersect(a, o, d), qm.intersect(b, o, d)
        hit = ra["hit"]
        fa, fb = qm.surface_frame(a, ra), qm.surface_frame(b, rb)
        assert hit.sum() > 50 and np.array_equal(hit, rb["hit"])
        assert np.array_equal(fa["ss"][hit], fb["ss"][hit]) and np.array_equal(fa["ns"][hit], -fb["ns"][hit]) and np.array_equal(fa["ts"][hit], -fb["ts"][hit])


@pytest.mark.parametrize("name", ["identity", "scaled"])
def test_a_ray_down_the_disks_axis_hits_the_centre(name):
    """intersect's contract for the axis ray: a hit at the centre from either side, not `near`, a finite frame whose tangent is
    the one of phi = 0 (the direction of M e_y), the limit of the points (x, 0) with x -> 0+"""
    s = qm.from_record(scenes.disk(0.1, 1.0, to_world=TRANSFORMS[name])[0])
    m = s["o2w"]  # the record's: rounded to float32
    centre, axis = m[:3, :3] @ [0.0, 0.0, s["z_min"]] + m[:3, 3], m[:3, :3] @ [0.0, 0.0, 1.0]
    o = np.stack([centre + 2.0 * axis, centre - 2.0 * axis])
    r = qm.intersect(s, o, np.stack([-axis, axis]))
    assert r["hit"].all() and not r["near"].any()
    assert (r["p"] == [0.0, 0.0, s["z_min"]]).all() and np.abs(r["t"] - 2.0).max() < 1e-7  # (the record's height is a float32)
    fr = qm.surface_frame(s, r)
    assert np.isfinite(fr["ss"]).all() and np.isfinite(fr["ts"]).all()
    e_y = m[:3, :3] @ [0.0, 1.0, 0.0]
    assert np.abs(fr["ss"] - e_y / np.linalg.norm(e_y)).max() < 1e-12
    beside = qm.intersect(s, o + m[:3, :3] @ [1e-7, 0.0, 0.0], np.stack([-axis, axis]))
    assert np.abs(qm.surface_frame(s, beside)["ss"] - fr["ss"]).max() < 1e-8  # (1e-16 of rounding over the 1e-7 of offset)
    # with a hole there is no centre to hit
    assert not qm.intersect(qm.from_record(scenes.disk(0.1, 1.0, 0.2, to_world=m)[0]), o, np.stack([-axis, axis]))["hit"].any()


def test_bsdf_quadrature_and_its_error_estimate():
    """bsdf_patch_radiance_by_quadrature with the Lambertian f is the closed form of the disk light, its halving estimate
    bounds its error (the midpoint rule's error falls by 4 under halved cells: a third of the difference is left), and a
    cosine-power lobe about the mirror direction agrees with itself at twice the cells within the estimate."""
    rho, L, h, R = 0.6, 5.0, 1.2, 1.2
    m = translate(0.3, h, -0.2) @ rot((1, 0, 0), 90.0) @ rot((0, 0, 1), 63.0)
    disk = qm.make("disk", R, 0.0, 0.0, o2w=m)
    p0, fr = np.array([0.3, 0.0, -0.2]), qm.frame_about([0.0, 1.0, 0.0])
    value, err = qm.bsdf_patch_radiance_by_quadrature(disk, p0, fr, [0.3, 0.8, 0.1], lambda wo, wi: np.full(len(wi), rho / np.pi), L, cells=200)
    closed = qm.disk_light_floor_radiance(rho, L, R, h)
    assert 0.0 < err < 1e-3 * closed and abs(value - closed) <= err
    assert value == pytest.approx(qm.patch_radiance_by_quadrature(disk, p0, [0.0, 1.0, 0.0], rho, L, cells=200), rel=1e-12)

    def lobe(wo, wi):
        mirror = wo * np.array([-1.0, -1.0, 1.0])
        return np.stack([np.maximum((mirror * wi).sum(axis=1), 0.0) ** 40] * 3, axis=1) * np.array([1.0, 0.5, 0.25])
    wo = np.array([0.2, 0.9, -0.1]) / np.linalg.norm([0.2, 0.9, -0.1])
    coarse, e_coarse = qm.bsdf_patch_radiance_by_quadrature(disk, p0, fr, wo, lobe, L, cells=100)
    fine, e_fine = qm.bsdf_patch_radiance_by_quadrature(disk, p0, fr, wo, lobe, L, cells=400)
    assert coarse.shape == (3,) and (fine > 0.0).all() and (e_fine < e_coarse).all()
    assert (np.abs(coarse - fine) <= e_coarse).all()


@pytest.mark.parametrize("kind", ["sphere", "disk", "cylinder"])
def test_area_matches_a_quadrature(kind):
    s = {"sphere": qm.make("sphere", 0.7, -0.4, 0.6, phi_max_deg=270.0),
         "disk": qm.make("disk", 0.9, 0.2, 0.2, inner_radius=0.3, phi_max_deg=135.0),
         "cylinder": qm.make("cylinder", 0.4, -0.3, 0.9, phi_max_deg=200.0)}[kind]
    n = 400
    u = (np.arange(n) + 0.5) / n
    uu, vv = np.meshgrid(u, u, indexing="ij")
    h = 1e-6
    p = qm.surface_points(s, uu, vv)
    du = (qm.surface_points(s, uu + h, vv) - qm.surface_points(s, uu - h, vv)) / (2 * h)
    dv = (qm.surface_points(s, uu, vv + h) - qm.surface_points(s, uu, vv - h)) / (2 * h)
    quad = np.sqrt((np.cross(du, dv) ** 2).sum(axis=-1)).mean()
    assert np.abs(qm.implicit_residual(s, p)).max() < 1e-12
    assert abs(quad - qm.area(s)) <= 2e-5 * qm.area(s)  # midpoint rule on 400 x 400 cells of a smooth integrand


def float32_corner_union(rec):
    """object_to_world * object_bound() as Transform * Bounds3 does it, every operation rounded to float32 in its order."""
    f = np.float32
    s = qm.from_record(rec)
    lo, hi = (np.asarray(v, dtype=np.float32) for v in qm.object_bound(s))
    m = np.asarray(rec["to_world"], dtype=np.float32).reshape(4, 4)
    mn, mx = np.full(3, np.inf, dtype=np.float32), np.full(3, -np.inf, dtype=np.float32)
    for c in range(8):
        x, y, z = (hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]
        for k in range(3):
            p = f(f(f(f(m[k, 0] * x) + f(m[k, 1] * y)) + f(m[k, 2] * z)) + m[k, 3])
            mn[k], mx[k] = min(mn[k], p), max(mx[k], p)
    return mn, mx


def test_shape_world_bounds_against_the_model_and_bit_for_bit():
    recs = np.concatenate([r[1] for r in RECORDS])
    lo, hi = pbrt_hip.shape_world_bounds(recs)
    assert lo.shape == (len(recs), 3) and lo.dtype == np.float32
    for i in range(len(recs)):
        s = qm.from_record(recs[i])
        mlo, mhi = qm.world_bounds(s)
        # contains the model's bound up to the rounding of three products and three sums in float32: gamma(6) of the terms' magnitude
        m = np.abs(s["o2w"][:3, :3]) @ np.maximum(np.abs(qm.object_bound(s)[0]), np.abs(qm.object_bound(s)[1])) + np.abs(s["o2w"][:3, 3])
        slack = 6 * 2.0 ** -24 * m
        assert (lo[i] <= mlo + slack).all() and (hi[i] >= mhi - slack).all(), RECORDS[i][0]
        # every surface point of the model lies inside
        u = np.linspace(0.0, 1.0, 41)
        pts = qm.surface_points(s, *np.meshgrid(u, u, indexing="ij")).reshape(-1, 3) @ s["o2w"][:3, :3].T + s["o2w"][:3, 3]
        assert (pts >= lo[i] - slack).all() and (pts <= hi[i] + slack).all(), RECORDS[i][0]
        flo, fhi = float32_corner_union(recs[i])
        assert lo[i].tobytes() == flo.tobytes() and hi[i].tobytes() == fhi.tobytes(), RECORDS[i][0]


def test_shape_world_bounds_rejects_bad_arguments():
    L = pbrt_hip.lib()
    assert L.pbrt_hip_shape_world_bounds(None, 0, None) == 0
    assert L.pbrt_hip_shape_world_bounds(None, 1, None) != 0
    bad = scenes.disk(0.0, 1.0)
    bad["type"] = 7
    out = np.zeros(6, dtype=np.float32)
    assert L.pbrt_hip_shape_world_bounds(bad.ctypes.data, 1, out.ctypes.data) != 0


def test_helpers_round_the_float64_inverse_once():
    rec = scenes.cylinder(0.5, -1.0, 1.0, to_world=TRANSFORMS["scaled"])[0]
    m = rec["to_world"].astype(np.float64).reshape(4, 4)
    inv = np.linalg.inv(m)
    inv[3] = (0, 0, 0, 1)
    assert rec["to_object"].tobytes() == inv.astype(np.float32).reshape(16).tobytes()
    assert scenes.SHAPE_DTYPE.itemsize == 176  # sizeof(PbrtShape)
    t = scenes.sphere_shape(0.5, to_world=translate(0.25, -1.5, 3.0))[0]
    assert (t["to_object"].reshape(4, 4)[:3, 3] == np.float32([-0.25, 1.5, -3.0])).all()  # translate(-c), exactly


@pytest.mark.parametrize("kind", ["sphere", "disk", "cylinder"])
def test_ray_generator_stays_within_the_near_cap(kind):
    """The GPU intersection test excludes rays flagged `near` and asserts that they are at most 1 % of the batch; here the
    same generator and shapes, with the model alone."""
    o, d = qm.rays_at_unit_cube(20000, 5)
    worst = 0.0
    for name, rec in RECORDS:
        if not name.startswith(kind):
            continue
        r = qm.intersect(qm.from_record(rec[0]), o, d)
        share = r["near"].mean()
        print(f"{name}: hits {r['hit'].mean():.3f} near {share:.5f}")
        worst = max(worst, share)
        assert r["hit"].mean() > 0.01
    assert worst <= 0.01


def probe_exclusion(probe):
    """(share of the batch the hit test flags near, share of the remaining hits whose shadow rays are not clear)."""
    comparable = probe["hit"] & ~probe["near"]
    return probe["near"].mean(), 1.0 - probe["keep"].sum() / comparable.sum()


@pytest.mark.parametrize("kind", ["sphere", "disk", "cylinder"])
def test_lambert_probe_stays_within_the_exclusion_cap(kind):
    """The GPU normal test compares hits that are not near and whose three shadow rays are clear (two offsets and the ray from
    the surface itself agree, none near), and asserts that the shadow rule excludes at most 1 % of the hits it could compare
    (and the hit test's near flag at most 1 % of the batch, as above); here the same rays, shapes and lights with the model
    alone. Measured: worst shadow-rule share 0.97 % (cylinder-mirrored-135; 0.89 % with the two offsets alone), fewest kept
    hits 1108 (disk-scaled-135); a shape that cannot shadow itself (disk) loses up to 0.49 % to the near flag of the
    offset ray's own start."""
    o, d = qm.rays_at_unit_cube(*PROBE_RAYS)
    worst_near = worst_shadow = 0.0
    fewest = len(o)
    for name, rec in RECORDS:
        if not name.startswith(kind):
            continue
        s = qm.from_record(rec[0])
        r = qm.lambert_probe(s, o, d, PROBE_AXES)
        near, shadow = probe_exclusion(r)
        k = r["keep"]
        print(f"{name}: hits {r['hit'].sum()} near {near:.5f} shadow rule excludes {shadow:.5f} kept {k.sum()} "
              f"with a shadowed channel {r['shadowed'][k].any(axis=1).mean():.3f}")
        worst_near, worst_shadow, fewest = max(worst_near, near), max(worst_shadow, shadow), min(fewest, k.sum())
        # what the model hands the GPU test: unit normals, values in [0, 1], 0 exactly where shadowed
        assert np.abs(np.sqrt((r["n"][k] ** 2).sum(axis=1)) - 1.0).max() < 1e-12
        assert (r["expect"][k] >= 0.0).all() and (r["expect"][k] <= 1.0).all() and (r["expect"][k][r["shadowed"][k]] == 0.0).all()
        lit = k & ~r["shadowed"].any(axis=1)
        assert np.abs((r["expect"][lit] ** 2).sum(axis=1) - 1.0).max() < 1e-12  # the axes are orthonormal
        if kind == "disk" or name.endswith("-360") and kind == "sphere":
            assert not r["shadowed"][k].any(), name  # flat or convex and seen from outside: nothing to shadow it
        elif not name.endswith("-360"):
            assert r["shadowed"][k].any(axis=1).sum() > 300, name  # open shapes do shadow themselves
    assert worst_near <= 0.01 and worst_shadow <= 0.01 and fewest >= 1000


def test_orthonormal_mirror_is_one():
    m = ORTHONORMAL_MIRROR[:3, :3]
    assert np.abs(m.T @ m - np.eye(3)).max() < 1e-15 and np.linalg.det(m) < 0.0
    assert np.abs(PROBE_AXES.T @ PROBE_AXES - np.eye(3)).max() < 1e-15
    for name, t in TRANSFORMS.items():  # no light along an object axis
        axes = t[:3, :3] / np.sqrt((t[:3, :3] ** 2).sum(axis=0))
        assert np.abs(axes.T @ PROBE_AXES).max() < 0.99, name


@pytest.mark.parametrize("phi_max_deg", [360.0, 200.0, 90.0])
def test_cylinder_light_closed_form_matches_a_quadrature(phi_max_deg):
    R, H, rho, L = 0.8, 1.1, 0.6, 5.0
    m = translate(0.2, -0.1, 0.3) @ rot((1, 0, 0), -90.0) @ rot((0, 0, 1), 20.0)
    s = qm.make("cylinder", R, -H, H, phi_max_deg=phi_max_deg, o2w=m)
    quad = qm.patch_radiance_by_quadrature(s, m[:3, 3], m[:3, :3] @ [0.0, 0.0, 1.0], rho, L)
    closed = qm.partial_cylinder_light_centre_radiance(rho, L, R, H, np.radians(phi_max_deg))
    assert abs(quad - closed) <= 2e-5 * closed
    if phi_max_deg == 360.0:
        assert closed == qm.cylinder_light_centre_radiance(rho, L, R, H)


def test_disk_annulus_and_sphere_light_closed_forms_match_a_quadrature():
    rho, L, h, R = 0.6, 5.0, 1.2, 1.2
    m = translate(0.3, h, -0.2) @ rot((1, 0, 0), 90.0) @ rot((0, 0, 1), 63.0)
    p0, up = [0.3, 0.0, -0.2], [0.0, 1.0, 0.0]
    quad = qm.patch_radiance_by_quadrature(qm.make("disk", R, 0.0, 0.0, o2w=m), p0, up, rho, L)
    assert abs(quad - qm.disk_light_floor_radiance(rho, L, R, h)) <= 2e-5 * quad
    quad = qm.patch_radiance_by_quadrature(qm.make("disk", R, 0.0, 0.0, inner_radius=0.5 * R, o2w=m), p0, up, rho, L)
    assert abs(quad - qm.annulus_light_floor_radiance(rho, L, R, 0.5 * R, h)) <= 2e-5 * quad
    # the sphere from outside: the quadrature sees both halves (two-sided, unshadowed), the floor only the near one, and the far
    # half subtends the same cone: twice the closed form
    for ratio in (0.5, 0.1):
        s = qm.make("sphere", ratio * h, -ratio * h, ratio * h, o2w=translate(0.3, h, -0.2) @ rot((1, 2, 3), 40.0))
        quad = qm.patch_radiance_by_quadrature(s, p0, up, rho, L)
        assert abs(0.5 * quad - qm.sphere_light_floor_radiance(rho, L, ratio * h, h)) <= 1e-4 * quad
