"""Cases shared by test_shape_material_model.py (the float64 models alone) and test_gpu_shape_materials.py (the device held to
them): glossy, specular and Disney rows on the quadric shapes. The rows with their BSDF models, the ray selections, the point-light
closed form on a shape through the model's tangent frame with its per-ray allowance and its wrong frames, the mirror under an
image environment map, the lossless glass sphere, the furnace on convex bodies and the shape lights seen by a narrow lobe."""
import numpy as np

from pbrt_hip import scenes
import bxdf_cases
import bxdf_model as bm
import disney_cases
import disney_model as dm
import envmap_model as em
import light_map_model as lmm
import microfacet_model as mm
import quadric_model as qm
from envmap_cases import _rot
from glossy_cases import ETA, K
from test_quadric_model import ORTHONORMAL_MIRROR, RECORDS, TRANSFORMS, rot, translate
from test_gpu_shapes import T_TOL, shape_scene

RTOL = 1e-4       # test_gpu_lobe_materials.py::test_point_light_closed_form: the same BSDF code on a plane, float32 against float64
MIN_KEPT = 150    # of N_RAYS
N_RAYS = 400
BATCH = (20_000, 41)  # qm.rays_at_unit_cube(*BATCH): the cases take their rays from it, in its order
MIN_COS = 0.1

# ---- the rows: strongly anisotropic, alphas set directly ----
KD, KS = (0.3, 0.2, 0.1), (0.5, 0.5, 0.5)
SUB_KD, SUB_KS = (0.5, 0.4, 0.3), (0.3, 0.3, 0.4)
DISNEY_DESC = scenes.disney((0.8, 0.5, 0.3), metallic=1.0, anisotropic=0.8, roughness=0.5)
AU, AV = 0.15, 0.6
# the glass row's index: a pair of directions across the surface has a transmission lobe only when the one in the thinner medium
# lies within cos theta > 1 / eta of the other's straight continuation (the generalised half vector must face both), so with eyes
# all round a shape eta = 1.5 leaves fewer than MIN_KEPT rays of N_RAYS on the cylinder's opposite-side cases, whatever the light
GLASS_POINT_ETA = 2.0
MATTE_ROW = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)


def _no_band(m, wo, wi):
    return np.zeros(len(wo), bool)


# name -> materials row 0, the descriptor set after creation (scene key, descriptor) or None, the set_material_roughness call or
# None, the model, its f, its discontinuity band, whether the lobe reads the tangent
ROWS = {
    "metal": dict(row=scenes.metal(ETA, K, 0.01), desc=None, roughness=(AU, AV, False),
                  model=mm.Material.metal(ETA, K, AU, AV, remap=False), f=mm.bsdf_f, band=_no_band, anisotropic=True),
    # pbrt_hip_scene_set_material_roughness refuses u != v on a plastic row (PlasticMaterial has one roughness): the row is
    # isotropic, reads no tangent, and is held to the closed form alone
    "plastic": dict(row=scenes.plastic(KD, KS, 0.1), desc=None, roughness=(0.3, 0.3, False),
                    model=mm.Material.plastic(KD, KS, 0.3, remap=False), f=mm.bsdf_f, band=_no_band, anisotropic=False),
    "substrate": dict(row=MATTE_ROW, desc=("material_descs", scenes.substrate(SUB_KD, SUB_KS, AU, AV, remap=False)), roughness=None,
                      model=bm.substrate(SUB_KD, SUB_KS, AU, AV, remap=False), f=bm.bsdf_f, band=bxdf_cases.in_band, anisotropic=True),
    "disney": dict(row=MATTE_ROW, desc=("disney_descs", DISNEY_DESC), roughness=None, model=dm.Disney(DISNEY_DESC), f=dm.bsdf_f,
                   band=disney_cases.in_band, anisotropic=True),
    "glass": dict(row=MATTE_ROW, desc=("material_descs", scenes.rough_glass(bxdf_cases.KR, bxdf_cases.KT, GLASS_POINT_ETA, AU, AV, remap=False)),
                  roughness=None, model=bm.rough_glass(bxdf_cases.KR, bxdf_cases.KT, GLASS_POINT_ETA, AU, AV, remap=False), f=bm.bsdf_f,
                  band=bxdf_cases.in_band, anisotropic=True),
}


def material_scene(rec, row, lights):
    """(scene dict, what to call on the created scene): the one shape with `row` as material 0 under `lights`"""
    sc = shape_scene([rec], materials=scenes._materials([row["row"]]), lights=lights)
    if row["desc"] is not None:
        sc[row["desc"][0]] = {0: row["desc"][1]}

    def after(scene):
        if row["roughness"] is not None:
            scene.set_material_roughness(0, *row["roughness"][:2], remap=row["roughness"][2])
    return sc, after


# ---- ray selections: computed from the model alone ----
_BATCH_CACHE = {}


def batch():
    if "rays" not in _BATCH_CACHE:
        _BATCH_CACHE["rays"] = qm.rays_at_unit_cube(*BATCH)
    return _BATCH_CACHE["rays"]


def outward(shape, m):
    """the model's normal turned to the side dpdu x dpdv names in object space (outward for a sphere or cylinder)"""
    return m["n"] * (-1.0 if shape["reverse"] != bool(qm.swaps_handedness(shape)) else 1.0)


def select_rays(shape, view="any", light=None, side=None, n=N_RAYS):
    """The first n rays of the batch that the model has hitting the shape; view "inside" / "outside": from the concave side (against the
    outward normal) / from the convex one; side "same" / "opposite": eye and the point `light` on the same side / on opposite sides of the surface."""
    o, d = batch()
    m = qm.intersect(shape, o, d)
    ok = m["hit"].copy()
    d64 = d.astype(np.float64)
    if view in ("inside", "outside"):
        ok &= ((outward(shape, m) * d64).sum(axis=1) > 0.0) == (view == "inside")
    if side is not None:
        to_light = np.asarray(light) - qm.world_point(shape, m["p"])
        same = (m["n"] * -d64).sum(axis=1) * (m["n"] * to_light).sum(axis=1) > 0.0
        ok &= same if side == "same" else ~same
    idx = np.flatnonzero(ok)[:n]
    assert len(idx) == n, (len(idx), n)
    return o[idx], d[idx]


# ---- 2.1 the point light ----
LIGHT_P = np.array([4.1, 2.9, -3.3])   # the first candidate: far from every shape
LIGHT_I = np.array([40.0, 60.0, 80.0])
FRAMES = ("right", "swapped", "object", "inverse_transpose")


def light_candidates(shape):
    """Where a case's point light may stand, every one generic (on no object axis of the shape's transform,
    test_point_lights_are_generic): LIGHT_P; then, given in object space and taken through o2w, 3 units out 17 degrees off the +z
    and the -z axis, 3 units out over the middle of the sweep and opposite it, and a point inside the body a fifth of the radius
    off the axis (it lights a concave side without the far wall between). A case takes the one that keeps most rays."""
    mid = 0.5 * shape["phi_max"]
    side = np.array([np.cos(mid), np.sin(mid), 0.2])
    unit = lambda v: np.asarray(v) / np.linalg.norm(v)  # noqa: E731
    z_mid = 0.5 * (shape["z_min"] + shape["z_max"])
    obj = [3.0 * unit([0.25, 0.15, 1.0]), 3.0 * unit([0.25, 0.15, -1.0]), 3.0 * unit(side), -3.0 * unit(side),
           np.array([0.2 * shape["radius"] * side[0], 0.2 * shape["radius"] * side[1], z_mid + 0.07])]
    return [LIGHT_P] + [qm.world_point(shape, q) for q in obj]


def frame_at(shape, p_obj, variant="right"):
    """qm.surface_frame at object-space points, or one of the frames a wrong make_surface_shape would give: `swapped` ss := ts;
    `object` ss from dpdu left in object space; `inverse_transpose` dpdu taken through (M^-1)^T. ts = ns x ss as make_frame."""
    fr = qm.surface_frame(shape, dict(p=p_obj, n=qm.normal_at(shape, p_obj)))
    if variant == "right":
        return fr
    lin = shape["o2w"][:3, :3]
    dpdu_obj = fr["dpdu"] @ np.linalg.inv(lin).T
    v = {"swapped": fr["ts"], "object": dpdu_obj, "inverse_transpose": dpdu_obj @ np.linalg.inv(lin)}[variant]
    ss = v / np.sqrt((v ** 2).sum(axis=1))[:, None]
    return dict(dpdu=v, ss=ss, ns=fr["ns"], ts=np.cross(fr["ns"], ss))


def frame_differs(shape, variant):
    """does the wrong frame differ from the right one under this shape's transform? (the records hold float32 matrices)"""
    lin = shape["o2w"][:3, :3]
    if variant == "object":
        return not np.allclose(lin, np.eye(3), atol=1e-6)
    if variant == "inverse_transpose":
        return not np.allclose(lin @ lin.T, np.eye(3), atol=1e-6)
    return True


def point_light_expectation(shape, row, light, o, d, t, variant="right"):
    """f(wo_l, wi_l) I |ns . wi| / r^2 at the points o + t d, with their local directions and the vector to the light"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    p_w = o + d * t[:, None]
    w2o = np.linalg.inv(shape["o2w"])
    p_obj = p_w @ w2o[:3, :3].T + w2o[:3, 3]
    fr = frame_at(shape, p_obj, variant)
    to_light = light - p_w
    r2 = (to_light ** 2).sum(axis=1)
    wi = to_light / np.sqrt(r2)[:, None]
    wo_l, wi_l = qm.to_local(fr, -d), qm.to_local(fr, wi)
    return row["f"](row["model"], wo_l, wi_l) * LIGHT_I * (np.abs(wi_l[:, 2]) / r2)[:, None], wo_l, wi_l, to_light


def point_light_case(shape, row, light, o, d, wrong_frames=True):
    """dict: ref (n, 3), allow (n, 3): the larger change of ref with the hit moved to t (1 +- T_TOL) plus RTOL |ref|, keep, and
    wrong[variant] (n, 3) for the wrong frames"""
    m = qm.intersect(shape, o, d)
    t = np.where(m["hit"], m["t"], 1.0)
    ref, wo_l, wi_l, to_light = point_light_expectation(shape, row, light, o, d, t)
    blocked, blocked_near = qm.occluded_from_surface(shape, m["p"], to_light, t_max=1.0)
    keep = m["hit"] & ~m["near"] & ~blocked & ~blocked_near
    keep &= (np.abs(wo_l[:, 2]) >= MIN_COS) & (np.abs(wi_l[:, 2]) >= MIN_COS)
    keep &= ~row["band"](row["model"], wo_l, wi_l)
    keep &= np.all(ref > 0.0, axis=1) & np.all(np.isfinite(ref), axis=1)
    if not wrong_frames:
        return dict(ref=ref, keep=keep)
    moved = [point_light_expectation(shape, row, light, o, d, t * (1.0 + s * T_TOL))[0] for s in (1.0, -1.0)]
    allow = np.maximum(np.abs(moved[0] - ref), np.abs(moved[1] - ref)) + RTOL * np.abs(ref)
    wrong = {v: point_light_expectation(shape, row, light, o, d, t, v)[0] for v in FRAMES[1:]}
    return dict(ref=ref, allow=allow, keep=keep, wrong=wrong)


def _named(name):
    return next(r[1] for r in RECORDS if r[0] == name)


# (id, record, row name, select_rays keywords)
POINT_CASES = []
for _kind in ("sphere", "cylinder", "disk"):
    for _t in TRANSFORMS:
        for _phi in (360, 135):
            for _row in ("metal", "plastic", "substrate", "disney"):
                # a full cylinder is as wide as it is long: a quarter of the batch's hits look through an open end at the inner
                # wall, which no light outside reaches and which hides a light inside from every other ray; one point light
                # lights less than half of a closed body, so those cases take their rays from outside (the inner wall is the
                # 135-degree cases' and the glass cases')
                _kw = dict(view="outside") if (_kind, _phi) == ("cylinder", 360) else dict()
                POINT_CASES.append((f"{_row}-{_kind}-{_t}-{_phi}", _named(f"{_kind}-{_t}-{_phi}"), _row, _kw))
for _t in TRANSFORMS:
    for _side in ("same", "opposite"):
        POINT_CASES.append((f"glass-disk-{_t}-{_side}", _named(f"disk-{_t}-360"), "glass", dict(side=_side)))
        POINT_CASES.append((f"glass-cylinder-{_t}-135-inside-{_side}", _named(f"cylinder-{_t}-135"), "glass", dict(view="inside", side=_side)))
for _t in ("scaled", "mirrored"):
    POINT_CASES.append((f"glass-sphere-reversed-{_t}", scenes.sphere_shape(0.8, to_world=TRANSFORMS[_t], reverse_orientation=True), "glass",
                        dict(side="same")))
POINT_IDS = [c[0] for c in POINT_CASES]
_SETUPS = {}


def point_setup(case):
    """(light, o, d): of light_candidates the light that keeps most of the case's rays (the first of equals), and those rays. The
    choice reads the model alone."""
    name, rec, row_name, kw = case
    if name not in _SETUPS:
        shape = qm.from_record(rec[0])
        best = None
        for light in light_candidates(shape):
            try:
                o, d = select_rays(shape, light=light, **kw)
            except AssertionError:
                continue  # fewer than N_RAYS rays of the batch on the side this case looks from
            kept = point_light_case(shape, ROWS[row_name], light, o, d, wrong_frames=False)["keep"].sum()
            if best is None or kept > best[0]:
                best = (kept, light, o, d)
        _SETUPS[name] = best[1:]
    return _SETUPS[name]


# ---- 2.2 the mirror under an image environment map ----
MIRROR_KR = (0.9, 0.8, 0.7)
MIRROR_ROW = dict(row=(scenes.MAT_MIRROR, MIRROR_KR, (0, 0, 0), 1.0), desc=None, roughness=None)
ENV_MAP = lmm.gentle_map(16, 32)
ENV_TO_WORLD = _rot((0.3, -0.5, 0.8), 37.0)
MIRROR_PLACES = {"scaled": TRANSFORMS["scaled"], "orthonormal-mirror": ORTHONORMAL_MIRROR}
MIRROR_SHAPES = {"sphere": lambda m: scenes.sphere_shape(0.8, to_world=m), "cylinder": lambda m: scenes.cylinder(0.5, -0.6, 0.7, to_world=m),
                 "disk": lambda m: scenes.disk(0.1, 1.0, to_world=m)}
MIRROR_CASES = [(f"{k}-{p}", MIRROR_SHAPES[k](MIRROR_PLACES[p])) for k in MIRROR_SHAPES for p in MIRROR_PLACES]


def env_model():
    if "env" not in _BATCH_CACHE:
        _BATCH_CACHE["env"] = em.EnvModel(ENV_MAP, (1.0, 1.0, 1.0), ENV_TO_WORLD)
    return _BATCH_CACHE["env"]


def mirror_expectation(shape, o, d, t):
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    w2o = np.linalg.inv(shape["o2w"])
    p_obj = (o + d * t[:, None]) @ w2o[:3, :3].T + w2o[:3, 3]
    r = qm.reflect_about(d, qm.normal_at(shape, p_obj))
    return np.asarray(MIRROR_KR) * env_model().le(r), r


def mirror_case(shape, o, d):
    """ref = Kr le(reflect(d, n)); keep: the reflected ray misses the shape (trivially so on a convex body's outside)"""
    m = qm.intersect(shape, o, d)
    t = np.where(m["hit"], m["t"], 1.0)
    ref, r = mirror_expectation(shape, o, d, t)
    moved = [mirror_expectation(shape, o, d, t * (1.0 + s * T_TOL))[0] for s in (1.0, -1.0)]
    allow = np.maximum(np.abs(moved[0] - ref), np.abs(moved[1] - ref)) + RTOL * np.abs(ref)
    blocked, blocked_near = qm.occluded_from_surface(shape, m["p"], r)
    return dict(ref=ref, allow=allow, keep=m["hit"] & ~m["near"] & ~blocked & ~blocked_near)


# ---- 2.3 the lossless glass sphere ----
GLASS_DEPTH, GLASS_ETA, GLASS_RAYS, GLASS_KEYS = 12, 1.5, 200, 64
GLASS_LE = (1.0, 0.8, 0.6)
GLASS_RTOL = 2e-5  # see test_lossless_glass
GLASS_PLACES = {"identity": TRANSFORMS["identity"], "rigid": TRANSFORMS["rigid"], "orthonormal-mirror": ORTHONORMAL_MIRROR}


def glass_sphere_share(shape, o, d):
    """(expected share of samples that return Le, rays to skip): 1 - (1 - R) R^(D - 1) with R the Fresnel reflectance at the first
    hit (a sphere's chord meets it at the same angle at both ends, so every internal hit has that R)"""
    m = qm.intersect(shape, o, d)
    cos = np.abs((m["n"] * -np.asarray(d, np.float64)).sum(axis=1))
    R = bm.fr_dielectric(cos, 1.0, GLASS_ETA)
    return 1.0 - (1.0 - R) * R ** (GLASS_DEPTH - 1), ~m["hit"] | m["near"]


# ---- 2.4 the furnace on convex bodies ----
FURNACE_ROWS = ("plastic", "substrate", "disney")
FURNACE_BODIES = {"sphere-scaled": scenes.sphere_shape(0.8, to_world=TRANSFORMS["scaled"]),
                  "cylinder-rigid": scenes.cylinder(0.5, -0.6, 0.7, to_world=TRANSFORMS["rigid"]),
                  "disk-mirrored": scenes.disk(0.1, 1.0, to_world=TRANSFORMS["mirrored"])}
FURNACE_RAYS, FURNACE_KEYS = 12, 4096
FURNACE_LE = (1.0, 0.8, 0.6)


def furnace_rays(shape, kind):
    """FURNACE_RAYS rays of the batch that hit the body's convex outside (the disk: either side) away from every boundary of
    the hit test, at |cos theta_o| >= 0.3: the whole hemisphere about the normal on the viewer's side is free of the shape"""
    o, d = batch()
    m = qm.intersect(shape, o, d)
    d64 = d.astype(np.float64)
    cos = -(outward(shape, m) * d64).sum(axis=1)
    ok = m["hit"] & ~m["near"] & ((np.abs(cos) if kind == "disk" else cos) >= 0.3)
    idx = np.flatnonzero(ok)[:FURNACE_RAYS]
    assert len(idx) == FURNACE_RAYS
    return o[idx], d[idx]


def _albedo_on_sphere_nodes(model, wo, n):
    wi, w = bm._sphere_nodes(bm.matte_sigma((0.5, 0.5, 0.5), 0.0), wo, n, 4 * n)
    return np.sum(mm.bsdf_f(model, np.broadcast_to(wo, wi.shape), wi) * (np.abs(wi[:, 2]) * w)[:, None], 0)


def furnace_albedo(shape, row, o, d):
    """(albedo (n, 3), its quadrature error (n, 3)) at each ray's wo in the model's frame"""
    m = qm.intersect(shape, o, d)
    wo_l = qm.to_local(qm.surface_frame(shape, m), -np.asarray(d, np.float64))
    model = row["model"]
    out, err = [], []
    for w in wo_l:
        if isinstance(model, mm.Material) and w[2] > 0.0:
            a, b = (mm.albedo(model, w, n, n) for n in (256, 128))
        elif isinstance(model, mm.Material):
            # mm.albedo is written for wo above the surface, and plastic is not even in z: FresnelDielectric(1.5, 1) takes the
            # cosine of wi to the half vector turned to +z, which is negative from below and exchanges the two indices. From
            # below: bxdf_model's nodes over the whole sphere (those of a BSDF without a transmission lobe)
            a, b = (_albedo_on_sphere_nodes(model, w, n) for n in (128, 64))
        else:
            lib = bm if isinstance(model, bm.Bsdf) else dm
            a, b = (lib.albedo(model, w, n, 4 * n) for n in (128, 64))
        out.append(a)
        err.append(np.abs(a - b))
    return np.asarray(out), np.asarray(err)


# ---- 2.5 a shape light seen by a narrow lobe ----
NARROW_ALPHA, NARROW_KS, NARROW_LE = 0.05, (0.6, 0.6, 0.6), 5.0
NARROW_ROW = dict(row=scenes.plastic((0, 0, 0), NARROW_KS, 0.1), desc=None, roughness=(NARROW_ALPHA, NARROW_ALPHA, False),
                  model=mm.Material.plastic((0, 0, 0), NARROW_KS, NARROW_ALPHA, remap=False))
NARROW_POINTS, NARROW_KEYS, NARROW_EYE = 8, 8192, 0.5
_AXIS_UP = rot((1, 0, 0), -90.0)  # object +z -> world +y


def _ring(centre, radius, offset_deg=10.0):
    """NARROW_POINTS points of the plane about `centre`, from 0.6 to 1.3 times `radius` away: no two under the same angle"""
    k = np.arange(NARROW_POINTS)
    a = np.radians(k * 360.0 / NARROW_POINTS + offset_deg)
    return np.asarray(centre) + (radius * (0.6 + 0.1 * k))[:, None] * np.stack([np.cos(a), np.zeros_like(a), np.sin(a)], axis=1), a


def narrow_setup(name):
    """The emitters of test_gpu_shapes.py's closed forms over a plastic plane y = const (normal +y): dict with the emitter's
    record (material 1, light 0), the plane's height, two_sided, the plane points, for each the emitter point its mirror
    direction aims at, the light's pdf over solid angle as weight(wi_l, r2, cos_s) arguments, and `halve`: whether the
    quadrature over the whole shape counts every direction twice (a sphere seen from outside)."""
    if name == "disk":  # test_disk_light_closed_form, "rotated", R = h
        p0, h = np.array([0.3, 0.0, -0.2]), 1.2
        rec = scenes.disk(0.0, h, to_world=translate(p0[0], h, p0[2]) @ rot((1, 0, 0), 90.0) @ rot((0, 0, 1), 63.0), material=1, light=0)
        pts, _ = _ring(p0, 0.5)
        area = np.pi * h * h
        return dict(rec=rec, y=0.0, two_sided=0, points=pts, targets=np.tile(p0 + [0.0, h, 0.0], (NARROW_POINTS, 1)), halve=False,
                    light_pdf=lambda wi_l, r2, cos_s: r2 / (cos_s * area))
    if name == "cylinder":  # test_cylinder_light_closed_form: emits inward, the plane through its middle across the axis
        R, H = 0.8, 1.1
        move = translate(0.2, -0.1, 0.3)
        rec = scenes.cylinder(R, -H, H, to_world=move @ _AXIS_UP @ rot((0, 0, 1), 20.0), material=1, light=0)
        pts, a = _ring(move[:3, 3], 0.2)
        b = a + np.radians(100.0)
        targets = move[:3, 3] + np.stack([R * np.cos(b), np.full_like(b, 0.5), R * np.sin(b)], axis=1)
        area = 2.0 * H * R * 2.0 * np.pi
        return dict(rec=rec, y=-0.1, two_sided=1, points=pts, targets=targets, halve=False, light_pdf=lambda wi_l, r2, cos_s: r2 / (cos_s * area))
    # test_rotated_sphere_light_closed_form at R / d = 0.5: Sphere::sample's uniform cone
    d, ratio, p0 = 1.5, 0.5, np.array([0.3, 0.0, -0.2])
    rec = scenes.sphere_shape(ratio * d, to_world=translate(p0[0], d, p0[2]) @ rot((1, 2, 3), 40.0), material=1, light=0)
    pts, _ = _ring(p0, 0.6)
    centre = p0 + [0.0, d, 0.0]

    def cone_pdf(point):
        sin2 = (ratio * d) ** 2 / ((centre - point) ** 2).sum()
        return lambda wi_l, r2, cos_s: np.full(len(r2), 1.0 / (2.0 * np.pi * (1.0 - np.sqrt(1.0 - sin2))))
    return dict(rec=rec, y=0.0, two_sided=0, points=pts, targets=np.tile(centre, (NARROW_POINTS, 1)), halve=True, light_pdf=cone_pdf)


NARROW_LIGHTS = ("disk", "cylinder", "sphere")


def narrow_rays(setup):
    """(o, d): for each plane point the eye NARROW_EYE away along the mirror image (about +y) of the direction to its target"""
    wi = setup["targets"] - setup["points"]
    wi /= np.sqrt((wi ** 2).sum(axis=1))[:, None]
    wo = wi * np.array([-1.0, 1.0, -1.0])
    return (setup["points"] + NARROW_EYE * wo).astype(np.float32), (-wo).astype(np.float32)


def narrow_reference(name):
    """per plane point: (radiance (n, 3), quadrature error (n, 3), share of the estimate the BSDF-sampled branch of
    estimate_direct carries: the integral of f cos w_bsdf over the emitter's solid angle over that of f cos, w_bsdf the power
    heuristic's weight with the model's pdfs). Cached."""
    if ("narrow", name) in _BATCH_CACHE:
        return _BATCH_CACHE[("narrow", name)]
    setup = narrow_setup(name)
    shape, model = qm.from_record(setup["rec"][0]), NARROW_ROW["model"]
    fr = dict(ss=np.array([1.0, 0.0, 0.0]), ts=np.array([0.0, 0.0, -1.0]), ns=np.array([0.0, 1.0, 0.0]))  # ts = ns x ss
    o, d = narrow_rays(setup)
    f = lambda wo_l, wi_l: mm.bsdf_f(model, wo_l, wi_l)  # noqa: E731
    out = []
    for k, point in enumerate(setup["points"]):
        # the model's point is where the float32 ray meets the plane, not the float64 point it was aimed at
        o64, d64 = o[k].astype(np.float64), d[k].astype(np.float64)
        p = o64 + d64 * ((setup["y"] - o64[1]) / d64[1])
        value, err = qm.bsdf_patch_radiance_by_quadrature(shape, p, fr, -d64, f, NARROW_LE)
        pdf_l = setup["light_pdf"](point) if name == "sphere" else setup["light_pdf"]
        wo_l = qm.to_local(fr, -d64[None, :])

        def w_bsdf(wi_l, r2, cos_s):
            pb = mm.bsdf_pdf(model, np.broadcast_to(wo_l, wi_l.shape), wi_l)
            pl = pdf_l(wi_l, r2, cos_s)
            return pb * pb / np.maximum(pb * pb + pl * pl, 1e-300)
        by_bsdf, _ = qm.bsdf_patch_radiance_by_quadrature(shape, p, fr, -d64, f, NARROW_LE, weight=w_bsdf)
        scale = 0.5 if setup["halve"] else 1.0
        out.append((scale * value, scale * err, float(by_bsdf[1] / value[1])))
    res = (np.array([v[0] for v in out]), np.array([v[1] for v in out]), np.array([v[2] for v in out]))
    _BATCH_CACHE[("narrow", name)] = res
    return res
