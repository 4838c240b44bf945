"""Cases and float64 references that hold estimate_direct (csrc/wf_lights.h: the MIS estimator behind every area light and
infinite light) for the level-2 rows (matte with sigma, rough glass, substrate), the Disney rows and the lobe rows (uber,
translucent, mix), shared by test_mis_model.py (the references against themselves, no GPU) and test_gpu_mis_materials.py (the
device against the references).

A row under test lies on the plane z = 0 (scenes._plane_z0: shading frame ss = +x, ts = +y, ns = +z on its first triangle, where
every test point is). Over or under it hangs a rectangular mesh emitter of two triangles, one diffuse area light each; or the
plane lies under an image environment map with a rotated light_to_world. What leaves a plane point p towards wo is

    L int f(wo, wi) |cos_p| cos_s / r^2 dA            (quad_light_radiance: the midpoint rule over the rectangle)
    int f(wo, wi) |cos_p| le(wi) d omega              (envmap_radiance: the midpoint rule over EnvModel.directions)

plus, for a lobe row, the weights f |cos| / pdf of its specular lobes times what their directions meet (specular_term). f and
pdf are the float64 models' (bxdf_model, disney_model, lobe_model under NON_SPECULAR). Every reference carries its own error
estimate, the change from half the grid. Nothing here reads the library's results."""
from functools import lru_cache

import numpy as np

from pbrt_hip import scenes
import bxdf_cases
import bxdf_model as bm
import disney_model as dm
import envmap_model as em
import lobe_model as lm

KD = (0.5, 0.4, 0.3)
GREY = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
BLACK = (scenes.MAT_MATTE, (0, 0, 0), (0, 0, 0), 1.0)
FRAME = dict(ss=np.array([1.0, 0, 0]), ts=np.array([0, 1.0, 0]), ns=np.array([0, 0, 1.0]))  # of the plane's first triangle


# ---- rows ----
class Row:
    """name, family ('level2', 'disney', 'lobe'), how a scene gets the row (key of the scene dict and descriptor, or for the mix
    the operand rows), and the model: f(wo, wi) and pdf(wo, wi) as estimate_direct asks for them (lobe rows: under
    NON_SPECULAR), the specular lobes (a lobe_model.Bsdf or None), the shim bxdf_cases.in_band reads with the glossy
    transmission lobe's own f (f_band, or None), albedo(wo, n_theta)."""

    def __init__(self, name, family, key, desc, model):
        self.name, self.family, self.key, self.desc, self.model = name, family, key, desc, model
        if family == "level2":
            self.f, self.pdf = (lambda wo, wi: bm.bsdf_f(model, wo, wi)), (lambda wo, wi: bm.bsdf_pdf(model, wo, wi))
            self.shim, self.albedo = model, (lambda wo, n=128: bm.albedo(model, wo, n, 4 * n))
            self.f_band = (lambda wo, wi: bm.trans_f(model, wo, wi)) if "trans" in model.lobes else None
        elif family == "disney":
            self.f, self.pdf = (lambda wo, wi: dm.bsdf_f(model, wo, wi)), (lambda wo, wi: dm.bsdf_pdf(model, wo, wi))
            self.shim, self.albedo = model.trans_shim(), (lambda wo, n=128: dm.albedo(model, wo, n, 4 * n))
            self.f_band = (lambda wo, wi: dm.trans_f(model, wo, wi)) if "trans" in model.lobes else None
        else:
            self.f = lambda wo, wi: lm.bsdf_f(model, wo, wi, lm.NON_SPECULAR)
            self.pdf = lambda wo, wi: lm.bsdf_pdf(model, wo, wi, lm.NON_SPECULAR)
            self.shim, self.albedo = model.trans_shim(), (lambda wo, n=128: lm.albedo(model, wo, n, 4 * n))
            glossy_t = [l for l in model.lobes if l.kind == lm.MICRO_T]
            self.f_band = (lambda wo, wi: sum(l.scale * lm.lobe_f(l, wo, wi) for l in glossy_t)) if glossy_t else None
        self.specular = model if family == "lobe" and any(l.type & lm.SPECULAR for l in model.lobes) else None

    def install(self, sc):
        """the scene dict with its material row 0 made this row"""
        sc = dict(sc)
        if self.key == "mix":
            (row_a, _), (row_b, _), _ = self.desc
            sc["materials"] = np.concatenate([sc["materials"], scenes._materials([row_a, row_b])])
        else:
            sc[self.key] = {0: self.desc}
        return sc

    def after(self, scene, n_rows):
        """what a mix needs once the scene exists: the metal operand's alphas set directly, then the mix over the two operand rows
        (the last two of the table), which copies their lists"""
        if self.key == "mix":
            (_, _), (_, alphas), amount = self.desc
            scene.set_material_roughness(n_rows + 1, alphas[0], alphas[1], remap=False)
            scene.set_lobe_material(0, scenes.mix(n_rows, n_rows + 1, amount))


def _level2(name, desc, model):
    return Row(name, "level2", "material_descs", desc, model)


def _disney(name, **kw):
    d = scenes.disney((0.8, 0.5, 0.3), **kw)
    return Row(name, "disney", "disney_descs", d, dm.Disney(d))


def _lobe(name, fn_s, fn_m, **kw):
    return Row(name, "lobe", "lobe_descs", fn_s(**kw), fn_m(**kw))


_METAL_ETA, _METAL_K, _METAL_ALPHA, _MIX_KD, _MIX_AMOUNT = (0.2, 0.9, 1.1), (3.0, 2.5, 2.0), (0.15, 0.3), (0.6, 0.5, 0.4), 0.3
# Roughness 0.1 or above everywhere (a Disney row's alphas are roughness^2 over / times its aspect: 0.4 with anisotropic 0.6 gives
# (0.236, 0.108); the thin row's transmission is scaled by 0.65 eta - 0.35: 0.55 gives 0.118; clearcoat gloss 0 is alpha 0.1).
ROWS = {r.name: r for r in [
    _level2("matte_sigma", scenes.matte_sigma((0.6, 0.5, 0.4), 30.0), bm.matte_sigma((0.6, 0.5, 0.4), 30.0)),
    _level2("substrate", scenes.substrate(KD, (0.3, 0.3, 0.4), 0.1, 0.2, remap=False), bm.substrate(KD, (0.3, 0.3, 0.4), 0.1, 0.2, remap=False)),
    _level2("rough_glass", scenes.rough_glass(bxdf_cases.KR, bxdf_cases.KT, 1.5, 0.15, remap=False),
            bm.rough_glass(bxdf_cases.KR, bxdf_cases.KT, 1.5, 0.15, remap=False)),
    _disney("disney_opaque", roughness=0.4, anisotropic=0.6, sheen=0.5, clearcoat=1.0, clearcoat_gloss=0.0),
    _disney("disney_spec_trans", spec_trans=0.7, roughness=0.4),
    _disney("disney_thin", thin=True, flatness=0.5, diff_trans=1.0, spec_trans=0.5, roughness=0.55),
    _lobe("uber", scenes.uber, lm.uber, kd=KD, ks=0.4, kr=0.3, kt=0.2, opacity=0.8, eta=1.5, u_roughness=0.12, v_roughness=0.25, remap=False),
    _lobe("translucent", scenes.translucent, lm.translucent, kd=KD, ks=0.5, reflect=(0.3, 0.5, 0.7), transmit=(0.7, 0.5, 0.3), roughness=0.2,
          remap=False),
    Row("mix_matte_metal", "lobe", "mix", (((scenes.MAT_MATTE, _MIX_KD, (0, 0, 0), 1.0), None), (scenes.metal(_METAL_ETA, _METAL_K, 0.2), _METAL_ALPHA),
                                          _MIX_AMOUNT),
        lm.mix(lm.matte(_MIX_KD), lm.metal(_METAL_ETA, _METAL_K, *_METAL_ALPHA, remap=False), _MIX_AMOUNT)),
]}
GLOSSY_OR_TRANSMISSIVE = [n for n in ROWS if n != "matte_sigma"]

# (row, side of the eye, side of the emitter): +1 above the plane (the side of ns), -1 below it
VIEWS = ([("matte_sigma", 1, 1), ("substrate", 1, 1), ("rough_glass", 1, 1), ("rough_glass", 1, -1), ("rough_glass", -1, 1), ("disney_opaque", 1, 1),
          ("disney_spec_trans", 1, 1), ("disney_spec_trans", 1, -1), ("disney_thin", 1, -1), ("uber", 1, 1), ("uber", -1, -1), ("uber", 1, -1)]
         + [("translucent", e, l) for e in (1, -1) for l in (1, -1)] + [("mix_matte_metal", 1, 1)])


def view_name(view):
    return f"{view[0]}-eye{view[1]:+d}-light{view[2]:+d}"


# ---- the emitters and the plane points ----
LE = np.array([3.0, 2.0, 1.5])
POINTS = np.array([(0.9, -0.9, 0.0), (0.1, -0.3, 0.0), (1.3, -0.2, 0.0), (1.9, -1.0, 0.0)])  # y < x: the plane's first triangle
# name: (centre (x, y), height, half-sizes, two-sided, faces the plane). `near`: 2 x 2 at 0.5, one-sided, seen along the mirror
# image of its centre (eye on its side) or straight through the plane (eye on the other side): the BSDF-sampled half carries much
# of the estimate; the last point lies outside its footprint. `far`: 1.0 x 0.6 at height 1, two-sided, seen off the lobes
# (view_wo): the light-sampled half carries it. `away`: `near` facing away from the plane: nothing arrives.
EMITTERS = {"near": ((0.4, -0.5), 0.5, (1.0, 1.0), 0, True), "far": ((0.7, 0.3), 1.0, (0.5, 0.3), 1, True), "away": ((0.4, -0.5), 0.5, (1.0, 1.0), 0, False)}
PLANE_HALF = 10.0
EYE_HEIGHT = 0.2   # the eye's rays start this far from the plane: below every emitter


def emitter_corners(name, side):
    """(4, 3) corners c0 .. c3 of the emitter on `side` of the plane; its triangles are (c0, c1, c2) and (c0, c2, c3) and it emits
    on the side of cross(c1 - c0, c2 - c0)"""
    (cx, cy), h, (hx, hy), _, faces = EMITTERS[name]
    c = np.array([(cx - hx, cy - hy), (cx - hx, cy + hy), (cx + hx, cy + hy), (cx + hx, cy - hy)])  # normal -z
    if (side > 0) != faces:
        c = c[::-1]
    return np.concatenate([c, np.full((4, 1), side * h)], axis=1)


AIM = {"near": (0.0, 0.0), "away": (0.0, 0.0), "far": (0.8, 0.5)}  # from the emitter's centre, in its plane


def view_wo(view, emitter):
    """(4, 3) unit directions towards the eye at POINTS: the mirror image (about the plane's normal) of the direction to the
    emitter's aim point when the eye is on the emitter's side, the opposite of that direction when it is not. The aim point is
    the centre of `near`; beside `far` it lies 0.6 of a half-size outside the rectangle, so the lobes pass it by. Rough glass seen
    from below, from inside the denser medium: the direction that refracts towards the aim point (straight through, the
    oblique points would see the emitter past the critical angle, where the transmission lobe is nowhere near it)."""
    name, eye, light = view
    (cx, cy), h, _, _, _ = EMITTERS[emitter]
    d = np.array([cx + AIM[emitter][0], cy + AIM[emitter][1], light * h]) - POINTS
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if eye == light:
        return d * np.array([-1.0, -1.0, 1.0])
    if name == "rough_glass" and eye < 0:
        eta = ROWS[name].model.eta
        return -np.concatenate([d[:, :2] / eta, np.sqrt(1.0 - (d[:, :2] ** 2).sum(axis=1, keepdims=True) / eta ** 2)], axis=1)
    return -d


def view_rays(view, emitter, rotation=None):
    """the eye's rays (scenes.RAY_DTYPE), one per point, under the rotation (3 x 3) of everything"""
    wo = view_wo(view, emitter)
    o = POINTS + wo * (EYE_HEIGHT / np.abs(wo[:, 2:3]))
    r = np.eye(3) if rotation is None else rotation
    rays = np.zeros(len(o), dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_max"] = (o @ r.T).astype(np.float32), (-wo @ r.T).astype(np.float32), np.inf
    return rays


def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


ROTATION = _rodrigues((0.3, 0.5, 0.81), 0.9)  # no axis of the plane's frame stays on a world axis
ORIENTATIONS = {"aligned": None, "rotated": ROTATION}


def light_scene(row, emitter, side, rotation=None):
    """(scene dict, after(scene)): the row on the plane, the emitter's two triangles on a black matte row with one diffuse area
    light each, everything turned by `rotation`"""
    pos, idx = scenes._plane_z0(PLANE_HALF)
    p = np.concatenate([pos.astype(np.float64), emitter_corners(emitter, side)])
    if rotation is not None:
        p = p @ rotation.T
    two_sided = EMITTERS[emitter][3]
    sc = dict(positions=p.astype(np.float32), indices=np.concatenate([idx, idx + 4]), tri_material=np.array([0, 0, 1, 1], np.int32),
              materials=scenes._materials([GREY, BLACK]), tri_light=np.array([-1, -1, 0, 1], np.int32),
              lights=scenes._lights([(scenes.LIGHT_DIFFUSE_AREA, tuple(LE), 2, two_sided, 1), (scenes.LIGHT_DIFFUSE_AREA, tuple(LE), 3, two_sided, 1)]))
    return row.install(sc), lambda scene: row.after(scene, 2)


# ---- references ----
def to_local(frame, w):
    return np.stack([w @ frame["ss"], w @ frame["ts"], w @ frame["ns"]], axis=-1)


def _power_share(pa, pb):
    """the power heuristic's weight of the strategy with pdf pa beside the one with pdf pb (0 where both are 0)"""
    a2, b2 = pa * pa, pb * pb
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a2 + b2 > 0, a2 / (a2 + b2), 0.0)


def _band_part(band, geometry, wo_l, wi_l):
    """the part of an integral that the glossy transmission lobe (band = (the shim bxdf_cases.in_band reads, that lobe's f))
    takes from its grazing band, where the device is held to the model less tightly (test_gpu_bxdfs.py)"""
    if band is None or band[1] is None:
        return np.zeros(3)
    inb = bxdf_cases.in_band(band[0], wo_l, wi_l)
    return (geometry[inb] * band[1](wo_l[inb], wi_l[inb])).sum(axis=0) if inb.any() else np.zeros(3)


def quad_light_terms(f, pdf, p, frame, wo, corners, L, two_sided, cells, band=None):
    """The integral of quad_light_radiance at one grid and what test_mis_model.py needs beside it, all (3,): `value`; `bsdf`,
    the part the power heuristic gives the BSDF-sampled half (pb the model's pdf, pl = r^2 / (cos_s area)); `no_cos`, the
    expectation of an estimator whose BSDF-sampled half weighs with a light pdf that lacks cos_s; `band`, the part of `value` from
    bxdf_cases.in_band's grazing band."""
    c = np.asarray(corners, np.float64)
    e1, e2 = c[1] - c[0], c[3] - c[0]
    n_e = np.cross(e1, c[2] - c[0])
    area = np.linalg.norm(np.cross(e1, e2))
    n_e /= np.linalg.norm(n_e)
    u = (np.arange(cells) + 0.5) / cells
    uu, vv = np.meshgrid(u, u, indexing="ij")
    q = c[0] + uu.reshape(-1, 1) * e1 + vv.reshape(-1, 1) * e2
    w = q - np.asarray(p, np.float64)
    r2 = (w * w).sum(axis=1)
    wi = w / np.sqrt(r2)[:, None]
    cos_s = -(wi @ n_e)
    emits = np.abs(cos_s) if two_sided else np.maximum(cos_s, 0.0)
    wi_l = to_local(frame, wi)
    wo_l = np.broadcast_to(to_local(frame, np.asarray(wo, np.float64)), wi_l.shape)
    geometry = (np.abs(wi_l[:, 2]) * emits / r2 * (area / (cells * cells)))[:, None] * np.asarray(L, np.float64)
    g = geometry * f(wo_l, wi_l)
    pb = pdf(wo_l, wi_l)
    with np.errstate(divide="ignore"):
        pl, pl_no_cos = np.where(emits > 0, r2 / (np.abs(cos_s) * area), np.inf), r2 / area
    share = _power_share(pb, pl)
    out = dict(value=g.sum(axis=0), bsdf=(g * share[:, None]).sum(axis=0),
               no_cos=(g * (1.0 - share + _power_share(pb, pl_no_cos))[:, None]).sum(axis=0))
    out["band"] = _band_part(band, geometry, wo_l, wi_l)
    return out


def quad_light_radiance(f, pdf, p, frame, wo, corners, L, two_sided, cells):
    """L int f(wo, wi) |cos_p| cos_s / r^2 dA over the rectangle `corners` (emitter_corners' convention) by the midpoint rule on
    cells x cells cells: the radiance leaving p (world) towards wo (world) in the shading frame `frame` under a diffuse emitter
    nothing shadows. One-sided: only cos_s > 0, the emitting side, counts. f(wo, wi), pdf(wo, wi): the model's, on local
    directions (n, 3). Returns (value (3,), |value - value at cells / 2|, the BSDF-branch share: the same integral weighted by
    pb^2 / (pb^2 + pl^2), summed over the channels, over the value's sum). The share describes the case, it is not compared
    with anything: the scenes hold one light per triangle, of half this area, so the device's own split leans a little
    further towards the light-sampled half, with the same expectation."""
    fine = quad_light_terms(f, pdf, p, frame, wo, corners, L, two_sided, cells)
    coarse = quad_light_terms(f, pdf, p, frame, wo, corners, L, two_sided, cells // 2)
    total = fine["value"].sum()
    return fine["value"], np.abs(fine["value"] - coarse["value"]), float(fine["bsdf"].sum() / total) if total > 0 else 0.0


def envmap_terms(f, pdf, frame, wo, env, n_theta, wrong_pdf=None, band=None):
    """as quad_light_terms over EnvModel.directions(n_theta, 2 n_theta): `value`, `bsdf` (pl = env.pdf), `band`, and `wrong_pdf`:
    the expectation of an estimator whose BSDF-sampled half weighs with wrong_pdf(world direction) in place of env.pdf"""
    wi, dw = env.directions(n_theta, 2 * n_theta)
    wi_l = to_local(frame, wi)
    wo_l = np.broadcast_to(to_local(frame, np.asarray(wo, np.float64)), wi_l.shape)
    geometry = (np.abs(wi_l[:, 2]) * dw)[:, None] * env.le(wi)
    g = geometry * f(wo_l, wi_l)
    pb = pdf(wo_l, wi_l)
    share = _power_share(pb, env.pdf(wi))
    out = dict(value=g.sum(axis=0), bsdf=(g * share[:, None]).sum(axis=0))
    if wrong_pdf is not None:
        out["wrong_pdf"] = (g * (1.0 - share + _power_share(pb, wrong_pdf(wi)))[:, None]).sum(axis=0)
    out["band"] = _band_part(band, geometry, wo_l, wi_l)
    return out


def envmap_radiance(f, pdf, frame, wo, env, n_theta):
    """int f(wo, wi) |cos_p| le(wi) d omega over the whole sphere by the midpoint rule in the light's (theta, phi), n_theta x
    2 n_theta cells. Returns (value, |value - value at n_theta / 2|, the BSDF-branch share with pl = env.pdf)."""
    fine = envmap_terms(f, pdf, frame, wo, env, n_theta)
    coarse = envmap_terms(f, pdf, frame, wo, env, n_theta // 2)
    return fine["value"], np.abs(fine["value"] - coarse["value"]), float(fine["bsdf"].sum() / fine["value"].sum())


def rect_hit(p, w, corners, two_sided):
    """where the ray p + t w meets the emitter's plane: (emitting side met inside the rectangle, margin). The margin is the
    distance of the meeting point from the rectangle's nearest edge over the half-size across that edge (inside or outside), inf
    where the ray never reaches the plane."""
    c = np.asarray(corners, np.float64)
    e1, e2 = c[1] - c[0], c[3] - c[0]
    n_e = np.cross(e1, c[2] - c[0])
    denom = w @ n_e
    if denom == 0.0:
        return False, np.inf
    t = ((c[0] - p) @ n_e) / denom
    if t <= 0.0:
        return False, np.inf
    q = p + t * w - (c[0] + 0.5 * (e1 + e2))
    a, b = 2.0 * (q @ e1) / (e1 @ e1), 2.0 * (q @ e2) / (e2 @ e2)  # in half-sizes from the centre
    inside = abs(a) < 1.0 and abs(b) < 1.0
    margin = min(1.0 - abs(a), 1.0 - abs(b)) if inside else max(abs(a) - 1.0, abs(b) - 1.0)
    return bool(inside and (two_sided or denom < 0.0)), float(margin)


def specular_term(model, wo, le_along, pl_along=None):
    """The specular lobes' part of the radiance towards wo (local, (3,)): the sum over the specular lobes of scale f |cos| / pdf from
    lm.specular_sample times le_along(wi) (local direction -> (3,): the emitter's Le where the direction meets its emitting side,
    or the environment's le along it). Returns (sum, per-lobe [(wi, weight (3,), radiance (3,))]). With pl_along(wi) (the light's
    pdf along wi, 0 where it misses) also what an estimate_direct that samples the BSDF under BSDF_ALL adds on top: each specular
    lobe once more, times the power heuristic's weight of its pdf 1 / n beside pl."""
    total, extra, lobes = np.zeros(3), np.zeros(3), []
    for l in model.lobes:
        if not l.type & lm.SPECULAR:
            continue
        ws, fs, ps = lm.specular_sample(l, np.asarray(wo, np.float64).reshape(1, 3))
        if ps[0] == 0:
            continue
        weight = l.scale * fs[0] * abs(ws[0, 2]) / ps[0]
        le = np.asarray(le_along(ws[0]), np.float64)
        total = total + weight * le
        lobes.append((ws[0], weight, le))
        if pl_along is not None:
            extra = extra + weight * le * _power_share(np.float64(1.0 / model.n), np.float64(pl_along(ws[0])))
    return (total, lobes) if pl_along is None else (total, lobes, extra)


CELLS = 128        # the rectangle's grid: halving errors of 1e-4 relative and below here (test_mis_model.py prints them) ...
CELLS_ACROSS = 256  # ... but through a glossy transmission lobe, whose f ends on an edge (a microfacet seen from behind)
N_THETA = 256      # the sphere's grid, a multiple of twice the map's 16 rows: the cells' edges lie on the kinks of its bilinear lookup


@lru_cache(maxsize=None)
def light_reference(view, emitter):
    """the references of one (view, emitter) at the four points, computed once for every estimator and orientation: dict of
    ref (4, 3) = quadrature + specular term, err (4, 3), share (4,), and the parts test_mis_model.py looks at"""
    row = ROWS[view[0]]
    corners, two_sided = emitter_corners(emitter, view[2]), EMITTERS[emitter][3]
    wo = view_wo(view, emitter)
    area = 4.0 * EMITTERS[emitter][2][0] * EMITTERS[emitter][2][1]
    keys = ("ref", "err", "quad", "bsdf", "no_cos", "band", "spec", "all_extra", "as_two_sided")
    out = {k: np.zeros((len(POINTS), 3)) for k in keys}
    out["share"], out["margin"], out["spec_hits"] = np.zeros(len(POINTS)), np.full(len(POINTS), np.inf), np.zeros(len(POINTS), int)
    cells = CELLS_ACROSS if view[1] != view[2] and row.f_band is not None else CELLS
    for i, p in enumerate(POINTS):
        fine = quad_light_terms(row.f, row.pdf, p, FRAME, wo[i], corners, LE, two_sided, cells, (row.shim, row.f_band))
        coarse = quad_light_terms(row.f, row.pdf, p, FRAME, wo[i], corners, LE, two_sided, cells // 2)
        for k in ("bsdf", "no_cos", "band"):
            out[k][i] = fine[k]
        out["quad"][i], out["err"][i] = fine["value"], np.abs(fine["value"] - coarse["value"])
        out["share"][i] = fine["bsdf"].sum() / fine["value"].sum() if fine["value"].sum() > 0 else 0.0
        if not EMITTERS[emitter][4]:  # what arrives from an emitter facing away if its side is not asked for
            out["as_two_sided"][i] = quad_light_terms(row.f, row.pdf, p, FRAME, wo[i], corners, LE, True, cells)["value"]
        if row.specular is not None:
            def le_along(wi, p=p):
                return LE if rect_hit(p, wi, corners, two_sided)[0] else np.zeros(3)

            def pl_along(wi, p=p):
                hit, _ = rect_hit(p, wi, corners, two_sided)
                if not hit:
                    return 0.0
                t = (corners[0, 2] - p[2]) / wi[2]
                return t * t / (abs(wi[2]) * area)   # the emitter is parallel to the plane: cos_s = |wi.z|

            out["spec"][i], lobes, out["all_extra"][i] = specular_term(row.specular, wo[i], le_along, pl_along)
            out["margin"][i] = min(rect_hit(p, wi, corners, True)[1] for wi, _, _ in lobes)
            out["spec_hits"][i] = sum(1 for _, _, le in lobes if le.any())
            out["as_two_sided"][i] += 0.0 if two_sided else specular_term(
                row.specular, wo[i], lambda wi, p=p: LE if rect_hit(p, wi, corners, True)[0] else np.zeros(3))[0]
    out["ref"] = out["quad"] + out["spec"]
    return out


# ---- the image environment map ----
def env_map():
    """32 x 16: a ground of 0.2 to 0.5 per channel with a block of 3 x 2 texels 30 times as bright"""
    rgb = np.random.default_rng(11).uniform(0.2, 0.5, size=(16, 32, 3))
    rgb[4:6, 20:23] *= 30.0
    return rgb.astype(np.float32)


ENV_MAP = env_map()
ENV_TO_WORLD = np.eye(4, dtype=np.float32)
ENV_TO_WORLD[:3, :3] = _rodrigues((0, 0, 1), 0.7) @ _rodrigues((1, 0, 0), 0.7)
# polar angles away from 30 to 40 degrees: seen from below near the critical angle (41.8 degrees) the grazing band of glossy
# transmission carries 2e-4 to 4e-4 of the integral, at these below 6e-5 (test_mis_model.py asserts it)
_ENV_THETA, _ENV_PHI = (20.0, 55.0), (20.0, 250.0)
# rows with a transmissive lobe are seen from both sides
ENV_VIEWS = [(n, s, k) for n in ROWS for s in ((1, -1) if n in ("rough_glass", "disney_spec_trans", "disney_thin", "uber", "translucent") else (1,))
             for k in (0, 1)]


def env_view_name(view):
    return f"{view[0]}-eye{view[1]:+d}-dir{view[2]}"


def env_wo(view):
    t, ph = np.radians(_ENV_THETA[view[2]]), np.radians(_ENV_PHI[view[2]])
    return np.array([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), view[1] * np.cos(t)])


def env_ray(view):
    wo = env_wo(view)
    rays = np.zeros(1, dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_max"] = (np.array([0.3, -0.4, 0.0]) + 2.0 * wo).astype(np.float32), (-wo).astype(np.float32), np.inf
    return rays


@lru_cache(maxsize=None)
def env_models():
    return em.EnvModel(ENV_MAP, (1.0, 1.0, 1.0), ENV_TO_WORLD), em.EnvModel(ENV_MAP, (1.0, 1.0, 1.0), None)


def env_scene(row):
    sc = scenes.glossy_plane_env_scene(GREY)
    return row.install(sc), lambda scene: (row.after(scene, 1), scene.set_environment_map(0, ENV_MAP, ENV_TO_WORLD))


@lru_cache(maxsize=None)
def env_reference(view):
    """dict of ref (3,) = quadrature + specular term, err, share and the parts test_mis_model.py looks at"""
    row, wo = ROWS[view[0]], env_wo(view)
    env, unrotated = env_models()
    fine = envmap_terms(row.f, row.pdf, FRAME, wo, env, N_THETA, unrotated.pdf, (row.shim, row.f_band))
    coarse = envmap_terms(row.f, row.pdf, FRAME, wo, env, N_THETA // 2)
    out = dict(quad=fine["value"], err=np.abs(fine["value"] - coarse["value"]), bsdf=fine["bsdf"], wrong_pdf=fine["wrong_pdf"], band=fine["band"],
               share=float(fine["bsdf"].sum() / fine["value"].sum()), spec=np.zeros(3), all_extra=np.zeros(3))
    if row.specular is not None:
        out["spec"], _, out["all_extra"] = specular_term(row.specular, wo, lambda wi: env.le(wi[None, :])[0], lambda wi: env.pdf(wi[None, :])[0])
    out["ref"] = out["quad"] + out["spec"]
    return out
