"""The curve cases test_curve_model.py and test_gpu_curves.py share: each a curve of one type, straight or bent, under a rigid, a
scaled or a mirrored transform, split into two segment records, with a batch of rays aimed at it from outside and from inside
its bound. A case's float64 and float32 model runs are computed once and kept.

EDGE_CASES (further down) are the inputs of the hit test those 18 cases never reach: hair-thin curves and the depth clamp, a
width of zero, a self-crossing loop, a hand-set u range, coincident control points, ribbon normals that are equal or at 90
degrees, grazing and chord-parallel rays, and far or scaled placements. Each has a margin and a tolerance of its own
(edge_model, edge_spread) and leaves out the rays whose verdict the device's push of the origin may turn (edge_keep); none of
them enters the 18 cases' shared tolerance."""
import functools
import zlib

import numpy as np

from pbrt_hip import scenes

import curve_model

N_RAYS = 4096
MARGIN = 1e-3          # rays nearer than this fraction of hit_width to a decision of the algorithm are left out
MAX_LEFT_OUT = 0.02    # at most this part of a case's rays

STRAIGHT = np.array([(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.8, 0.0, 0.0), (1.2, 0.0, 0.0)])
BENT = np.array([(0.0, 0.0, 0.0), (0.3, 0.8, 0.1), (0.9, -0.6, 0.3), (1.2, 0.2, -0.2)])


def _rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(deg)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def transform(kind):
    m = np.eye(4)
    m[:3, :3] = _rotation((1.0, 2.0, 0.5), 37.0)
    m[:3, 3] = (0.3, -0.2, 0.5)
    if kind == "scaled":
        m[:3, :3] = m[:3, :3] @ np.diag([1.7, 0.6, 1.2])
    elif kind == "mirrored":
        m[:3, :3] = m[:3, :3] @ np.diag([1.0, -1.0, 1.0])
    return m


TYPES = ("flat", "cylinder", "ribbon")
BENDS = ("straight", "bent")
TRANSFORMS = ("rigid", "scaled", "mirrored")
CASES = [(t, b, x) for t in TYPES for b in BENDS for x in TRANSFORMS]


def case_curves(kind, bend, xform, split_depth=1):
    cp = STRAIGHT if bend == "straight" else BENT
    normals = np.array([(0.0, 0.0, 1.0), (0.0, 1.0, 1.0)]) if kind == "ribbon" else None
    return scenes.curve(cp, 0.05, 0.02, type=kind, normals=normals, to_world=transform(xform), material=0, split_depth=split_depth,
                        reverse_orientation=(xform == "scaled"))


def _bezier(cp, u):
    u = u[:, None]
    return ((1 - u) ** 3) * cp[0] + 3 * u * (1 - u) ** 2 * cp[1] + 3 * u * u * (1 - u) * cp[2] + u ** 3 * cp[3]


def case_rays(kind, bend, xform, n=N_RAYS):
    """(o, d, t_max): three quarters aimed from outside at points within 1.5 widths of the curve, a quarter starting inside
    its bound (within 3 widths of it) in a random direction; direction lengths in [0.5, 2]; every eighth ray with a finite t_max"""
    seed = 1000 + 100 * TYPES.index(kind) + 10 * BENDS.index(bend) + TRANSFORMS.index(xform)
    rng = np.random.default_rng(seed)
    cp = STRAIGHT if bend == "straight" else BENT
    m = transform(xform)
    on_curve = _bezier(cp, rng.uniform(-0.05, 1.05, n)) @ m[:3, :3].T + m[:3, 3]
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    target = on_curve + unit * (rng.uniform(0, 1.5, (n, 1)) * 0.05)
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    inside = np.arange(n) % 4 == 3
    o = np.where(inside[:, None], on_curve + unit * (rng.uniform(0, 3, (n, 1)) * 0.05), target + away * 3.0)
    d = np.where(inside[:, None], away, target - o)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    t_max = np.where(np.arange(n) % 8 == 5, rng.uniform(0.5, 8.0, n), np.inf)
    return o.astype(np.float32), d.astype(np.float32), t_max.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_model(kind, bend, xform):
    """(curves, (o, d, t_max), float64 model, float32 model) of a case; the models are curve_model.intersect_many's dicts"""
    curves = case_curves(kind, bend, xform)
    o, d, t_max = case_rays(kind, bend, xform)
    m64 = curve_model.intersect_many(curves, o, d, t_max, np.float64)
    m32 = curve_model.intersect_many(curves, o, d, t_max, np.float32)
    return curves, (o, d, t_max), m64, m32


def case_spread(kind, bend, xform):
    """max |float32 - float64| of t, u, v over the rays of the case that both runs hit on the same record and that are not left out"""
    _, _, m64, m32 = case_model(kind, bend, xform)
    keep = (m64["margin"] >= MARGIN) & m64["hit"] & m32["hit"] & (m64["prim"] == m32["prim"])
    return {k: float(np.abs(m32[k][keep].astype(np.float64) - m64[k][keep]).max()) for k in ("t", "u", "v")}


# ---------------------------------------------------------------------------------------------------------------------
# edge cases of the hit test
# ---------------------------------------------------------------------------------------------------------------------
EDGE_N_RAYS = 2048
EDGE_MARGINS = (1e-3, 0.02, 0.05)   # a case takes the smallest at which the float32 model gives the float64 model's verdicts
LOOP = np.array([(0.0, 0.0, 0.0), (1.5, 1.0, 0.2), (-0.5, 1.0, -0.2), (1.0, 0.0, 0.0)])
CP01 = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.9, -0.6, 0.3), (1.2, 0.2, -0.2)])
CP23 = np.array([(0.0, 0.0, 0.0), (0.3, 0.8, 0.1), (1.2, 0.2, -0.2), (1.2, 0.2, -0.2)])
RIBBON_NORMALS = np.array([(0.0, 0.0, 1.0), (0.0, 1.0, 1.0)])
LOOP_NORMALS = np.array([(1.0, 0.2, 0.1), (0.2, 1.0, 0.1)])


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tangent(cp, u):
    u = u[:, None]
    return 3 * ((1 - u) ** 2 * (cp[1] - cp[0]) + 2 * u * (1 - u) * (cp[2] - cp[1]) + u * u * (cp[3] - cp[2]))


def aimed_rays(cp, m, width, n, seed, scale=1.0):
    """case_rays' families about the curve m * cp: the 1.5-width aim in units of `width`, the distances of `scale`"""
    rng = np.random.default_rng(seed)
    on_curve = _bezier(cp, rng.uniform(-0.05, 1.05, n)) @ m[:3, :3].T + m[:3, 3]
    unit = _unit(rng, n)
    target = on_curve + unit * (rng.uniform(0, 1.5, (n, 1)) * width)
    away = _unit(rng, n)
    inside = np.arange(n) % 4 == 3
    o = np.where(inside[:, None], on_curve + unit * (rng.uniform(0, 3, (n, 1)) * width), target + away * (3.0 * scale))
    d = np.where(inside[:, None], away, target - o)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    t_max = np.where(np.arange(n) % 8 == 5, rng.uniform(0.5, 8.0, n) * scale, np.inf)
    return o.astype(np.float32), d.astype(np.float32), t_max.astype(np.float32)


def chord_rays(cp, m, n, seed, jitter=0.01, back=3.0):
    """rays from one point of the curve's neighbourhood through another, the origin `back` before the first"""
    rng = np.random.default_rng(seed)
    pa = _bezier(cp, rng.uniform(0, 1, n)) @ m[:3, :3].T + m[:3, 3] + _unit(rng, n) * jitter
    pb = _bezier(cp, rng.uniform(0, 1, n)) @ m[:3, :3].T + m[:3, 3] + _unit(rng, n) * jitter
    w = pb - pa
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    d = w * rng.uniform(0.5, 2.0, (n, 1))
    return (pa - back * w).astype(np.float32), d.astype(np.float32), np.full(n, np.inf, np.float32)


def grazing_rays(cp, m, width, aim, n, seed):
    """rays at 0.2 to 5 degrees to the curve's tangent at a point of it, through a point within `aim` widths of that point"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.02, 0.98, n)
    on_curve = _bezier(cp, u) @ m[:3, :3].T + m[:3, 3]
    tan = _tangent(cp, u) @ m[:3, :3].T
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    side = np.cross(tan, _unit(rng, n))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    ang = np.radians(rng.uniform(0.2, 5.0, (n, 1)))
    w = tan * np.cos(ang) + side * np.sin(ang)
    target = on_curve + _unit(rng, n) * (rng.uniform(0, aim, (n, 1)) * width)
    d = w * rng.uniform(0.5, 2.0, (n, 1))
    t_max = np.where(np.arange(n) % 8 == 5, rng.uniform(0.5, 8.0, n), np.inf)
    return (target - 3.0 * w).astype(np.float32), d.astype(np.float32), t_max.astype(np.float32)


def _placed(how):
    m = transform("rigid")
    if how == "far":
        m[:3, 3] += (1000.0, -800.0, 600.0)
        return m, 1.0
    s = dict(small=1e-3, large=1e3)[how]
    return np.diag([s, s, s, 1.0]) @ m, s


def _edge(name, kind):
    """(curve records, (o, d, t_max)) of an edge case"""
    normals = RIBBON_NORMALS if kind == "ribbon" else None
    seed = 10 * (zlib.crc32(name.encode()) % 100000) + TYPES.index(kind) + SEED_SHIFT.get((name, kind), 0)
    mk = lambda cp, w0, w1, xf, sd, nrm=normals, rev=False: scenes.curve(cp, w0, w1, type=kind, normals=nrm, to_world=xf, material=0,
                                                                         split_depth=sd, reverse_orientation=rev)
    rigid = transform("rigid")
    if name == "thin":
        return mk(BENT, 2e-3, 1e-3, rigid, 0), aimed_rays(BENT, rigid, 2e-3, EDGE_N_RAYS, seed)
    if name == "hair":
        return mk(BENT, 1e-4, 5e-5, rigid, 0), aimed_rays(BENT, rigid, 1e-4, EDGE_N_RAYS, seed)
    if name == "clamp":
        return mk(BENT, 1.2e-5, 1.2e-5, np.eye(4), 0), aimed_rays(BENT, np.eye(4), 1.2e-5, 1024, seed)
    if name == "taper":   # aimed_rays' u runs over [-0.05, 1.05]: past the tip of zero width
        return mk(BENT, 0.05, 0.0, transform("scaled"), 2, rev=True), aimed_rays(BENT, transform("scaled"), 0.05, EDGE_N_RAYS, seed)
    if name == "loop":   # the loop and its chords lie near the xy plane: a ribbon facing z would be seen edge-on
        return mk(LOOP, 0.05, 0.03, transform("mirrored"), 3, nrm=LOOP_NORMALS if kind == "ribbon" else None), chord_rays(LOOP, transform("mirrored"), EDGE_N_RAYS, seed)
    if name == "loop_tmax":   # half of the loop's rays, stopped between their first and their second crossing where they have two
        curves, (o, d, _), _, _, _ = edge_model("loop", kind)
        t = np.sort(np.stack([np.where(r["hit"], r["t"], np.inf) for r in (curve_model.intersect(rec, o, d) for rec in curves)]), axis=0)
        two = np.isfinite(t[1])
        f = np.random.default_rng(seed).uniform(0.25, 0.75, len(o))
        first, second = np.where(two, t[0], 0.0), np.where(two, t[1], 0.0)
        t_max = np.where(two, first + f * (second - first), np.inf)
        half = np.arange(len(o)) % 2 == 0
        return curves, (o[half], d[half], t_max[half].astype(np.float32))
    if name == "u_range":
        rec = mk(BENT, 0.05, 0.02, rigid, 0)
        rec["u_min"], rec["u_max"] = 0.13, 0.71
        return rec, aimed_rays(BENT, rigid, 0.05, EDGE_N_RAYS, seed)
    if name == "split3":   # the same curve in eight records: each refines its own part to its own depth
        return mk(BENT, 0.05, 0.02, rigid, 3), aimed_rays(BENT, rigid, 0.05, EDGE_N_RAYS, seed)
    if name in ("cp0_is_cp1", "cp2_is_cp3"):
        cp = CP01 if name == "cp0_is_cp1" else CP23
        return mk(cp, 0.05, 0.02, rigid, 1), aimed_rays(cp, rigid, 0.05, EDGE_N_RAYS, seed)
    if name in ("normals_equal", "normals_square"):
        nrm = np.array([(0.0, 0.0, 1.0), (0.0, 0.0, 2.0) if name == "normals_equal" else (0.0, 1.0, 0.0)])
        return mk(BENT, 0.05, 0.02, rigid, 1, nrm=nrm), aimed_rays(BENT, rigid, 0.05, EDGE_N_RAYS, seed)
    if name in ("grazing_straight", "grazing_bent"):
        cp = STRAIGHT if name == "grazing_straight" else BENT
        # a ribbon seen along its axis is |n . d| wide: aimed closer, so that a tenth of its rays still hit
        return mk(cp, 0.05, 0.02, rigid, 1), grazing_rays(cp, rigid, 0.05, GRAZING_AIM[kind], EDGE_N_RAYS, seed)
    if name == "parallel_exact":   # d x (cp3 - cp0) == 0 exactly: the look_at frame comes from coordinate_system(d)
        rng = np.random.default_rng(seed)
        o = np.concatenate([np.full((EDGE_N_RAYS, 1), -1.0), rng.uniform(-0.05, 0.05, (EDGE_N_RAYS, 2))], axis=1)
        d = np.broadcast_to((1.5, 0.0, 0.0), o.shape)
        return mk(STRAIGHT, 0.05, 0.02, np.eye(4), 0), (o.astype(np.float32), d.astype(np.float32), np.full(EDGE_N_RAYS, np.inf, np.float32))
    if name == "parallel_chord":   # d along the float32 chord: the cross product is a rounding residue, or nothing at all
        rng = np.random.default_rng(seed)
        # (0.37 and not 0.5: half the chord is exact in float32, and the product would vanish in float64 as well)
        d = np.broadcast_to((np.float32(0.37) * (BENT[3] - BENT[0]).astype(np.float32)).astype(np.float64), (EDGE_N_RAYS, 3))
        target = _bezier(BENT, rng.uniform(-0.05, 1.05, EDGE_N_RAYS)) + _unit(rng, EDGE_N_RAYS) * (rng.uniform(0, PARALLEL_AIM[kind], (EDGE_N_RAYS, 1)) * 0.05)
        o = target - d * rng.uniform(2.0, 5.0, (EDGE_N_RAYS, 1))
        return mk(BENT, 0.05, 0.02, np.eye(4), 0), (o.astype(np.float32), d.astype(np.float32), np.full(EDGE_N_RAYS, np.inf, np.float32))
    if name.startswith("placed_"):
        m, s = _placed(name[len("placed_"):])
        return mk(BENT, 0.05, 0.02, m, 1), aimed_rays(BENT, m, 0.05 * s, EDGE_N_RAYS, seed, scale=s)
    raise KeyError(name)


GRAZING_AIM = dict(flat=1.5, cylinder=1.5, ribbon=0.3)
PARALLEL_AIM = dict(flat=1.5, cylinder=1.5, ribbon=0.5)   # likewise: along the chord most of this ribbon is seen nearly edge-on
# A ribbon 1.2e-5 wide seen nearly edge-on is 1e-6 wide or less, and the margin, which is stated in units of that width, no longer
# covers the float32 rounding of the ray-space position (1e-7): with the seed the formula gives, three of the 1024 rays differ
# between the model's float32 and float64 runs at margin 1e-3, two at 0.02 and one at 0.05. The next seed at which the rule
# settles on a margin is taken instead.
SEED_SHIFT = {("clamp", "ribbon"): 3}
ALL_TYPES, NOT_CYLINDER, RIBBON_ONLY = TYPES, ("flat", "ribbon"), ("ribbon",)
# The share of rays a margin may leave out. A ray's closest approach is aimed uniformly over 1.5 widths, so a band of `margin`
# widths on either side of the strip's edge holds about 2 margin / 1.5 of the rays: 0.027 at 0.02 and 0.067 at 0.05. At 1e-3 the
# 18 cases' cap stands.
EDGE_MAX_LEFT_OUT = {1e-3: MAX_LEFT_OUT, 0.02: 0.04, 0.05: 0.08}
# name: (types, the refinement depth some ray must reach or None, whether v is compared)
EDGE_NAMES = {
    "thin": (ALL_TYPES, 7, True),
    "hair": (ALL_TYPES, 9, True),
    # the position's float32 rounding is about 1 % of this width: the model's own float32 v is off by 0.19-0.59 of the strip
    "clamp": (NOT_CYLINDER, 10, False),
    "taper": (ALL_TYPES, None, True),
    "loop": (ALL_TYPES, None, True),
    "loop_tmax": (ALL_TYPES, None, True),
    "u_range": (ALL_TYPES, None, True),
    "split3": (ALL_TYPES, None, True),
    "cp0_is_cp1": (ALL_TYPES, None, True),
    "cp2_is_cp3": (ALL_TYPES, None, True),
    "normals_equal": (RIBBON_ONLY, None, True),
    "normals_square": (RIBBON_ONLY, None, True),
    "grazing_straight": (ALL_TYPES, None, True),
    "grazing_bent": (ALL_TYPES, None, True),
    "parallel_exact": (ALL_TYPES, None, True),
    "parallel_chord": (ALL_TYPES, None, True),
    "placed_far": (ALL_TYPES, None, True),
    "placed_small": (ALL_TYPES, None, True),
    "placed_large": (ALL_TYPES, None, True),
}
EDGE_CASES = [(name, kind) for name, spec in EDGE_NAMES.items() for kind in spec[0]]


@functools.lru_cache(maxsize=None)
def edge_model(name, kind):
    """(curves, (o, d, t_max), float64 model, float32 model, margin) of an edge case; margin: the smallest of EDGE_MARGINS at
    which the float32 run gives the float64 run's verdict on every ray kept, None where none does"""
    curves, (o, d, t_max) = _edge(name, kind)
    m64 = curve_model.intersect_many(curves, o, d, t_max, np.float64)
    m32 = curve_model.intersect_many(curves, o, d, t_max, np.float32)
    margin = None
    for mg in EDGE_MARGINS:
        keep = m64["margin"] >= mg
        if np.array_equal(m32["hit"][keep], m64["hit"][keep]):
            margin = mg
            break
    return curves, (o, d, t_max), m64, m32, margin


GAMMA3 = 3 * 2.0 ** -24 / (1 - 3 * 2.0 ** -24)


def origin_push(rec, o, d):
    """How far along the ray, in t, the device moves the object-space origin before the hit test (shape_object_ray; Ray::from,
    geometry.rs:1089-1093): dt = |d| . o_err / |d|^2 with o_err = gamma(3) times the sum of the absolute terms of each coordinate
    of world_to_object * o. curve_model.py does not model it. It is 1e-7 of the origin's distance, in units of the time the ray
    takes to travel that far: nothing for a curve near the world's origin, 1e-3 / |d| for one 1400 away, which is 0.05 of the
    thinnest width there."""
    mi = np.asarray(np.asarray(rec).reshape(-1)[0]["to_object"], dtype=np.float64).reshape(4, 4)
    o, d = o.astype(np.float64), d.astype(np.float64)
    o_err = ((np.abs(mi[:3, :3])[None, :, :] * np.abs(o)[:, None, :]).sum(-1) + np.abs(mi[:3, 3])) * GAMMA3
    od = d @ mi[:3, :3].T
    return (np.abs(od) * o_err).sum(-1) / (od * od).sum(-1)


@functools.lru_cache(maxsize=None)
def edge_keep(name, kind):
    """(the rays of an edge case that are kept, the device's origin push dt of every ray). Left out: a ray whose margin is
    below the case's, and a ray whose verdict the push may turn, since the device tests 0 <= t - dt <= t_max - dt + dt, that is a
    hit within 2 dt of the origin (it falls behind the moved origin) or, without the t_max, within 2 dt of a finite t_max (the
    moved origin brings it into range). Twice dt: dt itself is a float32 sum of bounds. The device reports t - dt."""
    curves, (o, d, t_max), m64, _, margin = edge_model(name, kind)
    dt = origin_push(curves, o, d)
    keep = m64["margin"] >= margin
    keep &= ~(m64["hit"] & (m64["t"] <= 2 * dt))
    stopped = np.isfinite(t_max)
    if stopped.any():
        free = curve_model.intersect_many(curves, o[stopped], d[stopped])
        close = free["hit"] & (np.abs(free["t"] - t_max[stopped].astype(np.float64)) <= 2 * dt[stopped])
        keep[np.flatnonzero(stopped)[close]] = False
    return keep, dt


def edge_spread(name, kind):
    """case_spread of an edge case at its own margin"""
    _, _, m64, m32, margin = edge_model(name, kind)
    keep = (m64["margin"] >= margin) & m64["hit"] & m32["hit"] & (m64["prim"] == m32["prim"])
    if not keep.any():
        return dict(t=0.0, u=0.0, v=0.0)
    return {k: float(np.abs(m32[k][keep].astype(np.float64) - m64[k][keep]).max()) for k in ("t", "u", "v")}


# what test_gpu_curve_shading.py puts on a curve to see the side of its normal and the turn of its tangents
GLASS = dict(kr=(1.0, 1.0, 1.0), kt=(1.0, 1.0, 1.0), eta=1.5, roughness=0.3)
METAL = dict(eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), u_roughness=0.05, v_roughness=0.4)
GLOSSY_RTOL = 2e-3


# ---------------------------------------------------------------------------------------------------------------------
# the surface at the model's nearest hit, and what a light gives there
# ---------------------------------------------------------------------------------------------------------------------
def surface_of(curves, o, d, t_max, m64):
    """n, p, dpdu (world space), width (hit_width) and p_err (p_error = 2 hit_width through |to_world|'s linear part) of the hit
    the float64 aggregate reports, ray by ray; zeros where it reports none"""
    R = len(o)
    s = dict(n=np.zeros((R, 3)), p=np.zeros((R, 3)), dpdu=np.zeros((R, 3)), width=np.zeros(R), p_err=np.zeros((R, 3)))
    for j, rec in enumerate(np.asarray(curves).reshape(-1)):
        mine = m64["hit"] & (m64["prim"] == j)
        if not mine.any():
            continue
        r = curve_model.intersect(rec, o[mine], d[mine], np.broadcast_to(t_max, (R,))[mine])
        for k in ("n", "p", "dpdu", "width"):
            s[k][mine] = r[k]
        lin = np.abs(np.asarray(rec["to_world"], dtype=np.float64).reshape(4, 4)[:3, :3])
        s["p_err"][mine] = 2 * r["width"][:, None] * lin.sum(1)[None, :]
    return s


def leaving(curves, surf, sel, wi, t_max=np.inf):
    """intersect_many of the rays that leave the hits `sel` along wi ((n, 3), need not be unit) from where spawn_ray starts
    them: p moved along n, to wi's side, by |n| . p_error"""
    n, p = surf["n"][sel], surf["p"][sel]
    side = np.sign((n * wi).sum(-1))[:, None]
    start = p + n * side * (np.abs(n) * surf["p_err"][sel]).sum(-1, keepdims=True)
    return curve_model.intersect_many(curves, start, wi, t_max)


def local_frame(surf, sel, flip=False, turn=False):
    """the shading frame make_frame builds: ss = normalize(dpdu), ts = n x ss, n. flip: the normal reversed (what an inverted
    orientation flag would give); turn: the tangents turned by 90 degrees about n (what a wrong dpdu would give)"""
    n = -surf["n"][sel] if flip else surf["n"][sel]
    ss = surf["dpdu"][sel] / np.linalg.norm(surf["dpdu"][sel], axis=1, keepdims=True)
    ts = np.cross(n, ss)
    if turn:
        ss, ts = ts, -ss
    return ss, ts, n


def point_light_radiance(surf, sel, d, p_light, intensity, f_of, flip=False, turn=False):
    """f(wo, wi) I |wi . n| / r^2 at the hits `sel` of the rays with directions d, f_of(wo_local, wi_local) -> (n, 3)"""
    ss, ts, n = local_frame(surf, sel, flip, turn)
    wo = -d[sel].astype(np.float64)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    wi = np.asarray(p_light, dtype=np.float64) - surf["p"][sel]
    r2 = (wi * wi).sum(-1)
    wi = wi / np.sqrt(r2)[:, None]
    to_local = lambda w: np.stack([(w * ss).sum(-1), (w * ts).sum(-1), (w * n).sum(-1)], -1)
    f = f_of(to_local(wo), to_local(wi))
    return f * np.asarray(intensity, dtype=np.float64) * (np.abs((wi * n).sum(-1)) / r2)[:, None]


ORIENT_W = (0.3, 0.2)   # a wide strip: most of the rays aimed at its middle hit
ORIENTATIONS = [("rigid", False), ("rigid", True), ("mirrored", False), ("mirrored", True), ("scaled", False)]
# In the curve's own space. The eye and the front light stand some 100 degrees apart as the curve sees them: the half vector then
# meets both at about 50 degrees, past glass's critical angle (41.8), where reflection seen from inside (total) and from outside
# (a few per cent) differ; nearer the normal the two Fresnel terms agree and a reversed normal would not show in reflection.
ORIENT_EYE, ORIENT_LIGHTS = (-1.0, 0.1, 1.5), dict(front=(2.4, 0.4, 1.2), behind=(0.9, 0.6, -2.0))
ORIENT_INTENSITY = (6.0, 5.0, 4.0)


@functools.lru_cache(maxsize=None)
def orient_case(kind, xform, reverse, n=256):
    """BENT as one record of `kind` under transform(xform) with the given reverse_orientation, n rays from about ORIENT_EYE to
    points near its axis, the float64 model and its surface. Returns (curves, (o, d), model, surface, {name: light position})."""
    m = transform(xform)
    curves = scenes.curve(BENT, *ORIENT_W, type=kind, normals=RIBBON_NORMALS if kind == "ribbon" else None, to_world=m, material=0,
                          split_depth=0, reverse_orientation=reverse)
    rng = np.random.default_rng(900 + 10 * TYPES.index(kind) + 2 * TRANSFORMS.index(xform) + int(reverse))
    to_world = lambda p: np.asarray(p) @ m[:3, :3].T + m[:3, 3]
    target = to_world(_bezier(BENT, rng.uniform(0.1, 0.9, n)) + _unit(rng, n) * (rng.uniform(0, 0.3, (n, 1)) * ORIENT_W[1]))
    o = to_world(np.asarray(ORIENT_EYE) + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    d = (target - o).astype(np.float32)
    model = curve_model.intersect_many(curves, o, d)
    lights = {k: to_world(v) for k, v in ORIENT_LIGHTS.items()}
    return curves, (o, d), model, surface_of(curves, o, d, np.inf, model), lights


def orient_kept(kind, xform, reverse, light):
    """the rays of orient_case that hit clear of a decision and whose way to the light the model decides clearly, and of those
    the ones it finds open"""
    curves, (o, d), model, surf, lights = orient_case(kind, xform, reverse)
    h = model["hit"] & (model["margin"] >= 0.05)
    to_light = lights[light] - surf["p"][h]
    way = leaving(curves, surf, h, to_light, 1.0 - 1e-4)
    keep = np.flatnonzero(h)[way["margin"] >= 0.05]
    return keep, ~way["hit"][way["margin"] >= 0.05]
