"""The curve cases test_curve_model.py and test_gpu_curves.py share: each a curve of one type, straight or bent, under a rigid, a
scaled or a mirrored transform, split into two segment records, with a batch of rays aimed at it from outside and from inside
its bound. A case's float64 and float32 model runs are computed once and kept."""
import functools

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
