"""The hair rows the tests share: descriptors (scenes.hair), their float64 models (hair_model.py) and the query points."""
import numpy as np

import hair_model as hm
from pbrt_hip import scenes

BROWN = (0.84, 1.39, 2.74)  # eumelanin 2: sigma_a of brown hair
# name, scenes.hair's arguments
CASES = [
    ("bm0.1_bn0.1_white_a0", dict(sigma_a=0.0, beta_m=0.1, beta_n=0.1, alpha=0.0)),
    ("bm0.1_bn0.9_brown_a2", dict(sigma_a=BROWN, beta_m=0.1, beta_n=0.9, alpha=2.0)),
    ("bm0.1_bn0.3_black_a-3", dict(eumelanin=8.0, beta_m=0.1, beta_n=0.3, alpha=-3.0)),
    ("bm0.1_bn0.3_brown_eta1.2", dict(sigma_a=BROWN, beta_m=0.1, beta_n=0.3, alpha=2.0, eta=1.2)),
    ("defaults", dict()),
    ("bm0.3_bn0.3_white_a0", dict(sigma_a=0.0, alpha=0.0)),
    ("bm0.3_bn0.1_black_a2", dict(eumelanin=8.0, beta_n=0.1)),
    ("bm0.3_bn0.9_color_a-3_eta1.2", dict(color=(0.8, 0.5, 0.2), beta_n=0.9, alpha=-3.0, eta=1.2)),
    ("bm0.5_bn0.5_pheomelanin_a0", dict(eumelanin=0.3, pheomelanin=1.1, beta_m=0.5, beta_n=0.5, alpha=0.0)),
    ("bm0.9_bn0.1_brown_a-3", dict(sigma_a=BROWN, beta_m=0.9, beta_n=0.1, alpha=-3.0)),
    ("bm0.9_bn0.9_white_a2", dict(color=1.0, beta_m=0.9, beta_n=0.9)),
    ("bm0.9_bn0.3_white_eta1.2_a0", dict(sigma_a=0.0, beta_m=0.9, beta_n=0.3, alpha=0.0, eta=1.2)),
]
DESCS = [scenes.hair(**kw) for _, kw in CASES]


def model_of(desc):
    """the float64 model of a scenes.hair descriptor: the absorption of its parametrisation from the float32 fields"""
    f32 = lambda x: float(np.float32(x))
    bn = f32(desc["beta_n"])
    if desc["absorption"] == scenes.HAIR_SIGMA_A:
        sa = [f32(x) for x in desc["sigma_a"]]
    elif desc["absorption"] == scenes.HAIR_COLOR:
        sa = hm.sigma_a_from_color([f32(x) for x in desc["color"]], bn)
    else:
        sa = hm.sigma_a_from_melanin(f32(desc["eumelanin"]), f32(desc["pheomelanin"]))
    # the device holds sigma_a rounded to float32: the model starts from those
    sa = np.asarray(sa, np.float64).astype(np.float32)
    return hm.HairModel(sigma_a=sa, eta=desc["eta"], beta_m=desc["beta_m"], beta_n=bn, alpha=desc["alpha"])


MODELS = [model_of(d) for d in DESCS]
N_POINTS = 4096
N_ZERO = 8  # points with wo.z == 0


def _sphere(rng, n):
    z = rng.uniform(-1.0, 1.0, n)
    p = rng.uniform(0.0, 2.0 * np.pi, n)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(p), r * np.sin(p), z], axis=1)


def points(seed, n=N_POINTS):
    """(h, wo, wi, u) in float32: uniform directions; h uniform in [-1, 1] after the fixed -1, 0, 1; the last N_ZERO wo have z == 0"""
    rng = np.random.default_rng(seed)
    wo, wi = _sphere(rng, n), _sphere(rng, n)
    a = rng.uniform(0.0, 2.0 * np.pi, N_ZERO)
    wo[-N_ZERO:] = np.stack([np.cos(a), np.sin(a), np.zeros(N_ZERO)], axis=1)
    h = rng.uniform(-1.0, 1.0, n)
    h[:3] = (-1.0, 0.0, 1.0)
    u = rng.random((n, 2))
    wo, wi = wo.astype(np.float32), wi.astype(np.float32)
    wo[-N_ZERO:, 2] = 0.0
    return h.astype(np.float32), wo, wi, np.minimum(u.astype(np.float32), np.float32(hm.ONE_MINUS_EPSILON))


def left_out(wo, wi):
    """the points the device is not compared at: eta' divides by cos(theta_o) (|w.x| > 0.999), and |wo.z| < 1e-3"""
    return (np.abs(wo[:, 0]) > 0.999) | (np.abs(wi[:, 0]) > 0.999) | (np.abs(wo[:, 2]) < 1e-3)


LEFT_OUT_MAX_SHARE = 0.02
