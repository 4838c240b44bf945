"""Cases shared by test_bxdf_model.py (the float64 model alone) and test_gpu_bxdfs.py (the device held to the model):
descriptors with their models, the direction tables, the grazing band of glossy transmission and the furnace cases."""
import numpy as np

from pbrt_hip import scenes
import bxdf_model as bm
from glossy_cases import _unit

W, Z = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
KR, KT = (0.9, 0.8, 0.7), (0.7, 0.8, 0.9)


def _glass(name, kr, kt, eta, a, remap=False):
    au, av = a if isinstance(a, tuple) else (a, a)
    return (name, scenes.rough_glass(kr, kt, eta, au, av, remap=remap), bm.rough_glass(kr, kt, eta, au, av, remap=remap))


# (name, descriptor, model): rough glass at eta 1.5 and 1.33, alpha 0.05, 0.2 and (0.15, 0.6), with Kr black, Kt black and neither;
# substrate isotropic and anisotropic; Oren-Nayar at sigma 20 and 60 degrees
CASES = []
for eta in (1.5, 1.33):
    for a in (0.05, 0.2, (0.15, 0.6)):
        tag = f"glass_eta{eta:g}_a{a if not isinstance(a, tuple) else 'niso'}"
        CASES += [_glass(tag + "_both", KR, KT, eta, a), _glass(tag + "_kr0", Z, KT, eta, a), _glass(tag + "_kt0", KR, Z, eta, a)]
CASES += [
    ("substrate_iso", scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.2, remap=False), bm.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.2, remap=False)),
    ("substrate_aniso", scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.15, 0.6, remap=False),
     bm.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.15, 0.6, remap=False)),
    ("substrate_remap", scenes.substrate((0.2, 0.2, 0.2), (0.6, 0.5, 0.4), 0.1, 0.3), bm.substrate((0.2, 0.2, 0.2), (0.6, 0.5, 0.4), 0.1, 0.3)),
    ("oren_sigma20", scenes.matte_sigma((0.6, 0.5, 0.4), 20.0), bm.matte_sigma((0.6, 0.5, 0.4), 20.0)),
    ("oren_sigma60", scenes.matte_sigma((0.6, 0.5, 0.4), 60.0), bm.matte_sigma((0.6, 0.5, 0.4), 60.0)),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


BAND = 0.05          # the grazing band of glossy transmission: min(|wo.wh|, |wi.wh|) < BAND on the generalised half vector
BAND_MAX_SHARE = 0.15


def in_band(m, wo, wi):
    """float64: pairs across the surface whose microfacet is seen at grazing incidence from either side"""
    if m.kind != bm.GLASS or "trans" not in m.lobes:
        return np.zeros(len(wo), bool)
    _, ow, iw, _ = bm.trans_parts(m, wo, wi)
    return (wo[:, 2] * wi[:, 2] <= 0) & (np.minimum(np.abs(ow), np.abs(iw)) < BAND)


def special_directions():
    """normal incidence, grazing, wi = -wo, wo.z = 0, from both sides"""
    g = 1e-3
    s = [(0, 0, 1), (0, 0, -1), _unit(np.array([1.0, 0, g])), _unit(np.array([0, 1.0, -g])), (1, 0, 0), (0, -1, 0),
         _unit(np.array([0.6, 0.0, 0.8])), _unit(np.array([0.3, -0.5, -0.81])), _unit(np.array([-0.7, 0.7, 0.14]))]
    s = np.array([np.asarray(v, np.float64) for v in s])
    wo = np.repeat(s, len(s), 0)
    wi = np.tile(s, (len(s), 1))
    wo = np.concatenate([wo, s])
    wi = np.concatenate([wi, -s])
    return wo, wi


def directions(m, n, seed):
    """(wo, wi, u) float32: random pairs with wo on both sides, a third of the wi near the mirror direction, a third near the
    refracted direction of a random microfacet normal (where the transmission lobe lives), then the special directions"""
    rng = np.random.default_rng(seed)
    wo = _unit(rng.normal(size=(n, 3)))
    wi = _unit(rng.normal(size=(n, 3)))
    k = n // 3
    wi[:k] = _unit(wo[:k] * np.array([-1, -1, 1]) + 0.15 * rng.normal(size=(k, 3)))
    if m.kind == bm.GLASS:
        o = wo[k:2 * k]
        wh = _unit(np.array([0, 0, 1.0]) + 0.3 * rng.normal(size=(k, 3))) * np.where(o[:, 2:3] < 0, -1, 1)
        ow = np.sum(o * wh, -1)
        eta = np.where(o[:, 2] > 0, 1 / m.eta, m.eta)
        s2 = eta * eta * np.maximum(0, 1 - ow * ow)
        okr = (s2 < 1) & (ow > 0)
        wt = -o * eta[:, None] + wh * (eta * ow - np.sqrt(np.where(okr, 1 - s2, 0)))[:, None]
        wi[k:2 * k] = np.where(okr[:, None], _unit(wt + 0.05 * rng.normal(size=(k, 3))), wi[k:2 * k])
    so, si = special_directions()
    wo, wi = np.concatenate([wo, so]).astype(np.float32), np.concatenate([wi, si]).astype(np.float32)
    u = rng.random((len(wo), 2)).astype(np.float32)
    return wo, wi, u


# ---- furnace (alpha >= 0.2): (name, descriptor, model, camera below the plane) ----
FURNACE = [
    ("glass_above", scenes.rough_glass(KR, KT, 1.5, 0.2, remap=False), bm.rough_glass(KR, KT, 1.5, 0.2, remap=False), False),
    ("glass_below", scenes.rough_glass(KR, KT, 1.5, 0.2, remap=False), bm.rough_glass(KR, KT, 1.5, 0.2, remap=False), True),
    ("substrate", scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.25, remap=False), bm.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.25, remap=False), False),
    ("oren", scenes.matte_sigma((0.6, 0.5, 0.4), 40.0), bm.matte_sigma((0.6, 0.5, 0.4), 40.0), False),
]


def furnace_wo(below):
    t = np.radians(50.0)
    return np.array([0.0, -np.sin(t), -np.cos(t) if below else np.cos(t)])


# ---- chi^2: (name, theta_o degrees); every lobe set at two wo, for glass one above and one below the surface ----
CHI2_DESC = {"glass_both": scenes.rough_glass(KR, KT, 1.5, 0.45, remap=False), "glass_kr0": scenes.rough_glass(Z, KT, 1.33, 0.25, remap=False),
             "glass_kt0": scenes.rough_glass(KR, Z, 1.5, 0.3, remap=False), "substrate": scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.3, remap=False),
             "oren": scenes.matte_sigma((0.6, 0.5, 0.4), 40.0)}
CHI2_MODEL = {"glass_both": bm.rough_glass(KR, KT, 1.5, 0.45, remap=False), "glass_kr0": bm.rough_glass(Z, KT, 1.33, 0.25, remap=False),
              "glass_kt0": bm.rough_glass(KR, Z, 1.5, 0.3, remap=False), "substrate": bm.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.3, remap=False),
              "oren": bm.matte_sigma((0.6, 0.5, 0.4), 40.0)}
CHI2 = [("glass_both", 35.0), ("glass_both", 140.0), ("glass_kr0", 60.0), ("glass_kr0", 155.0), ("glass_kt0", 50.0), ("glass_kt0", 130.0),
        ("substrate", 35.0), ("substrate", 75.0), ("oren", 20.0), ("oren", 110.0)]
# The sampler as pbrt-v3 has it (the device's), 10^6 samples as test_gpu_glossy.py::test_sampler_chi2. Left out: glass_kr0 seen
# from above. The rational fit of slope_y in trowbridge_reitz_sample11 stops at |slope| = 7.26 (bxdf_model.FIT_MAX_SLOPE), so
# 1.09e-3 of the visible normals are never returned (slope_tail_mass). With the transmission lobe alone and wo above, every
# sample crosses the surface, so those normals' directions fall into bins of their own that expect 10 to 20 samples and get
# none (nothing lands under the horizon, nothing is shared with a second lobe): in float64 with the fit p = 1.5e-43 at 10^6
# samples, 0.40 with the exact inverse (test_bxdf_model.py::test_sampler_chi2 holds that case's pdf with the exact inverse, and
# test_fit_breaks_transmission_alone_from_above asserts the figure). As D65 / glossy_cases.CHI2 leave out metal_aniso.
N_FIT = 1_000_000
CHI2_FIT_LEFT_OUT = ("glass_kr0", 60.0)
CHI2_FIT = [c for c in CHI2 if c != CHI2_FIT_LEFT_OUT]


def chi2_wo(theta_o):
    t = np.radians(theta_o)
    return np.array([np.sin(t) * np.cos(0.7), np.sin(t) * np.sin(0.7), np.cos(t)])
