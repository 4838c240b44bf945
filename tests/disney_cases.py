"""Cases shared by test_disney_model.py (the float64 model alone) and test_gpu_disney.py (the device held to the model):
Disney descriptors with their models, the direction tables, the grazing band of glossy transmission, the chi^2 and furnace
cases and the descriptors pbrt_hip_scene_set_disney_material refuses."""
import numpy as np

from pbrt_hip import scenes
import bxdf_cases
import bxdf_model as bm
import disney_model as dm
from bxdf_cases import BAND, BAND_MAX_SHARE  # noqa: F401 (the GPU test's rules are test_gpu_bxdfs.py's)

C = (0.8, 0.5, 0.3)


def _case(name, color=C, **kw):
    d = scenes.disney(color, **kw)
    return (name, d, dm.Disney(d))


# (name, descriptor, model). Every lobe is on at least once, and each optional lobe alone with the reflection lobe (lobe 4):
# the diffuse pair in `defaults`, the clearcoat in `metal_clearcoat`, glossy transmission in `spec_trans1` (dw = 0),
# LambertianTransmission in `thin_metal`; sheen only exists beside the diffuse lobes.
CASES = [
    _case("defaults"),
    _case("metallic1", metallic=1.0),
    _case("aniso0.8", anisotropic=0.8, roughness=0.4),
    _case("sheen_tint0", sheen=1.0, sheen_tint=0.0),
    _case("sheen_tint1", sheen=0.8, sheen_tint=1.0),
    _case("clearcoat_gloss0", clearcoat=1.0, clearcoat_gloss=0.0),
    _case("clearcoat_gloss1", clearcoat=0.7, clearcoat_gloss=1.0),
    _case("metal_clearcoat", metallic=1.0, clearcoat=1.0, clearcoat_gloss=0.5),
    _case("spec_trans0.7", spec_trans=0.7, roughness=0.4),
    _case("spec_trans1", spec_trans=1.0, roughness=0.3),
    _case("thin_dt0", thin=True, flatness=0.5, diff_trans=0.0, spec_trans=0.5),
    _case("thin_dt1.5", thin=True, flatness=0.5, diff_trans=1.5, spec_trans=0.5),
    _case("thin_metal", thin=True, metallic=1.0, diff_trans=1.2),
    _case("roughness0", roughness=0.0),
    _case("roughness1", roughness=1.0, specular_tint=0.6),
    _case("black", color=(0.0, 0.0, 0.0), sheen=0.5, spec_trans=0.3),
    _case("everything", thin=True, metallic=0.3, eta=1.4, roughness=0.35, specular_tint=0.5, anisotropic=0.5, sheen=0.6, sheen_tint=0.7,
          clearcoat=0.8, clearcoat_gloss=0.4, spec_trans=0.4, flatness=0.3, diff_trans=0.8),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


def in_band(m, wo, wi):
    """bxdf_cases.in_band for the transmission lobe of a Disney model"""
    return bxdf_cases.in_band(m.trans_shim(), wo, wi)


def directions(m, n, seed):
    """bxdf_cases.directions: random pairs, a third near the mirror direction, a third near a refracted direction when there is a
    transmission lobe, then the special directions"""
    return bxdf_cases.directions(m.trans_shim(), n, seed)


# ---- chi^2: (name, theta_o degrees). Roughness >= 0.4 and clearcoat gloss 0 (g = 0.1), so the 16 x 32 bins resolve every lobe;
# every lobe is in one of the sets, the transmissive ones seen from both sides. Transmission is never the only lobe.
CHI2_DESC = {
    "opaque": scenes.disney(C, roughness=0.5, sheen=0.5, clearcoat=1.0, clearcoat_gloss=0.0),
    "metal_cc": scenes.disney(C, metallic=1.0, roughness=0.5, anisotropic=0.5, clearcoat=1.0, clearcoat_gloss=0.0),
    "trans": scenes.disney(C, spec_trans=0.7, roughness=0.5),
    "trans_dw0": scenes.disney(C, spec_trans=1.0, roughness=0.6),
    "thin": scenes.disney(C, thin=True, flatness=0.5, diff_trans=1.0, spec_trans=0.5, roughness=0.6, sheen=0.3),
}
CHI2_MODEL = {k: dm.Disney(v) for k, v in CHI2_DESC.items()}
CHI2 = [("opaque", 35.0), ("opaque", 110.0), ("metal_cc", 50.0), ("trans", 140.0), ("trans_dw0", 30.0), ("trans_dw0", 150.0), ("thin", 45.0),
        ("thin", 125.0)]
# The sampler as pbrt-v3 has it (the device's), 10^6 samples. Left out: trans_dw0 seen from above, for the reason
# bxdf_cases.CHI2_FIT_LEFT_OUT gives. Transmission is not the only lobe there, but it is the only one under the surface when the
# row is not thin: the 1.09e-3 of the visible normals beyond the rational fit's last slope (bxdf_model.FIT_MAX_SLOPE) refract into
# bins of the lower hemisphere that expect samples and get none. In float64 with the fit p = 2.2e-12 at 10^6 samples, 0.35 with
# the exact inverse (test_disney_model.py::test_sampler_chi2 holds that case's pdf with the exact inverse, and
# test_fit_breaks_transmission_from_above asserts the figure); no wo above the surface mends it (theta_o 10 .. 75 degrees:
# p 1e-11 .. 2e-3 for this row and for `trans`). Seen from below, and thin (LambertianTransmission fills the far side), it passes.
N_FIT = 1_000_000
CHI2_FIT_LEFT_OUT = ("trans_dw0", 30.0)
CHI2_FIT = [c for c in CHI2 if c != CHI2_FIT_LEFT_OUT]
chi2_wo = bxdf_cases.chi2_wo

# ---- furnace: (name, descriptor, model, camera below the plane); roughness >= 0.3 and clearcoat gloss 0 ----
_OPAQUE = scenes.disney(C, roughness=0.5, sheen=0.5, clearcoat=1.0, clearcoat_gloss=0.0)
_TRANS = scenes.disney(C, spec_trans=0.7, roughness=0.5)
_THIN = scenes.disney(C, thin=True, flatness=0.5, diff_trans=1.0, spec_trans=0.5, roughness=0.5)
FURNACE = [("opaque_above", _OPAQUE, dm.Disney(_OPAQUE), False), ("opaque_below", _OPAQUE, dm.Disney(_OPAQUE), True),
           ("trans_above", _TRANS, dm.Disney(_TRANS), False), ("trans_below", _TRANS, dm.Disney(_TRANS), True),
           ("thin_above", _THIN, dm.Disney(_THIN), False), ("thin_below", _THIN, dm.Disney(_THIN), True)]
furnace_wo = bxdf_cases.furnace_wo


def furnace_reference(m, wo):
    """(albedo, its quadrature error: the change under a doubled grid)"""
    a, b = dm.albedo(m, wo), dm.albedo(m, wo, 256, 1024)
    return b, np.abs(a - b)


# ---- refusals: (row, descriptor, what pbrt_hip_last_error names); rows 0 and 1 exist ----
def _d(**kw):
    return scenes.disney(kw.pop("color", C), **kw)


REFUSED = [
    (0, None, "null desc"),
    (2, _d(), "out of range"),
    (-1, _d(), "out of range"),
    (0, _d(color=(0.5, -0.1, 0.5)), "color"),
    (0, _d(color=(0.5, np.nan, 0.5)), "color"),
    (0, _d(color=(np.inf, 0.5, 0.5)), "color"),
    (0, _d(eta=0.0), "eta must be > 0"),
    (0, _d(eta=-1.5), "eta"),
    (0, _d(eta=np.nan), "eta"),
    (0, _d(diff_trans=2.5), "diff_trans must be <= 2"),
    (0, _d(diff_trans=-0.1), "diff_trans"),
    (0, _d(sheen=-1.0), "sheen"),
    (0, _d(sheen=np.inf), "sheen"),
    (0, _d(clearcoat=-0.5), "clearcoat"),
    (0, _d(clearcoat=np.nan), "clearcoat"),
] + [(0, _d(**{k: 1.5}), f"{k} must be <= 1") for k in ("metallic", "roughness", "specular_tint", "anisotropic", "sheen_tint", "clearcoat_gloss",
                                                        "spec_trans", "flatness")] + \
    [(0, _d(**{k: -0.25}), k) for k in ("metallic", "roughness", "specular_tint", "anisotropic", "sheen_tint", "clearcoat_gloss", "spec_trans",
                                        "flatness")]
ACCEPTED = [_d(sheen=3.0), _d(clearcoat=2.5), _d(diff_trans=2.0), _d(eta=0.8), _d(roughness=0.0), _d(metallic=1.0, spec_trans=1.0),
            _d(color=(0.0, 0.0, 0.0)), _d(color=(2.0, 1.5, 1.0))]
