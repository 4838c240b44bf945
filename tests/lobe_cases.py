"""Cases shared by test_lobe_model.py (the float64 model and the host's lobe lists) and test_gpu_lobe_materials.py (the device held
to the model): uber / translucent / mix descriptors with their models, how they are installed into a scene's material table,
the direction tables and grazing band (bxdf_cases'), the furnace cases and the descriptors pbrt_hip_scene_set_lobe_material
refuses."""
import numpy as np

from pbrt_hip import scenes
import bxdf_cases
import bxdf_model as bm
import lobe_model as lm
from bxdf_cases import BAND, BAND_MAX_SHARE  # noqa: F401 (the GPU test's rules are test_gpu_bxdfs.py's)

MATTE = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
KD = (0.5, 0.4, 0.3)

# Operand rows of the mixes: (how the scene gets the row, its model). "row": a PbrtMaterial tuple for scenes._materials;
# "desc": a PbrtMaterialDesc over a matte row; "lobe": a PbrtLobeMaterialDesc over a matte row.
_METAL = ("row", scenes.metal((0.2, 0.9, 1.1), (3.0, 2.5, 2.0), 0.2), lm.metal((0.2, 0.9, 1.1), (3.0, 2.5, 2.0), 0.2))
_MATTE = ("row", (scenes.MAT_MATTE, (0.6, 0.5, 0.4), (0, 0, 0), 1.0), lm.matte((0.6, 0.5, 0.4)))
_PLASTIC = ("row", scenes.plastic((0.4, 0.3, 0.2), (0.3, 0.3, 0.3), 0.15), lm.plastic((0.4, 0.3, 0.2), (0.3, 0.3, 0.3), 0.15))
_MIRROR = ("row", (scenes.MAT_MIRROR, (0.9, 0.8, 0.7), (0, 0, 0), 1.0), lm.mirror((0.9, 0.8, 0.7)))
_OREN = ("desc", scenes.matte_sigma((0.6, 0.5, 0.4), 40.0), lm.from_bxdf_model(bm.matte_sigma((0.6, 0.5, 0.4), 40.0)))
_GLASS = ("desc", scenes.rough_glass((0.8, 0.8, 0.8), (0.7, 0.8, 0.9), 1.5, 0.3, remap=False),
          lm.from_bxdf_model(bm.rough_glass((0.8, 0.8, 0.8), (0.7, 0.8, 0.9), 1.5, 0.3, remap=False)))
_SUBSTRATE = ("desc", scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.25, remap=False),
              lm.from_bxdf_model(bm.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.25, remap=False)))
_UBER_SPEC_KW = dict(kd=(0.3, 0.4, 0.5), ks=0.0, kr=0.4, kt=0.5, opacity=0.75, eta=1.4)
_UBER_SPEC = ("lobe", scenes.uber(**_UBER_SPEC_KW), lm.uber(**_UBER_SPEC_KW))


def _single(name, fn_s, fn_m, **kw):
    return dict(name=name, operands=[], desc=lambda rows: fn_s(**kw), model=fn_m(**kw))


def _mix(name, a, b, amount):
    return dict(name=name, operands=[a, b], desc=lambda rows: scenes.mix(rows[0], rows[1], amount), model=lm.mix(a[2], b[2], amount))


# Every lobe kind is in at least one list, specular beside non-specular, one transmissive specular lobe beside another (uber_all),
# and every Fresnel (none, (1, eta), (1.5, 1), conductor).
CASES = [
    _single("uber_defaults", scenes.uber, lm.uber),
    _single("uber_all", scenes.uber, lm.uber, kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5, eta=1.5, u_roughness=0.2, v_roughness=0.3),
    _single("uber_opacity0", scenes.uber, lm.uber, opacity=0.0),
    _single("uber_specular_only", scenes.uber, lm.uber, kd=0.0, ks=0.0, kr=0.6, kt=0.7, eta=1.33),
    _single("uber_aniso_noremap", scenes.uber, lm.uber, kd=0.2, ks=(0.5, 0.6, 0.7), u_roughness=0.15, v_roughness=0.4, remap=False),
    _single("translucent_defaults", scenes.translucent, lm.translucent, roughness=0.3),
    _single("translucent_transmit0", scenes.translucent, lm.translucent, kd=KD, transmit=0.0),
    _single("translucent_ks0", scenes.translucent, lm.translucent, kd=KD, ks=0.0, reflect=0.3, transmit=0.7),
    _single("translucent_rough", scenes.translucent, lm.translucent, kd=KD, ks=(0.6, 0.5, 0.4), reflect=(0.2, 0.5, 0.8), transmit=(0.8, 0.5, 0.2),
            roughness=0.35, remap=False),
    _mix("mix_matte_metal", _MATTE, _METAL, 0.3),
    _mix("mix_plastic_uber", _PLASTIC, _UBER_SPEC, (0.2, 0.5, 0.8)),
    _mix("mix_glass_substrate", _GLASS, _SUBSTRATE, 0.6),
    _mix("mix_oren_mirror", _OREN, _MIRROR, 0.5),
]
NAMES = [c["name"] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


def install(sc, cases):
    """sc with the cases' rows appended to its material table: per case its operand rows, then one matte row that becomes the
    lobe row. Returns (scene dict, the lobe row of each case)."""
    sc = dict(sc)
    mats = [tuple(m) for m in sc["materials"].tolist()] if len(sc["materials"]) else []
    mats = [(int(t), tuple(kd), tuple(kt), float(e)) for t, kd, kt, e in mats]
    mdescs, ldescs, rows = dict(sc.get("material_descs") or {}), dict(sc.get("lobe_descs") or {}), []
    for c in cases:
        ops = []
        for how, what, _ in c["operands"]:
            ops.append(len(mats))
            mats.append(what if how == "row" else MATTE)
            if how == "desc":
                mdescs[ops[-1]] = what
            elif how == "lobe":
                ldescs[ops[-1]] = what
        rows.append(len(mats))
        mats.append(MATTE)
        ldescs[rows[-1]] = c["desc"](ops)
    sc["materials"] = scenes._materials(mats)
    sc["material_descs"], sc["lobe_descs"] = mdescs, ldescs
    return sc, rows


def in_band(m, wo, wi):
    return bxdf_cases.in_band(m.trans_shim(), wo, wi)


def directions(m, n, seed):
    """bxdf_cases.directions: random pairs, a third near the mirror direction, a third near a refracted direction when there is a
    glossy transmission lobe, then the special directions"""
    return bxdf_cases.directions(m.trans_shim(), n, seed)


furnace_wo = bxdf_cases.furnace_wo
chi2_wo = bxdf_cases.chi2_wo

# ---- furnace: (name, case, camera below the plane); alphas >= 0.2 ----
FURNACE = [
    ("uber_opacity_half", _single("f0", scenes.uber, lm.uber, kd=KD, ks=0.0, opacity=0.5), False),
    ("uber_all_above", _single("f1", scenes.uber, lm.uber, kd=KD, ks=0.3, kr=0.2, kt=0.3, eta=1.5, u_roughness=0.3, v_roughness=0.3, remap=False), False),
    ("uber_all_below", _single("f2", scenes.uber, lm.uber, kd=KD, ks=0.3, kr=0.2, kt=0.3, eta=1.5, u_roughness=0.3, v_roughness=0.3, remap=False), True),
    ("translucent", _single("f3", scenes.translucent, lm.translucent, kd=KD, ks=0.4, roughness=0.3, remap=False), False),
    ("mix_matte_uber", _mix("f4", _MATTE, _UBER_SPEC, 0.4), False),
]


def furnace_reference(m, wo):
    """(albedo, its quadrature error: the change under a doubled grid)"""
    a, b = lm.albedo(m, wo), lm.albedo(m, wo, 256, 1024)
    return b, np.abs(a - b)


# ---- refusals of pbrt_hip_scene_set_lobe_material on a table of rows
#      0 matte, 1 metal, 2 smooth glass, 3 Disney, 4 a mix of 0 and 1, 5 uber with 5 lobes, 6 matte:
#      (row, descriptor, what pbrt_hip_last_error names) ----
REFUSAL_ROWS = [MATTE, _METAL[1], (scenes.MAT_GLASS, (1, 1, 1), (1, 1, 1), 1.5), MATTE, MATTE, MATTE, MATTE]
_FIVE = scenes.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5)
REFUSED = [
    (6, None, "null desc"),
    (7, scenes.uber(), "out of range"),
    (-1, scenes.uber(), "out of range"),
    (6, dict(scenes.uber(), type=7), "unknown lobe material type"),
    (6, scenes.uber(kd=(0.5, -0.1, 0.5)), "Kd"),
    (6, scenes.uber(ks=(np.nan, 0.1, 0.5)), "Ks"),
    (6, scenes.uber(kr=(np.inf, 0.1, 0.5)), "Kr"),
    (6, scenes.uber(kt=-1.0), "Kt"),
    (6, scenes.uber(opacity=-0.5), "opacity"),
    (6, scenes.uber(eta=0.0), "eta"),
    (6, scenes.uber(eta=np.nan), "eta"),
    (6, scenes.uber(u_roughness=-0.1), "roughness"),
    (6, scenes.uber(v_roughness=np.inf), "roughness"),
    (6, scenes.uber(u_roughness=0.0, remap=False), "roughness 0 without remapping"),
    (6, scenes.translucent(reflect=-0.1), "reflect"),
    (6, scenes.translucent(transmit=np.nan), "transmit"),
    (6, scenes.translucent(kd=-1.0), "Kd"),
    (6, scenes.translucent(roughness=0.0, remap=False), "roughness 0 without remapping"),
    (6, scenes.mix(0, 1, -0.5), "amount"),
    (6, scenes.mix(0, 1, np.nan), "amount"),
    (6, scenes.mix(0, 7, 0.5), "material_b out of range"),
    (6, scenes.mix(-1, 0, 0.5), "material_a out of range"),
    (6, scenes.mix(3, 0, 0.5), "material_a: a Disney row"),
    (6, scenes.mix(0, 4, 0.5), "material_b is a mix row"),
    (6, scenes.mix(2, 0, 0.5), "material_a: smooth glass.*an uber row with Kr, Kt"),
    (6, scenes.mix(5, 5, 0.5), "more than 8 lobes"),
]
# accepted where a neighbour is refused: no microfacet lobe carries the zero alpha
ACCEPTED = [scenes.uber(ks=0.0, u_roughness=0.0, remap=False), scenes.translucent(ks=0.0, roughness=0.0, remap=False),
            scenes.uber(kd=(2.0, 1.5, 1.0)), scenes.mix(5, 0, 0.5)]


def refusal_scene(sc):
    sc = dict(sc)
    sc["materials"] = scenes._materials(REFUSAL_ROWS)
    sc["disney_descs"] = {3: scenes.disney((0.8, 0.5, 0.3))}
    sc["lobe_descs"] = {4: scenes.mix(0, 1, 0.5), 5: _FIVE}
    return sc
