"""The lobe-list BSDF's float64 model (lobe_model.py) held to itself and to hand-written lists, and the host's context-free lobe
listing (pbrt_hip_material_lobes) held to the model: the lists of uber / translucent / mix stated literally, the library's
float32 values against the model's as32(), reciprocity, the sampler against the pdf and against the albedo, the lossless cases,
mix(a, a), the refusals the entry point can see, and the ABI layout. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import lobe_model as lm
from lobe_cases import BAND_MAX_SHARE, CASES, KD, directions, in_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda *v: tuple(float(np.float32(c)) for c in v)  # noqa: E731
ONE = (1.0, 1.0, 1.0)


def _lit(m):
    return [l.literal() for l in m.lobes]


def _prod(*factors):
    """a colour product formed in float32, left to right"""
    out = np.ones(3, np.float32)
    for f in factors:
        out = out * np.asarray(f if not np.isscalar(f) else (f,) * 3, np.float32)
    return tuple(float(c) for c in out)


# ---- the lists, stated literally: (kind, fresnel, scale, colour) in order, and the BSDF's eta ----
def test_lobe_lists_are_pbrt_v3s():
    R, T, D, G, S = lm.REFLECTION, lm.TRANSMISSION, lm.DIFFUSE, lm.GLOSSY, lm.SPECULAR
    assert lm.TYPE == {lm.LAMBERT_R: R | D, lm.LAMBERT_T: T | D, lm.OREN: R | D, lm.SPEC_R: R | S, lm.SPEC_T: T | S, lm.MICRO_R: R | G,
                       lm.MICRO_T: T | G, lm.BLEND: R | G}
    # opacity 1: no pass-through lobe, eta is the material's
    m = lm.uber()
    assert _lit(m) == [(lm.LAMBERT_R, lm.NOOP, ONE, f32(0.25, 0.25, 0.25)), (lm.MICRO_R, lm.DIELECTRIC, ONE, f32(0.25, 0.25, 0.25))]
    assert m.eta == 1.5 and (m.lobes[1].eta_i, m.lobes[1].eta_t) == (1.0, 1.5)
    assert m.lobes[1].ax == pytest.approx(lm.mm.roughness_to_alpha(0.1)) and m.lobes[1].ay == m.lobes[1].ax
    # opacity 0: the pass-through lobe alone, SpecularTransmission(1, 1, 1), eta 1
    m = lm.uber(opacity=0.0)
    assert _lit(m) == [(lm.SPEC_T, lm.DIELECTRIC, ONE, ONE)] and m.eta == 1.0 and (m.lobes[0].eta_i, m.lobes[0].eta_t) == (1.0, 1.0)
    # opacity 0.5 with all four colours: five lobes in pbrt-v3's order, two of them transmissive and specular
    m = lm.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5, eta=1.4)
    assert _lit(m) == [(lm.SPEC_T, lm.DIELECTRIC, ONE, f32(0.5, 0.5, 0.5)), (lm.LAMBERT_R, lm.NOOP, ONE, _prod(0.5, KD)),
                       (lm.MICRO_R, lm.DIELECTRIC, ONE, _prod(0.5, 0.3)), (lm.SPEC_R, lm.DIELECTRIC, ONE, _prod(0.5, 0.2)),
                       (lm.SPEC_T, lm.DIELECTRIC, ONE, _prod(0.5, 0.3))]
    assert m.eta == 1.0 and m.lobes[4].eta_t == 1.4 and m.lobes[0].eta_t == 1.0
    assert lm.num_components(m) == 5 and lm.num_components(m, lm.NON_SPECULAR) == 2
    assert lm.num_components(m, T | S) == 2 and lm.num_components(m, R | S) == 1
    # black Kd: the Lambertian lobe is left out
    m = lm.uber(kd=0.0)
    assert _lit(m) == [(lm.MICRO_R, lm.DIELECTRIC, ONE, f32(0.25, 0.25, 0.25))]
    # colours are clamped to [0, 1] before the products; per-channel opacity
    m = lm.uber(kd=(2.0, 0.5, 0.0), ks=0.0, opacity=(1.0, 0.5, 0.0))
    assert _lit(m) == [(lm.SPEC_T, lm.DIELECTRIC, ONE, (0.0, 0.5, 1.0)), (lm.LAMBERT_R, lm.NOOP, ONE, (1.0, 0.25, 0.0))]
    # translucent: defaults, transmit 0, Ks 0, both black
    m = lm.translucent()
    q = f32(0.125, 0.125, 0.125)
    assert _lit(m) == [(lm.LAMBERT_R, lm.NOOP, ONE, q), (lm.LAMBERT_T, lm.NOOP, ONE, q), (lm.MICRO_R, lm.DIELECTRIC, ONE, q),
                       (lm.MICRO_T, lm.DIELECTRIC, ONE, q)]
    assert m.eta == 1.5 and all((l.eta_i, l.eta_t) == (1.0, 1.5) for l in m.lobes[2:])
    m = lm.translucent(transmit=0.0)
    assert [l[0] for l in _lit(m)] == [lm.LAMBERT_R, lm.MICRO_R]
    m = lm.translucent(kd=KD, ks=0.0, reflect=0.3, transmit=0.7)
    assert _lit(m) == [(lm.LAMBERT_R, lm.NOOP, ONE, _prod(0.3, KD)), (lm.LAMBERT_T, lm.NOOP, ONE, _prod(0.7, KD))]
    assert _lit(lm.translucent(reflect=0.0, transmit=0.0)) == []
    # a mix of matte and metal: a's lobes under s1, b's under clamp(1 - s1); eta is a's
    a, b = lm.matte((0.6, 0.5, 0.4)), lm.metal((0.2, 0.9, 1.1), (3.0, 2.5, 2.0), 0.2)
    m = lm.mix(a, b, 0.3)
    s2 = float(np.float32(1) - np.float32(0.3))
    assert _lit(m) == [(lm.LAMBERT_R, lm.NOOP, f32(0.3, 0.3, 0.3), f32(0.6, 0.5, 0.4)), (lm.MICRO_R, lm.CONDUCTOR, (s2, s2, s2), ONE)]
    # a black scale is kept
    assert len(lm.mix(a, b, 1.0).lobes) == 2 and lm.mix(a, b, 1.0).lobes[1].scale.tolist() == [0.0, 0.0, 0.0]


# ---- the library's lists against the model's ----
def _library_list(c):
    ops = []
    for how, what, _ in c["operands"]:
        if how == "row":
            t, kd, kt, eta = what
            ops.append(pbrt_hip.material_lobes(scenes.material_row(t, kd, kt, eta)))
        else:
            ops.append(pbrt_hip.material_lobes(what))
    return pbrt_hip.material_lobes(c["desc"]([0, 1]), *ops)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_library_lists_equal_the_models(i):
    """kinds, order, types and Fresnel equal; every float32 the library returns equals the model's as32() value"""
    lobes, eta = _library_list(CASES[i])
    m = CASES[i]["model"].as32()
    assert len(lobes) == m.n and float(eta) == m.eta
    for got, want in zip(lobes, m.lobes):
        assert (got["kind"], got["type"], got["fresnel"]) == (want.kind, want.type, want.fresnel)
        for name in ("scale", "r", "s", "eta", "k"):
            assert tuple(float(v) for v in got[name]) == tuple(getattr(want, name)), name
        for name in ("ax", "ay", "eta_i", "eta_t", "A", "B"):
            assert float(got[name]) == getattr(want, name), name


# ---- the model against itself ----
def _pairs(m, n, seed):
    wo, wi, u = directions(m, n, seed)  # float32 tables: unit to 6e-8, so normalised again in float64
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)  # noqa: E731
    return unit(wo.astype(np.float64)), unit(wi.astype(np.float64)), u


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_band_share(i):
    """the grazing band of glossy transmission holds at most BAND_MAX_SHARE of each case's table (the GPU test's rule)"""
    m = CASES[i]["model"]
    wo, wi, _ = _pairs(m, 3000, 300 + i)
    assert in_band(m, wo, wi).mean() <= BAND_MAX_SHARE


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_reflection_side_is_reciprocal(i):
    m = CASES[i]["model"]
    wo, wi, _ = _pairs(m, 2000, 40 + i)
    same = (wo[:, 2] * wi[:, 2] > 0) & (np.abs(wo[:, 2]) > 1e-3) & (np.abs(wi[:, 2]) > 1e-3)
    a, b = lm.bsdf_f(m, wo[same], wi[same]), lm.bsdf_f(m, wi[same], wo[same])
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(a).max()))


@pytest.mark.parametrize("flags", [lm.ALL, lm.NON_SPECULAR], ids=["all", "non_specular"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_sampler_returns_the_pdf(i, flags):
    """pdf_s == pdf(wo, wi_s) and f_s == f(wo, wi_s) for non-specular picks; a specular pick has the lobe's pdf over the number of
    matching lobes; the picked lobe is the floor(u0 n)-th matching one"""
    m = CASES[i]["model"]
    wo, _, u = _pairs(m, 2000, 70 + i)
    wi, f, pdf, ok, types, index = lm.bsdf_sample_f(m, wo, u, flags)
    nm = lm.num_components(m, flags)
    if nm == 0:
        assert not ok.any()
        return
    match = [k for k, l in enumerate(m.lobes) if (l.type & flags) == l.type]
    want = np.array(match)[np.minimum(np.floor(u[:, 0].astype(np.float64) * nm), nm - 1).astype(int)]
    assert np.array_equal(index[ok], want[ok])
    spec = ok & ((types & lm.SPECULAR) != 0)
    ns = ok & ~spec
    if flags == lm.NON_SPECULAR:
        assert not spec.any()
    if ns.any():
        # (the sampler's own pdf belongs to the half vector it drew; pdf() rebuilds it from wo + wi: 1e-6 covers that in float64
        # away from grazing wo)
        sel = ns & (np.abs(wo[:, 2]) > 1e-2) & ~in_band(m, wo, np.where(ok[:, None], wi, 1.0))
        np.testing.assert_allclose(pdf[sel], lm.bsdf_pdf(m, wo[sel], wi[sel], flags), rtol=1e-6)
        np.testing.assert_allclose(f[sel], lm.bsdf_f(m, wo[sel], wi[sel], flags), rtol=1e-9, atol=1e-300)
    if spec.any():
        assert np.all(pdf[spec] == 1.0 / nm)
        refl = spec & ((types & lm.REFLECTION) != 0)
        np.testing.assert_allclose(wi[refl], wo[refl] * np.array([-1.0, -1.0, 1.0]))
        assert np.all(wi[spec & ~refl][:, 2] * wo[spec & ~refl][:, 2] < 0)


ALBEDO = ["uber_all", "uber_defaults", "translucent_rough", "mix_plastic_uber", "mix_glass_substrate"]


@pytest.mark.parametrize("name", ALBEDO)
@pytest.mark.parametrize("theta_o", [35.0, 130.0])
def test_sampler_albedo(name, theta_o):
    """the Monte-Carlo albedo of sample_f(BSDF_ALL), f |cos| / pdf, within 4 standard errors of albedo()"""
    m = CASES[[c["name"] for c in CASES].index(name)]["model"]
    t = np.radians(theta_o)
    wo1 = np.array([np.sin(t) * np.cos(0.7), np.sin(t) * np.sin(0.7), np.cos(t)])
    n = 200_000
    u = np.random.default_rng(3).random((n, 2))
    wi, f, pdf, ok, _, _ = lm.bsdf_sample_f(m, np.broadcast_to(wo1, (n, 3)).copy(), u)
    w = np.where(ok[:, None], f * np.abs(wi[:, 2:3]) / np.where(ok, pdf, 1.0)[:, None], 0.0)
    mean, se = w.mean(0), w.std(0) / np.sqrt(n)
    ref = lm.albedo(m, wo1)
    print(f"{name} {theta_o}: MC {mean} +- {se}, quadrature {ref}")
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-9)


@pytest.mark.parametrize("name,m", [("uber_kd1_opacity_half", lm.uber(kd=1.0, ks=0.0, opacity=0.5)),
                                    ("translucent_kd1", lm.translucent(kd=1.0, ks=0.0, reflect=0.5, transmit=0.5))])
@pytest.mark.parametrize("theta_o", [20.0, 75.0, 140.0])
def test_lossless_cases(name, m, theta_o):
    """albedo 1 to the quadrature's own error (the change under a doubled grid)"""
    t = np.radians(theta_o)
    wo = np.array([np.sin(t), 0.0, np.cos(t)])
    a, b = lm.albedo(m, wo), lm.albedo(m, wo, 256, 1024)
    err = np.abs(a - b)
    print(f"{name} {theta_o}: albedo {b}, quadrature error {err}")
    assert np.all(np.abs(b - 1.0) <= err + 1e-12)


@pytest.mark.parametrize("name", ["uber_all", "translucent_rough"])
def test_mix_identity(name):
    """mix(a, a, s) has a's f and pdf: the scales s and 1 - s add to 1 per lobe pair, the pdf is averaged over twice the lobes"""
    a = CASES[[c["name"] for c in CASES].index(name)]["model"]
    if 2 * a.n > 8:
        a = lm.Bsdf(a.lobes[1:], a.eta)  # (uber_all has five lobes)
    wo, wi, _ = _pairs(a, 2000, 11)
    for s in (0.25, (0.1, 0.5, 0.9)):
        m = lm.mix(a, a, s)
        # (s and 1 - s are float32: their sum is 1 to 6e-8, so the comparison is against the scales the mix really has)
        tot = (m.lobes[0].scale + m.lobes[a.n].scale)
        np.testing.assert_allclose(lm.bsdf_f(m, wo, wi), lm.bsdf_f(a, wo, wi) * tot, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(lm.bsdf_pdf(m, wo, wi), lm.bsdf_pdf(a, wo, wi), rtol=1e-12, atol=1e-300)
        assert np.all(np.abs(tot - 1.0) <= 6e-8)


# ---- what the context-free entry point refuses ----
def test_entry_point_refusals():
    five = pbrt_hip.material_lobes(scenes.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5))
    four = pbrt_hip.material_lobes(scenes.translucent())
    assert len(five[0]) == 5 and len(four[0]) == 4
    assert len(pbrt_hip.material_lobes(scenes.mix(0, 1, 0.5), four, four)[0]) == 8
    with pytest.raises(pbrt_hip.PbrtHipError, match="more than 8 lobes"):
        pbrt_hip.material_lobes(scenes.mix(0, 1, 0.5), five, four)
    with pytest.raises(pbrt_hip.PbrtHipError, match="smooth glass.*an uber row with Kr, Kt"):
        pbrt_hip.material_lobes(scenes.material_row(scenes.MAT_GLASS, (1, 1, 1), (1, 1, 1), 1.5))
    with pytest.raises(pbrt_hip.PbrtHipError, match="smooth glass"):
        pbrt_hip.material_lobes(scenes.rough_glass((1, 1, 1), (1, 1, 1), 1.5, 0.0))
    for desc, why in ((scenes.uber(kd=(0.5, -0.1, 0.5)), "Kd"), (scenes.uber(eta=0.0), "eta"), (scenes.uber(opacity=np.nan), "opacity"),
                      (scenes.uber(u_roughness=0.0, remap=False), "roughness 0 without remapping"),
                      (scenes.translucent(transmit=-1.0), "transmit"), (scenes.translucent(roughness=np.inf), "roughness"),
                      (dict(scenes.uber(), type=9), "unknown lobe material type"),
                      (scenes.material_row(scenes.MAT_METAL, (0, 1, 1), (1, 1, 1), 0.1), "metal eta"),
                      (scenes.matte_sigma((0.5, 0.5, 0.5), -1.0), "sigma")):
        with pytest.raises(pbrt_hip.PbrtHipError, match=why):
            pbrt_hip.material_lobes(desc)
    with pytest.raises(pbrt_hip.PbrtHipError, match="amount"):
        pbrt_hip.material_lobes(scenes.mix(0, 1, -0.5), four, four)
    # exactly one description
    L = pbrt_hip.lib()
    out, n, eta, why = (pbrt_hip.Lobe * 8)(), ctypes.c_int32(), ctypes.c_float(), ctypes.c_char_p()
    rc = L.pbrt_hip_material_lobes(None, None, None, None, 0, 1.0, None, 0, ctypes.addressof(out), ctypes.byref(n), ctypes.byref(eta),
                                   ctypes.byref(why))
    assert rc == 1 and b"exactly one" in why.value


# ---- ABI ----
def test_abi_layout(tmp_path):
    """PbrtLobeMaterialDesc and PbrtLobe against a compiled C probe: sizes, offsets and the enums"""
    probe = [("PbrtLobeMaterialDesc", pbrt_hip.LobeMaterialDesc), ("PbrtLobe", pbrt_hip.Lobe)]
    items = []
    for cname, cls in probe:
        items.append(f"sizeof({cname})")
        items += [f"offsetof({cname}, {k})" for k, _ in cls._fields_]
    enums = ["PBRT_LOBEMAT_UBER", "PBRT_LOBEMAT_TRANSLUCENT", "PBRT_LOBEMAT_MIX", "PBRT_LOBE_LAMBERTIAN_REFLECTION", "PBRT_LOBE_FRESNEL_BLEND",
             "PBRT_FRESNEL_CONDUCTOR"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_hip.h"\nint main(void) {\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in items + enums) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, cls in probe:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, k).offset for k, _ in cls._fields_]
    want += [scenes.LOBEMAT_UBER, scenes.LOBEMAT_TRANSLUCENT, scenes.LOBEMAT_MIX, scenes.LOBE_LAMBERTIAN_REFLECTION, scenes.LOBE_FRESNEL_BLEND,
             scenes.FRESNEL_CONDUCTOR]
    assert got == want
    assert ctypes.sizeof(pbrt_hip.Lobe) == 96 and ctypes.sizeof(pbrt_hip.LobeMaterialDesc) == 124
