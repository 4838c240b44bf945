"""The float64 model of the Disney material (disney_model.py) held to what a BSDF has to satisfy, before any device is compared
with it: its sampler against its pdf (chi^2, with the exact slope inverse and with pbrt-v3's fit as the device has it), pdf
normalisation against the sampler's success rate, reciprocity, the lobes written out by hand, the furnace references'
convergence; and the host side of pbrt_hip_scene_set_disney_material: the descriptor's validation, layout and the export."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import disney_model as dm
import microfacet_model as mm
from disney_cases import ACCEPTED, BAND_MAX_SHARE, CASES, CHI2, CHI2_FIT, CHI2_FIT_LEFT_OUT, CHI2_MODEL, FURNACE, N_FIT, REFUSED, chi2_wo, directions, furnace_reference, furnace_wo, in_band
from glossy_cases import _unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pbrt_hip.h")
IDS = [f"{c[0]}-{c[1]:g}" for c in CHI2]


def _chi2(m, theta_o, seed, exact_slope):
    wo = chi2_wo(theta_o)
    u = np.random.default_rng(seed).random((N_FIT, 2))
    wi, _, _, ok, _, _ = dm.bsdf_sample_f(m, np.broadcast_to(wo, (N_FIT, 3)), u, exact_slope=exact_slope)
    return dm.chi2_p(m, wo, wi, ok, N_FIT)


@pytest.mark.parametrize("name,theta_o", CHI2, ids=IDS)
def test_sampler_chi2(name, theta_o):
    """sample_f against the integrated pdf, 10^6 samples, the visible-normal sampler with the exact slope inverse: the lobes'
    pdfs, the clearcoat's sampler and the lobe choice"""
    p, chi2, bins, stray = _chi2(CHI2_MODEL[name], theta_o, 170 + CHI2.index((name, theta_o)), True)
    print(f"{name} {theta_o}: chi2 {chi2:.5g} over {bins} bins, p {p:.3g}")
    assert stray == 0, "samples where the pdf has no mass"
    assert p > 1e-3, (chi2, bins, p)


@pytest.mark.parametrize("name,theta_o", CHI2_FIT, ids=[f"{c[0]}-{c[1]:g}" for c in CHI2_FIT])
def test_sampler_chi2_with_the_fit(name, theta_o):
    """the cases, seed and sample count of test_gpu_disney.py::test_sampler_chi2 with pbrt-v3's slope fit in float64;
    disney_cases.CHI2_FIT says which case is left out and why"""
    p, chi2, bins, stray = _chi2(CHI2_MODEL[name], theta_o, 7, False)
    print(f"{name} {theta_o} with the fit: chi2 {chi2:.5g} over {bins} bins, p {p:.3g}")
    assert stray == 0 and p > 1e-3, (chi2, bins, p)


def test_fit_breaks_transmission_from_above():
    """the case disney_cases.CHI2_FIT leaves out: the fit's missing slope tail is resolved under the surface, where a row that
    is not thin has no other lobe; the exact inverse passes (test_sampler_chi2)"""
    name, theta_o = CHI2_FIT_LEFT_OUT
    p, chi2, bins, _ = _chi2(CHI2_MODEL[name], theta_o, 7, False)
    print(f"{name} {theta_o} with the fit: chi2 {chi2:.4g} over {bins} bins, p {p:.3g}")
    assert p < 1e-3


@pytest.mark.parametrize("name,theta_o", CHI2, ids=IDS)
def test_pdf_integral_is_the_sampler_success_rate(name, theta_o):
    """the pdf integrates to at most 1, and to the share of samples that return a direction (the rest: reflected under the
    horizon, total internal reflection, microfacets seen from behind), within the sampling error"""
    m, wo, n = CHI2_MODEL[name], chi2_wo(theta_o), 400_000
    total, finer = dm.pdf_integral(m, wo), dm.pdf_integral(m, wo, 256, 1024)
    assert abs(total - finer) < 2e-4, (total, finer)
    assert 0 < finer <= 1 + 1e-4
    u = np.random.default_rng(3).random((n, 2))
    ok = dm.bsdf_sample_f(m, np.broadcast_to(wo, (n, 3)), u, exact_slope=True)[3]
    rate, se = ok.mean(), np.sqrt(max(ok.mean() * (1 - ok.mean()), 1e-6) / n)
    print(f"{name} {theta_o}: integral {finer:.5f}, success rate {rate:.5f} +- {se:.2g}")
    assert abs(rate - finer) < 4 * se + 2e-4, (rate, finer, se)


def _pairs(n, seed, across=False):
    rng = np.random.default_rng(seed)
    wo = _unit(rng.normal(size=(n, 3)))
    wi = _unit(rng.normal(size=(n, 3)))
    wi[:, 2] = np.abs(wi[:, 2]) * np.sign(wo[:, 2]) * (-1 if across else 1)
    return wo, wi


OPAQUE = [i for i, c in enumerate(CASES) if "trans" not in c[2].lobes and "lambert_t" not in c[2].lobes]


@pytest.mark.parametrize("i", OPAQUE, ids=[CASES[i][0] for i in OPAQUE])
def test_reciprocity(i):
    m = CASES[i][2]
    wo, wi = _pairs(4000, 11 + i)
    a, b = dm.bsdf_f(m, wo, wi), dm.bsdf_f(m, wi, wo)
    assert np.count_nonzero(a) > 3000
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * np.abs(a).max())


@pytest.mark.parametrize("r", [0.2, 0.5, 0.9])
def test_plain_dielectric_is_lobes_1_2_4_by_hand(r):
    """every optional weight 0, metallic 0: DisneyDiffuse + DisneyRetro + the reflection lobe, written out here from the
    formulas without the model's functions (Trowbridge-Reitz's D in pbrt's tan^2 form, Lambda from microfacet_model)"""
    col, eta = np.array([0.7, 0.4, 0.2]), 1.5
    m = dm.Disney(scenes.disney(col, roughness=r, specular_tint=0.0))
    assert m.lobes == ["diffuse", "retro", "micro"]
    wo, wi = np.abs(_pairs(3000, 5))  # above the surface: below it the Fresnel term is the inside's (cos on the flipped wh < 0)
    col = np.asarray(col, np.float32).astype(np.float64)
    r = float(np.float32(r))
    co, ci = np.abs(wo[:, 2]), np.abs(wi[:, 2])
    fo, fi = (1 - co) ** 5, (1 - ci) ** 5
    wh = _unit(wo + wi)
    cd = np.sum(wi * wh, 1)
    diffuse = col / np.pi * ((1 - fo / 2) * (1 - fi / 2))[:, None]
    rr = 2 * r * cd * cd
    retro = col / np.pi * (rr * (fo + fi + fo * fi * (rr - 1)))[:, None]
    a = max(1e-3, r * r)
    g = 1 / ((1 + mm.tr_lambda(wo, a, a)) * (1 + mm.tr_lambda(wi, a, a)))
    # metallic 0: F = FrDielectric(cd, 1, eta), the same for every channel (specular_tint 0 or not: Cspec0 is not read)
    st = np.sqrt(np.maximum(0, 1 - cd * cd)) / eta
    ct = np.sqrt(1 - st * st)
    F = (((eta * cd - ct) / (eta * cd + ct)) ** 2 + ((cd - eta * ct) / (cd + eta * ct)) ** 2) / 2
    micro = (mm.tr_d(wh, a, a) * g * F / (4 * co * ci))[:, None]
    np.testing.assert_allclose(dm.bsdf_f(m, wo, wi), diffuse + retro + micro, rtol=1e-9)
    for lobe, want in (("diffuse", diffuse), ("retro", retro), ("micro", np.repeat(micro, 3, 1))):
        np.testing.assert_allclose(dm.lobe_f(m, lobe, wo, wi), want, rtol=1e-9, atol=1e-300)
    # and nothing crosses the surface
    wo, wi = _pairs(500, 6, across=True)
    assert np.all(dm.bsdf_f(m, wo, wi) == 0) and np.all(dm.bsdf_pdf(m, wo, wi) == 0)


def test_lobe_sets_and_constants():
    """which lobes a descriptor turns on, in which order, and the host-side constants of DESIGN.md"""
    lobes = {c[0]: c[2].lobes for c in CASES}
    assert lobes["defaults"] == ["diffuse", "retro", "micro"]
    assert lobes["metallic1"] == ["micro"]
    assert lobes["sheen_tint0"] == ["diffuse", "retro", "sheen", "micro"]
    assert lobes["metal_clearcoat"] == ["micro", "clearcoat"]
    assert lobes["spec_trans1"] == ["micro", "trans"]
    assert lobes["thin_metal"] == ["micro", "lambert_t"]
    assert lobes["thin_dt0"] == ["diffuse", "fakess", "retro", "micro", "trans", "lambert_t"]
    assert lobes["black"] == ["diffuse", "retro", "sheen", "micro", "trans"]  # added even when black
    assert lobes["everything"] == list(dm.LOBES)
    assert set(sum(lobes.values(), [])) == set(dm.LOBES)
    m = dm.Disney(scenes.disney((0.8, 0.5, 0.3), roughness=0.4, anisotropic=0.8))
    aspect = np.sqrt(1 - 0.9 * np.float32(0.8))
    assert m.ax == pytest.approx(np.float32(0.4) ** 2 / aspect) and m.ay == pytest.approx(np.float32(0.4) ** 2 * aspect)
    m = dm.Disney(scenes.disney((0.8, 0.5, 0.3), roughness=0.0))
    assert (m.ax, m.ay) == (1e-3, 1e-3)
    assert dm.Disney(scenes.disney((0.8, 0.5, 0.3), clearcoat=1.0, clearcoat_gloss=1.0)).a2 == pytest.approx(1e-6)
    assert dm.Disney(scenes.disney((0.8, 0.5, 0.3), clearcoat=1.0, clearcoat_gloss=0.0)).a2 == pytest.approx(1e-2)
    m = dm.Disney(scenes.disney((0.8, 0.5, 0.3), thin=True, spec_trans=0.5, roughness=0.5, eta=1.5))
    assert m.tax == pytest.approx(((0.65 * 1.5 - 0.35) * 0.5) ** 2) and not m.sep_trans
    m = dm.Disney(scenes.disney((0, 0, 0), sheen=1.0, sheen_tint=1.0))
    assert np.all(m.c_sheen == 1.0)  # a black colour has no tint: Ctint = 1
    m = dm.Disney(scenes.disney((0.8, 0.5, 0.3), metallic=1.0))
    np.testing.assert_allclose(m.cspec0, np.float32([0.8, 0.5, 0.3]))


def test_clearcoat_is_normalised_and_its_sampler_follows_it():
    """GTR1 integrates to 1 against cos theta_h, and the sampler's cos theta_h is its inverse CDF, at gloss 0, 0.5 and 1"""
    for gloss in (0.0, 0.5, 1.0):
        m = dm.Disney(scenes.disney((0.8, 0.5, 0.3), clearcoat=1.0, clearcoat_gloss=gloss))
        # CDF of cos theta_h: int_c^1 2 pi GTR1(x) x dx = ln(1 + (a2 - 1) c^2) / ln(a2) -> 1 at c = 0
        u = np.linspace(0.0, 0.999, 50)
        wo = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (50, 3))
        c = dm.clearcoat_sample_wh(m, wo, u, np.zeros(50))[:, 2]
        np.testing.assert_allclose(1 - np.log(1 + (m.a2 - 1) * c * c) / np.log(m.a2), u, atol=1e-9)
        x, w = np.polynomial.legendre.leggauss(400)
        t = np.exp(0.5 * (x + 1) * np.log(2.0))  - 1  # nodes crowded towards theta = 0: t in [0, 1]
        th = t * np.pi / 2
        wh = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], 1)
        jac = 0.5 * np.log(2.0) * (t + 1) * np.pi / 2
        total = np.sum(2 * np.pi * dm.gtr1(m, wh) * np.cos(th) * np.sin(th) * jac * w)
        assert total == pytest.approx(1.0, abs=2e-3 if gloss == 1.0 else 1e-6), (gloss, total)


@pytest.mark.parametrize("k", range(len(FURNACE)), ids=[c[0] for c in FURNACE])
def test_furnace_reference_is_converged(k):
    """a doubled quadrature grid changes the furnace reference by less than 1e-4 of it: test_gpu_disney.py asserts that this
    error is below a quarter of its render's standard error"""
    _, _, m, below = FURNACE[k]
    ref, err = furnace_reference(m, furnace_wo(below))
    print(f"{FURNACE[k][0]}: albedo {ref}, quadrature error {err}")
    assert np.all(ref > 0.05) and np.all(err < 1e-4 * ref), (ref, err)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_direction_table(i):
    """what test_gpu_disney.py assumes of its table: a small grazing band, finite values, every lobe exercised"""
    m = CASES[i][2]
    wo, wi, u = directions(m, 3000, 300 + i)
    wo, wi = wo.astype(np.float64), wi.astype(np.float64)
    band = in_band(m, wo, wi)
    assert band.mean() <= BAND_MAX_SHARE, band.mean()
    ok = (np.abs(wo[:, 2]) >= 1e-3) & (np.abs(wi[:, 2]) >= 1e-3) & (np.linalg.norm(wo + wi, axis=1) > 1e-2)
    assert np.isfinite(dm.bsdf_f(m, wo, wi)[ok]).all() and np.isfinite(dm.bsdf_pdf(m, wo, wi)[ok]).all()
    for lobe in m.lobes:
        black = lobe not in ("micro", "clearcoat") and not np.any(getattr(m, "c_" + lobe))
        if not black and not (lobe == "retro" and m.roughness == 0):  # (DisneyRetro is 0 at roughness 0)
            assert np.count_nonzero(dm.lobe_f(m, lobe, wo, wi)[ok & ~band, 1]) > 300, lobe
    comp = dm.bsdf_sample_f(m, wo, u)[5]
    assert set(np.unique(comp)) == set(range(m.n))


def test_sample_f_flags_and_consistency():
    for _, _, m in CASES:
        rng = np.random.default_rng(5)
        wo = _unit(rng.normal(size=(4000, 3)))
        wi, f, pdf, ok, flags, comp = dm.bsdf_sample_f(m, wo, rng.random((4000, 2)))
        assert ok.mean() > 0.3
        np.testing.assert_allclose(pdf[ok], dm.bsdf_pdf(m, wo[ok], wi[ok]), rtol=1e-12)
        across = wo[ok, 2] * wi[ok, 2] < 0
        assert np.all((flags[ok] & dm.TRANSMISSION != 0) == across)
        assert np.all(flags[~ok] == 0)
        assert np.array_equal(flags[ok], np.array([dm.FLAGS[m.lobes[k]] for k in comp[ok]]))


# ---- the host side of the entry point ----
def test_descriptor_validation():
    """scenes.disney_invalid states the rules of pbrt_hip_scene_set_disney_material (test_gpu_disney.py holds the library to
    the same list)"""
    d = scenes.disney((0.8, 0.5, 0.3))
    assert d == dict(color=(0.8, 0.5, 0.3), metallic=0.0, eta=1.5, roughness=0.5, specular_tint=0.0, anisotropic=0.0, sheen=0.0, sheen_tint=0.5,
                     clearcoat=0.0, clearcoat_gloss=1.0, spec_trans=0.0, flatness=0.0, diff_trans=1.0, thin=0)  # pbrt-v3's defaults
    assert scenes.disney_invalid(d) is None
    for row, desc, why in REFUSED:
        if 0 <= row < 2:
            assert re.search(why, scenes.disney_invalid(desc) or ""), (desc, why)
    for desc in ACCEPTED + [c[1] for c in CASES]:
        assert scenes.disney_invalid(desc) is None, desc


def test_disney_desc_layout(tmp_path):
    src = tmp_path / "d.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrt_hip.h"\nint main(void) { printf("%d %d %d %d %d %d", '
                   '(int)sizeof(PbrtDisneyDesc), (int)offsetof(PbrtDisneyDesc, metallic), (int)offsetof(PbrtDisneyDesc, sheen_tint), '
                   '(int)offsetof(PbrtDisneyDesc, diff_trans), (int)offsetof(PbrtDisneyDesc, thin), (int)sizeof(PbrtMaterialDesc)); return 0; }\n')
    exe = tmp_path / "d"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    D = pbrt_hip.DisneyDesc
    assert got == [ctypes.sizeof(D), D.metallic.offset, D.sheen_tint.offset, D.diff_trans.offset, D.thin.offset, ctypes.sizeof(pbrt_hip.MaterialDesc)]
    assert got[0] == 64 and got[5] == 72  # PbrtMaterialDesc keeps its size
    assert [f[0] for f in D._fields_] == ["color"] + list(scenes.DISNEY_SCALARS) + ["thin"]


def test_header_and_library_export_the_entry_point():
    h = open(HEADER).read()
    assert re.search(r"int pbrt_hip_scene_set_disney_material\(PbrtHipScene\* scene, int32_t material, const PbrtDisneyDesc\* desc\);", h)
    L = ctypes.CDLL(pbrt_hip.LIB_PATH)
    assert hasattr(L, "pbrt_hip_scene_set_disney_material")
    assert "pbrt_hip_scene_set_disney_material" in pbrt_hip.EXPORTS
