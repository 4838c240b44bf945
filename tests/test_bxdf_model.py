"""The float64 model of Oren-Nayar, rough glass and substrate (bxdf_model.py) held to what a BSDF has to satisfy, before any
device is compared with it: its sampler against its pdf (chi^2; the reference's reflection.rs:1185 form of the transmission pdf
fails the same test), pdf normalisation, reciprocity, energy, limits, and that the furnace references and the
direction tables of test_gpu_bxdfs.py are what that test assumes."""
import numpy as np
import pytest

import bxdf_model as bm
import microfacet_model as mm
from bxdf_cases import (BAND_MAX_SHARE, CASES, CHI2, CHI2_FIT, CHI2_FIT_LEFT_OUT, CHI2_MODEL, FURNACE, KR, KT, N_FIT, W, Z, chi2_wo, directions, furnace_wo,
                        in_band)
from glossy_cases import _unit

N_CHI2 = 1_000_000
N_WRONG = 100_000  # a wrong pdf fails by orders of magnitude at a tenth of the samples


def _chi2(m, theta_o, seed, n=N_CHI2, exact_slope=True):
    wo = chi2_wo(theta_o)
    u = np.random.default_rng(seed).random((n, 2))
    wi, _, _, ok, _ = bm.bsdf_sample_f(m, np.broadcast_to(wo, (n, 3)), u, exact_slope=exact_slope)
    return bm.chi2_p(m, wo, wi, ok, n)


@pytest.mark.parametrize("name,theta_o", CHI2, ids=[f"{c[0]}-{c[1]:g}" for c in CHI2])
def test_sampler_chi2(name, theta_o):
    """sample_f against the integrated pdf, 10^6 samples: every lobe set at two wo, one below the surface for glass. The
    visible-normal sampler draws slope_y from the exact inverse here: what is tested are the lobes' pdfs, Jacobians and the
    lobe choice, not the rational fit (test_sampler_chi2_with_the_fit holds the sampler as it is, bxdf_cases.CHI2_FIT)."""
    p, chi2, bins, stray = _chi2(CHI2_MODEL[name], theta_o, 70 + CHI2.index((name, theta_o)))
    assert stray == 0, "samples where the pdf has no mass"
    assert p > 1e-3, (chi2, bins, p)


@pytest.mark.parametrize("name,theta_o", CHI2_FIT, ids=[f"{c[0]}-{c[1]:g}" for c in CHI2_FIT])
def test_sampler_chi2_with_the_fit(name, theta_o):
    """the cases and sample count of test_gpu_bxdfs.py::test_sampler_chi2, with pbrt-v3's sampler in float64"""
    p, chi2, bins, stray = _chi2(CHI2_MODEL[name], theta_o, 7, n=N_FIT, exact_slope=False)
    assert stray == 0 and p > 1e-3, (chi2, bins, p)


def test_fit_breaks_transmission_alone_from_above():
    """the case bxdf_cases.CHI2_FIT leaves out: the fit's missing slope tail is resolved, the exact inverse passes (test_sampler_chi2)"""
    name, theta_o = CHI2_FIT_LEFT_OUT
    p, chi2, bins, _ = _chi2(CHI2_MODEL[name], theta_o, 7, n=N_FIT, exact_slope=False)
    print(f"{name} {theta_o} with the fit: chi2 {chi2:.4g} over {bins} bins, p {p:.3g}")
    assert p < 1e-3


def test_fit_truncates_the_slope_tail():
    assert bm.FIT_MAX_SLOPE == pytest.approx(7.256, abs=1e-3)
    assert bm.slope_tail_mass(bm.FIT_MAX_SLOPE) == pytest.approx(1.086e-3, rel=1e-3)
    u2 = np.linspace(0.5, 1, 1001)[:-1]
    _, sy = mm._sample11(np.full(1000, 0.5), np.full(1000, 0.5), u2)
    sx, _ = mm._sample11(np.full(1000, 0.5), np.full(1000, 0.5), u2)
    assert np.max(np.abs(sy) / np.sqrt(1 + sx * sx)) < bm.FIT_MAX_SLOPE


@pytest.mark.parametrize("theta_o", [35.0, 140.0])
def test_reference_transmission_pdf_fails_chi2(theta_o):
    """reflection.rs:1185 multiplies by the denominator where pbrt-v3 divides by its square: the same sampler is not
    distributed by that pdf (D70)"""
    m = bm.rough_glass(Z, KT, 1.5, 0.3, remap=False, pdf_form="reference")
    p, chi2, bins, _ = _chi2(m, theta_o, 5, n=N_WRONG)
    print(f"reference form, theta_o {theta_o}: chi2 {chi2:.4g} over {bins} bins at {N_WRONG} samples, p {p:.3g}")
    assert p < 1e-3


def test_v3_transmission_pdf_counts_back_faces():
    """pbrt-v3's MicrofacetTransmission::Pdf as it stands gives mass to half vectors wo sees from behind, which its sampler
    never returns (wo.wh < 0 is rejected): seen from above at 60 degrees it integrates to more than 1 and fails the chi^2 test;
    with those microfacets at 0 (D72) both hold (test_sampler_chi2, test_pdf_integrates_to_at_most_one)"""
    m = bm.rough_glass(Z, KT, 1.33, 0.25, remap=False, pdf_form="v3")
    total = bm.pdf_integral(m, chi2_wo(60.0))
    p, chi2, bins, _ = _chi2(m, 60.0, 5, n=N_WRONG)
    print(f"pbrt-v3 form, theta_o 60: integral {total:.5f}, chi2 {chi2:.4g} over {bins} bins at {N_WRONG} samples, p {p:.3g}")
    assert total > 1.02 and p < 1e-3


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_pdf_integrates_to_at_most_one(i):
    m = CASES[i][2]
    for wo in (_unit(np.array([0.3, -0.4, 0.7])), _unit(np.array([0.5, 0.2, -0.4]))):
        total = bm.pdf_integral(m, wo)
        assert 0 < total <= 1 + 1e-4, (wo, total)  # (less than 1: reflected samples under the horizon, total internal reflection)


def _pairs(n, seed, across):
    rng = np.random.default_rng(seed)
    wo = _unit(rng.normal(size=(n, 3)))
    wi = _unit(rng.normal(size=(n, 3)))
    wi[:, 2] = np.abs(wi[:, 2]) * np.sign(wo[:, 2]) * (-1 if across else 1)
    return wo, wi


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_reciprocity(i):
    """f(wo, wi) = f(wi, wo) for the reflection lobes; for transmission in radiance mode f(wo, wi) eta(wi)^2 = f(wi, wo) eta(wo)^2,
    eta(w) the index on w's side (1 above, eta below). From the formula: with wo above, f(wo, wi) carries eta^2 / eta^2 over
    (wo.wh + eta wi.wh)^2; the swapped pair has relative index 1 / eta and the same half vector, so its denominator is
    (wi.wh + wo.wh / eta)^2 = (wo.wh + eta wi.wh)^2 / eta^2 with everything else equal (1 - F is symmetric by Snell's law):
    f(wi, wo) = eta^2 f(wo, wi)."""
    m = CASES[i][2]
    wo, wi = _pairs(4000, 11 + i, across=False)
    a, b = bm.bsdf_f(m, wo, wi), bm.bsdf_f(m, wi, wo)
    scale = np.maximum(np.abs(a), np.abs(b)).max() + 1e-300
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * scale)
    if m.kind == bm.GLASS:
        wo, wi = _pairs(4000, 31 + i, across=True)
        eta_of = lambda w: np.where(w[:, 2] > 0, 1.0, m.eta)[:, None]
        a, b = bm.bsdf_f(m, wo, wi) * eta_of(wi) ** 2, bm.bsdf_f(m, wi, wo) * eta_of(wo) ** 2
        if "trans" in m.lobes:
            assert np.count_nonzero(a) > 1000
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * (np.abs(a).max() + 1e-300))


ENERGY = [bm.rough_glass(W, W, 1.5, 0.2, remap=False), bm.rough_glass(W, W, 1.33, 0.5, remap=False), bm.rough_glass(W, W, 1.5, 0.15, 0.6, remap=False),
          bm.substrate((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.2, remap=False), bm.substrate((1, 1, 1), (0, 0, 0), 0.3, remap=False),
          bm.substrate((0, 0, 0), (1, 1, 1), 0.15, 0.6, remap=False), bm.matte_sigma(W, 20.0), bm.matte_sigma(W, 90.0)]


@pytest.mark.parametrize("k", range(len(ENERGY)))
def test_albedo_at_most_one(k):
    """albedo <= 1 seen from above. In radiance mode f carries 1 / eta^2 towards the denser side and eta^2 back (radiance is
    compressed into the denser medium), so from inside the glass a furnace looks brighter than 1, as it does through
    specular glass; what is conserved is the reflected part plus the transmitted part times eta(wi)^2 / eta(wo)^2 (the
    reciprocity relation carries the integral over wi to the one over outgoing directions), and that is <= 1 on both sides."""
    m = ENERGY[k]
    for theta in (10.0, 50.0, 80.0, 130.0, 170.0):
        t = np.radians(theta)
        wo = np.array([np.sin(t), 0.0, np.cos(t)])
        same, across = bm.albedo_parts(m, wo)
        rho = same + across
        assert np.all(rho > 0.02), (theta, rho)
        if wo[2] > 0:
            assert np.all(rho <= 1 + 1e-4), (theta, rho)
        ratio = (m.eta if wo[2] > 0 else 1 / m.eta) ** 2
        assert np.all(same + across * ratio <= 1 + 1e-4), (theta, same, across)


def test_oren_nayar_limits():
    """sigma -> 0 is Lambert; sin theta <= 1e-4 takes the branch without the azimuth term"""
    kd = np.array([0.6, 0.5, 0.4])
    wo, wi = _pairs(1000, 3, across=False)
    m0 = bm.matte_sigma(kd, 0.0)
    assert (m0.A, m0.B) == (1.0, 0.0)
    np.testing.assert_allclose(bm.bsdf_f(m0, wo, wi), np.broadcast_to(kd / np.pi, (1000, 3)), rtol=1e-15)
    np.testing.assert_allclose(bm.bsdf_f(bm.matte_sigma(kd, 1e-6), wo, wi), np.broadcast_to(kd / np.pi, (1000, 3)), rtol=1e-9)
    m = bm.matte_sigma(kd, 40.0)
    s = np.radians(40.0) ** 2
    assert m.A == pytest.approx(1 - s / (2 * (s + 0.33))) and m.B == pytest.approx(0.45 * s / (s + 0.09))
    # wo within 1e-4 of the normal: max_cos = 0, f = Kd / pi * A whatever wi is ...
    near = _unit(np.array([5e-5, 0.0, 1.0]))
    f = bm.bsdf_f(m, np.broadcast_to(near, (1000, 3)), np.abs(wi))
    np.testing.assert_allclose(f, np.broadcast_to(kd / np.pi * m.A, (1000, 3)), rtol=1e-15)
    # ... and just outside the branch the azimuth term is there
    out = _unit(np.array([0.3, 0.0, 1.0]))
    wi1 = _unit(np.array([0.5, 0.0, 0.6]))[None]
    assert bm.bsdf_f(m, out[None], wi1)[0, 0] > kd[0] / np.pi * m.A * 1.01
    # sigma is clamped to [0, 90] degrees
    assert bm.matte_sigma(kd, 200.0).A == bm.matte_sigma(kd, 90.0).A


@pytest.mark.parametrize("k", range(len(FURNACE)), ids=[c[0] for c in FURNACE])
def test_furnace_reference_is_converged(k):
    """alpha >= 0.2: a doubled quadrature grid changes the furnace reference by < 1e-4"""
    _, _, m, below = FURNACE[k]
    assert m.kind == bm.OREN or min(m.ax, m.ay) >= 0.2
    wo = furnace_wo(below)
    a, b = bm.albedo(m, wo), bm.albedo(m, wo, 256, 1024)
    assert np.all(np.abs(a - b) < 1e-4 * b), (a, b)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_direction_table_keeps_the_grazing_band_small(i):
    """the band where float32 loses 1 - F and cos theta_t holds at most 15 % of a case's pairs, on the model alone"""
    m = CASES[i][2]
    wo, wi, _ = directions(m, 3000, 200 + i)
    wo, wi = wo.astype(np.float64), wi.astype(np.float64)
    band = in_band(m, wo, wi)
    assert band.mean() <= BAND_MAX_SHARE, band.mean()
    f = bm.bsdf_f(m, wo, wi)
    assert np.isfinite(f[np.abs(wo[:, 2]) > 0]).all()
    if "trans" in m.lobes:
        across = (wo[:, 2] * wi[:, 2] < 0) & ~band
        assert np.count_nonzero(f[across, 1]) > 300  # the transmission lobe is exercised outside the band


def test_sample_f_flags_and_consistency():
    """sample_f's f and pdf are f and pdf at the sampled direction, the flags name the sampled lobe"""
    for _, _, m in CASES:
        rng = np.random.default_rng(5)
        wo = _unit(rng.normal(size=(4000, 3)))
        wi, f, pdf, ok, flags = bm.bsdf_sample_f(m, wo, rng.random((4000, 2)))
        assert ok.mean() > 0.3
        np.testing.assert_allclose(pdf[ok], bm.bsdf_pdf(m, wo[ok], wi[ok]), rtol=1e-12)
        np.testing.assert_allclose(f[ok], bm.bsdf_f(m, wo[ok], wi[ok]), rtol=1e-12)
        across = wo[ok, 2] * wi[ok, 2] < 0
        assert np.all((flags[ok] & bm.TRANSMISSION != 0) == across)
        assert np.all(flags[~ok] == 0)
        want = {bm.OREN: {bm.REFLECTION | bm.DIFFUSE}, bm.SUBSTRATE: {bm.REFLECTION | bm.GLOSSY},
                bm.GLASS: {bm.FLAGS[l] for l in m.lobes}}[m.kind]
        assert set(np.unique(flags[ok])) == want
