"""The hair model (hair_model.py) against what defines it, not against itself: the normalisations of Ap, Mp and Np, the white furnace
per h, the sampler against the pdf, the three absorption parametrisations; and the host against the model: pbrt_hip.hair_tables bit
for bit, the refusals hair_of_desc can see without a scene, the layouts of the new structs."""
import ctypes
import math

import numpy as np
import pytest

import hair_model as hm
import pbrt_hip
from hair_cases import CASES, DESCS, LEFT_OUT_MAX_SHARE, MODELS, left_out, points
from pbrt_hip import scenes


def test_ap_sums_to_one_without_absorption():
    rng = np.random.default_rng(3)
    n = 1000
    h = rng.uniform(-1, 1, n)
    sin_o = rng.uniform(-1, 1, n)
    cos_o = np.sqrt(1 - sin_o * sin_o)
    phi = rng.uniform(0, 2 * np.pi, n)
    wo = np.stack([sin_o, cos_o * np.cos(phi), cos_o * np.sin(phi)], axis=1)
    for eta in (1.55, 1.2):
        g = hm._geometry(hm.HairModel(eta=eta), h, wo)
        total = g.ap[0] + g.ap[1] + g.ap[2] + g.ap[3]
        assert np.abs(total - 1).max() <= 1e-12
    # h = +-1: F == 1, the residual's 0 / 0 is 0 (D111)
    g = hm._geometry(hm.HairModel(), np.array([-1.0, 1.0]), wo[:2])
    assert np.all(g.ap[0] == 1) and all(np.all(a == 0) for a in g.ap[1:])


def _simpson(f, a, b, n):
    x = np.linspace(a, b, n + 1)
    y = f(x)
    return (b - a) / (3 * n) * (y[0] + y[-1] + 4 * y[1:-1:2].sum() + 2 * y[2:-1:2].sum())


@pytest.mark.parametrize("v", [0.0065, 0.05, 0.1, 0.5, 4.0])
@pytest.mark.parametrize("theta_o", [0.0, 0.6, -1.3])
def test_mp_is_normalised(v, theta_o):
    """int Mp cos(theta_i) d theta_i = 1 for the exact Bessel function. The bound is the quadrature's own error (Simpson, the step
    halved) plus what the model's closed forms are off by over the arguments x = cos(theta_i) cos(theta_o) / v this integral
    reaches, measured against scipy's I0: I0's series cut after twenty terms (x <= 12: 1e-10), log I0's asymptotic series cut
    after 225 / (3072 x^3) (x > 12: 5e-6), 0.6931 for ln 2 (4.72e-5), and 2 sinh(1 / v) taken as exp(1 / v) (exp(-2 / v)).
    Measured: 0.99995 at v <= 0.1, 1.00000 above."""
    from scipy import special
    so, co = math.sin(theta_o), math.cos(theta_o)
    x = np.linspace(1e-9, co / v, 20001)
    exact_log = np.log(special.ive(0, x)) + x
    ours_log = hm.log_i0(x) if v <= 0.1 else np.log(hm.i0(x))
    closed_form = float(np.max(np.abs(np.expm1(ours_log - exact_log)))) + (-math.expm1(0.6931 - math.log(2.0)) + 2 * math.exp(-2 / v) if v <= 0.1 else 0.0)
    f = lambda t: hm.mp(np.cos(t), co, np.sin(t), so, np.float64(v)) * np.cos(t)
    fine, coarse = _simpson(f, -np.pi / 2, np.pi / 2, 1 << 15), _simpson(f, -np.pi / 2, np.pi / 2, 1 << 14)
    err = abs(fine - coarse)
    print(f"v {v} theta_o {theta_o}: {fine:.8f}, quadrature error {err:.2g}, closed forms off by at most {closed_form:.2g}")
    assert err < 1e-4  # (the integrand steps where log I0 changes branch at x = 12)
    assert abs(fine - 1) <= err + closed_form + 1e-9


@pytest.mark.parametrize("s", [hm.HairModel(beta_n=b).s for b in (0.1, 0.3, 0.9)])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_np_is_normalised(s, p):
    """int Np d phi = 1 over a full turn, by Simpson on either side of the logistic's kink; the bound is the quadrature's error"""
    go, gt = 0.4, 0.25
    centre = hm.phi_p(p, go, gt)
    f = lambda x: hm.np_(x, p, s, go, gt)
    val = [sum(_simpson(f, a, b, n) for a, b in ((centre - np.pi, centre), (centre, centre + np.pi))) for n in (1 << 14, 1 << 13)]
    err = abs(val[0] - val[1])
    print(f"s {s:.4f} p {p}: {val[0]:.10f}, quadrature error {err:.2g}")
    assert abs(val[0] - 1) <= err + 1e-9


def _furnace(m, h, n_theta, n_phi, theta_o=0.3):
    """int f |cos| d omega_i by the midpoint rule on a (theta_i, phi_i) product grid, for wo at theta_o, phi_o = 0.7: the channel
    that is farthest from 1 (at sigma_a = 0 the three are one number)"""
    th = (np.arange(n_theta) + 0.5) / n_theta * np.pi - np.pi / 2
    ph = (np.arange(n_phi) + 0.5) / n_phi * 2 * np.pi - np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    T, P = T.ravel(), P.ravel()
    wi = np.stack([np.sin(T), np.cos(T) * np.cos(P), np.cos(T) * np.sin(P)], axis=1)
    wo = np.tile(np.array([[math.sin(theta_o), math.cos(theta_o) * math.cos(0.7), math.cos(theta_o) * math.sin(0.7)]]), (len(T), 1))
    f = hm.hair_f(m, np.full(len(T), h), wo, wi) * np.abs(wi[:, 2:3])
    rgb = (f * np.cos(T)[:, None]).sum(0) * (np.pi / n_theta) * (2 * np.pi / n_phi)
    return float(rgb[np.argmax(np.abs(rgb - 1))])


# alpha = 2: pbrt-v3 is itself only approximately conserving. RECORDED from this model, not derived: over the cases below the
# integral at alpha = 2 and the one at alpha = 0 agree in all six digits printed (0.999953 .. 1.000006 at either).
FURNACE_ALPHA2_RECORDED = 2e-6


@pytest.mark.parametrize("alpha", [0.0, 2.0])
@pytest.mark.parametrize("beta_n", [0.1, 0.3, 0.9])
@pytest.mark.parametrize("beta_m", [0.1, 0.3, 0.9])
def test_white_furnace_per_h(beta_m, beta_n, alpha):
    """int f |cos| d omega_i = 1 at sigma_a = 0 for h in {-0.95, 0, 0.3, 0.999}: the midpoint rule on a product grid with 24 points
    per standard deviation of the narrowest Mp (v[1], 0.0016 at beta_m = 0.1) and 16 per logistic scale. The bound is the
    quadrature's error estimate (the step halved in both directions) plus 1e-3 (alpha = 2: plus the recorded value above).

    Measured: 0.999953 .. 0.999961 at beta_m = 0.1 and 0.3 (what is missing is 0.6931 for ln 2, 4.7e-5) and 1.000005 .. 1.000006
    at beta_m = 0.9, with a quadrature error below 2e-5. With pbrt-v3's own I0 (ten terms) and log I0 (1 / (16 x) for the
    series' tail) the same integral is 0.9930 .. 0.9983 at beta_m = 0.3: the model and the device use the longer forms
    (DESIGN.md D112)."""
    m = hm.HairModel(beta_m=beta_m, beta_n=beta_n, alpha=alpha)
    n_theta = int(min(2048, max(256, 2 * math.ceil(12 * np.pi / math.sqrt(m.v[1])))))
    n_phi = int(min(4096, max(1024, 2 * math.ceil(16 * np.pi / m.s))))
    for h in (-0.95, 0.0, 0.3, 0.999):
        fine, coarse = _furnace(m, h, n_theta, n_phi), _furnace(m, h, n_theta // 2, n_phi // 2)
        err = abs(fine - coarse)
        print(f"beta_m {beta_m} beta_n {beta_n} alpha {alpha} h {h}: {fine:.6f} on {n_theta} x {n_phi}, quadrature error {err:.2g}")
        assert abs(fine - 1) <= err + 1e-3 + (FURNACE_ALPHA2_RECORDED if alpha else 0.0)


@pytest.mark.parametrize("alpha", [0.0, 2.0])
@pytest.mark.parametrize("beta_m", [0.3, 0.9])
def test_white_furnace_at_a_grazing_theta_o(beta_m, alpha):
    """the same integral with wo 74 degrees off the fibre's normal plane (theta_o = 1.3), where the tilted cos(theta_o') is small and
    eta' large: beta_n = 0.3, h in {-0.95, 0.3}, 1024 x 1024 against 512 x 512. The same bound. Measured: 0.999965 .. 1.000000."""
    m = hm.HairModel(beta_m=beta_m, beta_n=0.3, alpha=alpha)
    for h in (-0.95, 0.3):
        fine, coarse = _furnace(m, h, 1024, 1024, 1.3), _furnace(m, h, 512, 512, 1.3)
        err = abs(fine - coarse)
        print(f"theta_o 1.3 beta_m {beta_m} alpha {alpha} h {h}: {fine:.6f}, quadrature error {err:.2g}")
        assert abs(fine - 1) <= err + 1e-3 + (FURNACE_ALPHA2_RECORDED if alpha else 0.0)


@pytest.mark.parametrize("i", [0, 5, 10, 11], ids=[CASES[i][0] for i in (0, 5, 10, 11)])
def test_sample_weights_are_one_without_absorption(i):
    """pbrt-v3's own test: at sigma_a = 0 every sample has f |wi.z| / pdf in [1 - 1e-3, 1 + 1e-3]"""
    m = MODELS[i]
    assert np.all(m.sigma_a == 0)
    h, wo, wi, u = (a.astype(np.float64) for a in points(40 + i))
    wis, f, pdf, ok, p = hm.bsdf_sample_f(m, h, wo, u)
    sel = ok & ~left_out(wo, wis) & (np.abs(h) < 1)
    w = f[sel] * np.abs(wis[sel, 2:3]) / pdf[sel, None]
    print(f"{CASES[i][0]}: weights {w.min():.6f} .. {w.max():.6f} over {sel.sum()} samples, p counts {np.bincount(p[sel], minlength=4)}")
    assert sel.sum() > 0.9 * len(h) and w.min() >= 1 - 1e-3 and w.max() <= 1 + 1e-3
    np.testing.assert_allclose(hm.hair_pdf(m, h[sel], wo[sel], wis[sel]), pdf[sel], rtol=1e-9)


def test_sampler_chi2_with_absorption():
    """10^6 samples over a 16 x 32 (theta, phi) grid against the pdf integrated per cell (8 x 8 midpoints), Pearson chi^2, bins
    expecting fewer than 5 pooled; p > 1e-3, the significance of test_disney_model.py::test_sampler_chi2"""
    from scipy import stats
    m = MODELS[4]  # the defaults: eumelanin 1.3
    assert np.all(m.sigma_a > 0)
    n, nt, npi, sub = 1_000_000, 16, 32, 8
    rng = np.random.default_rng(11)
    wo1 = np.array([math.sin(-0.4), math.cos(-0.4) * math.cos(1.1), math.cos(-0.4) * math.sin(1.1)])
    h0 = 0.35
    wis, _, pdf, ok, _ = hm.bsdf_sample_f(m, np.full(n, h0), np.tile(wo1, (n, 1)), rng.random((n, 2)))
    assert ok.all()
    theta, phi = np.arcsin(np.clip(wis[:, 0], -1, 1)), np.arctan2(wis[:, 2], wis[:, 1])
    it = np.clip(((theta + np.pi / 2) / np.pi * nt).astype(int), 0, nt - 1)
    ip = np.clip(((phi + np.pi) / (2 * np.pi) * npi).astype(int), 0, npi - 1)
    counts = np.bincount(it * npi + ip, minlength=nt * npi).astype(np.float64)
    th = (np.arange(nt * sub) + 0.5) / (nt * sub) * np.pi - np.pi / 2
    ph = (np.arange(npi * sub) + 0.5) / (npi * sub) * 2 * np.pi - np.pi
    T, P = (a.ravel() for a in np.meshgrid(th, ph, indexing="ij"))
    wi = np.stack([np.sin(T), np.cos(T) * np.cos(P), np.cos(T) * np.sin(P)], axis=1)
    dens = hm.hair_pdf(m, np.full(len(T), h0), np.tile(wo1, (len(T), 1)), wi) * np.cos(T)
    cell = dens.reshape(nt, sub, npi, sub).sum(axis=(1, 3)) * (np.pi / (nt * sub)) * (2 * np.pi / (npi * sub))
    print(f"pdf integrates to {cell.sum():.6f}")
    assert abs(cell.sum() - 1) < 2e-3
    expected = cell.ravel() / cell.sum() * n
    order = np.argsort(expected)
    e, c = expected[order], counts[order]
    k = int(np.searchsorted(np.cumsum(e), 5.0)) + 1  # the smallest bins pooled into one that expects at least 5
    e, c = np.append(e[k:], e[:k].sum()), np.append(c[k:], c[:k].sum())
    chi2 = float(((c - e) ** 2 / e).sum())
    p = float(stats.chi2.sf(chi2, len(e) - 1))
    print(f"chi2 {chi2:.5g} over {len(e)} bins, p {p:.3g}")
    assert p > 1e-3


def test_absorption_parametrisations():
    bn = 0.3
    d = 5.969 - 0.215 * bn + 2.532 * bn ** 2 - 10.73 * bn ** 3 + 5.574 * bn ** 4 + 0.245 * bn ** 5
    np.testing.assert_allclose(hm.sigma_a_from_color((0.8, 0.5, 0.2), bn), [(math.log(c) / d) ** 2 for c in (0.8, 0.5, 0.2)], rtol=1e-15)
    assert np.all(hm.sigma_a_from_color((1.0, 1.0, 1.0), bn) == 0)
    np.testing.assert_allclose(hm.sigma_a_from_melanin(1.3, 0.2), [1.3 * 0.419 + 0.2 * 0.187, 1.3 * 0.697 + 0.2 * 0.4, 1.3 * 1.37 + 0.2 * 1.05],
                               rtol=1e-15)
    # scenes.hair: pbrt-v3's precedence and default
    assert scenes.hair()["absorption"] == scenes.HAIR_MELANIN and scenes.hair()["eumelanin"] == 1.3
    assert scenes.hair(sigma_a=1.0, color=0.5, eumelanin=2.0)["absorption"] == scenes.HAIR_SIGMA_A
    assert scenes.hair(color=0.5, eumelanin=2.0)["absorption"] == scenes.HAIR_COLOR
    assert scenes.hair(pheomelanin=0.5) == dict(scenes.hair(eumelanin=0.0, pheomelanin=0.5))
    # ... and through the host: the three parametrisations and color = 1
    t = pbrt_hip.hair_tables(scenes.hair(color=(0.8, 0.5, 0.2), beta_n=0.3))
    assert np.array_equal(t["sigma_a"], hm.sigma_a_from_color(np.float32([0.8, 0.5, 0.2]).astype(np.float64), float(np.float32(0.3))).astype(np.float32))
    assert np.all(pbrt_hip.hair_tables(scenes.hair(color=1.0))["sigma_a"] == 0)
    t = pbrt_hip.hair_tables(scenes.hair())
    assert np.array_equal(t["sigma_a"], hm.sigma_a_from_melanin(float(np.float32(1.3)), 0.0).astype(np.float32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_host_tables_equal_the_model_bit_for_bit(i):
    t = pbrt_hip.hair_tables(DESCS[i])
    got = np.concatenate([t["sigma_a"], [t["eta"]], t["v"], [t["s"]], t["sin2k"], t["cos2k"]]).astype(np.float32)
    want = MODELS[i].tables()
    assert got.tobytes() == want.tobytes(), (got, want)


def test_left_out_share():
    for i in range(len(CASES)):
        h, wo, wi, u = points(100 + i)
        share = left_out(wo, wi).mean()
        assert share <= LEFT_OUT_MAX_SHARE, share
    print(f"left out: {share:.4f}")


REFUSED = [
    (dict(beta_m=1.5), "beta_m must be in [0, 1]"), (dict(beta_m=-0.1), "beta_m must be in [0, 1]"),
    (dict(beta_n=1.01), "beta_n must be in [0, 1]"), (dict(beta_n=-1.0), "beta_n must be in [0, 1]"),
    (dict(eta=0.0), "eta must be > 0"), (dict(eta=-1.0), "eta must be > 0"),
    (dict(sigma_a=(0.1, -0.1, 0.1)), "sigma_a must be >= 0"),
    (dict(eumelanin=-1.0), "eumelanin and pheomelanin must be >= 0"), (dict(pheomelanin=-0.5), "eumelanin and pheomelanin must be >= 0"),
    (dict(color=(0.5, 0.0, 0.5)), "color must be in (0, 1]"), (dict(color=(0.5, 1.5, 0.5)), "color must be in (0, 1]"),
    (dict(alpha=float("nan")), "every field must be finite"), (dict(sigma_a=(0.0, float("inf"), 0.0)), "every field must be finite"),
    (dict(eta=float("nan")), "every field must be finite"),
]


@pytest.mark.parametrize("kw,why", REFUSED, ids=[f"{list(k)[0]}-{n}" for n, (k, _) in enumerate(REFUSED)])
def test_refusals_without_a_scene(kw, why):
    with pytest.raises(pbrt_hip.PbrtHipError, match=why.replace("(", r"\(").replace("]", r"\]").replace("[", r"\[")):
        pbrt_hip.hair_tables(scenes.hair(**kw))


def test_unknown_absorption_is_refused():
    d = scenes.hair()
    d["absorption"] = 7
    with pytest.raises(pbrt_hip.PbrtHipError, match="unknown absorption"):
        pbrt_hip.hair_tables(d)
    with pytest.raises(pbrt_hip.PbrtHipError, match="null pointer"):
        pbrt_hip.hair_tables(None)


def test_abi_layout_of_the_hair_structs():
    """the layouts csrc/abi_guard.h asserts, restated by the binding"""
    D, T = pbrt_hip.HairDesc, pbrt_hip.HairTables
    assert ctypes.sizeof(D) == 52
    assert [getattr(D, k).offset for k in ("absorption", "sigma_a", "color", "eumelanin", "pheomelanin", "eta", "beta_m", "beta_n", "alpha")] == \
        [0, 4, 16, 28, 32, 36, 40, 44, 48]
    assert ctypes.sizeof(T) == 60
    assert [getattr(T, k).offset for k in ("sigma_a", "eta", "v", "s", "sin2k", "cos2k")] == [0, 12, 16, 32, 36, 48]
    for name in ("pbrt_hip_scene_set_hair_material", "pbrt_hip_hair_tables", "pbrt_hip_bsdf_query_hair"):
        assert name in pbrt_hip.EXPORTS and getattr(pbrt_hip.lib(), name)
