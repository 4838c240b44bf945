"""The references of test_gpu_mis_materials.py held to themselves (mis_cases.py), with the float64 models alone: the rectangle
quadrature against the closed-form configuration factor, the sphere quadrature against the models' own albedo, and the
conditions the cases must meet to be worth running: both MIS regimes are there, every wrong estimator a slip in estimate_direct
would amount to misses the reference by far more than the reference is uncertain, the specular directions stay clear of the
emitters' edges, and the grazing band of glossy transmission carries next to nothing. No GPU."""
import numpy as np
import pytest

import bxdf_model as bm
import envmap_model as em
import mis_cases as mc

LIGHT_CASES = [(v, e) for v in mc.VIEWS for e in mc.EMITTERS]
LIGHT_IDS = [f"{mc.view_name(v)}-{e}" for v, e in LIGHT_CASES]


def _threshold(r):
    """what a wrong estimator must differ by: 10 times the quadrature's error plus 1e-4 of the reference"""
    return 10.0 * r["err"] + 1e-4 * r["ref"]


def _configuration_factor(p, corners):
    """from a surface element at p (normal +z) to a rectangle parallel to it: the four-corner sum of
    1 / (2 pi) [x / sqrt(1 + x^2) atan(y / sqrt(1 + x^2)) + y / sqrt(1 + y^2) atan(x / sqrt(1 + y^2))], x and y the corner's
    offsets from the point over the height"""
    def g(x, y):
        a, b = np.sqrt(1 + x * x), np.sqrt(1 + y * y)
        return (x / a * np.arctan(y / a) + y / b * np.arctan(x / b)) / (2 * np.pi)

    h = corners[0, 2] - p[2]
    x0, x1 = (corners[:, 0].min() - p[0]) / h, (corners[:, 0].max() - p[0]) / h
    y0, y1 = (corners[:, 1].min() - p[1]) / h, (corners[:, 1].max() - p[1]) / h
    return g(x1, y1) - g(x0, y1) - g(x1, y0) + g(x0, y0)


@pytest.mark.parametrize("emitter", ["near", "far"])
def test_rectangle_quadrature_reproduces_the_configuration_factor(emitter):
    """f = rho / pi: L rho F with the closed-form F, at three of the plane points (the last outside the near emitter's
    footprint, all outside the far one's). The midpoint rule's error falls by four per halving, so the change from half the grid
    is three times the fine grid's error: the tolerance is that change."""
    rho = np.array([0.6, 0.5, 0.4])
    corners = mc.emitter_corners(emitter, 1)
    inside = [bool(abs(p[0] - mc.EMITTERS[emitter][0][0]) < mc.EMITTERS[emitter][2][0] and abs(p[1] - mc.EMITTERS[emitter][0][1]) < mc.EMITTERS[emitter][2][1])
              for p in mc.POINTS[[0, 2, 3]]]
    assert not inside[2]
    for p in mc.POINTS[[0, 2, 3]]:
        value, err, share = mc.quad_light_radiance(lambda wo, wi: np.where(wi[:, 2:3] > 0, rho / np.pi, 0.0), bm.cos_pdf, p, mc.FRAME,
                                                   np.array([0.3, 0.2, 0.933]), corners, mc.LE, False, mc.CELLS)
        want = mc.LE * rho * _configuration_factor(p, corners)
        print(f"{emitter} at {p[:2]}: quadrature {value} closed form {want} halving error {err}, off by {np.abs(value - want)}, share {share:.3f}")
        assert (err < 1e-3 * want).all() and 0.0 < share < 1.0
        assert (np.abs(value - want) <= err + 1e-12).all()
    # facing away nothing arrives, and read as two-sided the same as facing the plane
    away = mc.emitter_corners("away", 1)
    f = lambda wo, wi: np.where(wi[:, 2:3] > 0, rho / np.pi, 0.0)  # noqa: E731
    assert (mc.quad_light_radiance(f, bm.cos_pdf, mc.POINTS[0], mc.FRAME, np.array([0.0, 0.0, 1.0]), away, mc.LE, False, 64)[0] == 0.0).all()
    a = mc.quad_light_radiance(f, bm.cos_pdf, mc.POINTS[0], mc.FRAME, np.array([0.0, 0.0, 1.0]), away, mc.LE, True, 64)[0]
    b = mc.quad_light_radiance(f, bm.cos_pdf, mc.POINTS[0], mc.FRAME, np.array([0.0, 0.0, 1.0]), mc.emitter_corners("near", 1), mc.LE, False, 64)[0]
    np.testing.assert_allclose(a, b, rtol=1e-12)


CONSTANT_VIEWS = [v for v in mc.ENV_VIEWS if v[2] == 0]


@pytest.mark.parametrize("view", CONSTANT_VIEWS, ids=[mc.env_view_name(v) for v in CONSTANT_VIEWS])
def test_sphere_quadrature_of_a_constant_map_is_the_albedo(view):
    """under a constant map the sphere quadrature plus the specular term is Le albedo(wo), the models' own albedo (Gauss-Legendre
    nodes split at the BSDF's kinks: another rule on another grid). Tolerance: twice the sum of the two halving errors (a halving
    error estimates an error, it does not bound it)."""
    le = np.array([1.0, 0.8, 0.6])
    env = em.EnvModel(np.ones((8, 16, 3), np.float32), le, mc.ENV_TO_WORLD)
    row, wo = mc.ROWS[view[0]], mc.env_wo(view)
    value, err, share = mc.envmap_radiance(row.f, row.pdf, mc.FRAME, wo, env, 128)
    if row.specular is not None:
        value = value + mc.specular_term(row.specular, wo, lambda wi: le)[0]
    albedo, coarse = row.albedo(wo, 128), row.albedo(wo, 64)
    tol = 2.0 * (err + le * np.abs(albedo - coarse))
    print(f"{mc.env_view_name(view)}: quadrature {value} Le albedo {le * albedo}, off by {np.abs(value - le * albedo)}, tolerance {tol}, share {share:.3f}")
    assert (tol < 5e-3 * value).all()
    assert (np.abs(value - le * albedo) <= tol).all()


@pytest.mark.parametrize("name", mc.GLOSSY_OR_TRANSMISSIVE)
def test_both_mis_regimes_are_present(name):
    """for every row with a glossy or transmissive lobe, by the model: some (emitter, point) puts at least half of the estimate on
    the BSDF-sampled half, and some puts at most a fifth there"""
    shares = []
    for view in mc.VIEWS:
        if view[0] != name:
            continue
        for e in ("near", "far"):
            r = mc.light_reference(view, e)
            lit = r["quad"].sum(axis=1) > 0
            shares += list(r["share"][lit])
            print(f"{mc.view_name(view)} {e}: BSDF-branch share {np.round(r['share'], 4)}")
    assert max(shares) >= 0.5 and min(shares) <= 0.2, (min(shares), max(shares))


@pytest.mark.parametrize("view,emitter", LIGHT_CASES, ids=LIGHT_IDS)
def test_area_light_cases_tell_wrong_estimators_apart(view, emitter):
    """What a slip in estimate_direct would compute, by the model, against the reference of each case (four points, three
    channels): the light-sampled half alone, the BSDF-sampled half alone, a light pdf without cos_s in the BSDF-sampled half's
    weight, a one-sided emitter read as two-sided (the emitter facing away), the BSDF sampled under BSDF_ALL (where a specular
    direction meets the emitter: elsewhere that estimator has the reference's expectation). Each misses the reference by more
    than 10 quadrature errors + 1e-4 ref somewhere in the case, which is what a comparison of the case would report. Where the
    row scatters nothing but specular lobes towards the emitter (uber from across the plane) there is no MIS estimate to get wrong,
    and where the emitter faces away only its side can be."""
    r = mc.light_reference(view, emitter)
    row, thr = mc.ROWS[view[0]], _threshold(r)
    faces, mis = mc.EMITTERS[emitter][4], r["quad"].sum() > 0
    told = {}
    if faces and mis:
        told["light half alone"] = r["bsdf"] > thr                    # misses by the BSDF-sampled half's part
        told["BSDF half alone"] = r["quad"] - r["bsdf"] > thr
        told["light pdf without cos_s"] = np.abs(r["no_cos"] - r["quad"]) > thr
    if not faces:
        assert (r["ref"] == 0.0).all() and (r["err"] == 0.0).all()
        told["read as two-sided"] = r["as_two_sided"] > thr
    if r["spec_hits"].any():
        told["sampled under BSDF_ALL"] = r["all_extra"] > thr
    print(f"{mc.view_name(view)} {emitter}: green {r['ref'][:, 1]} relative error {np.max(r['err'] / np.maximum(r['ref'], 1e-300)):.2g} "
          f"share {np.round(r['share'], 4)}; points told apart: " + ", ".join(f"{k} {v.any(axis=1).sum()}" for k, v in told.items()))
    assert told or (view[0] == "uber" and view[1] != view[2] and not r["ref"].any())
    for what, t in told.items():
        assert t.any(), what
    if faces and mis:
        assert (r["err"] <= 1e-3 * r["quad"]).all()
    if row.specular is not None and emitter == "near":
        assert r["spec_hits"].all()   # every row with specular lobes meets the BSDF_ALL condition at every point of a case


@pytest.mark.parametrize("view,emitter", LIGHT_CASES, ids=LIGHT_IDS)
def test_margins(view, emitter):
    """specular directions hit or miss the emitter by at least 0.05 of its half-size, no point lies under an edge or on the
    plane's diagonal, the eye's rays start between the plane and the emitter, and the grazing band of glossy transmission
    (bxdf_cases.in_band), where the device is held to the model less tightly, carries no more of a reference than the part of the
    acceptance that is not statistical: the quadrature's error + 1e-4 ref"""
    r = mc.light_reference(view, emitter)
    assert (r["margin"] >= 0.05).all(), r["margin"]
    (cx, cy), h, (hx, hy), _, _ = mc.EMITTERS[emitter]
    for p in mc.POINTS:
        assert abs(abs(p[0] - cx) - hx) >= 0.05 * hx and abs(abs(p[1] - cy) - hy) >= 0.05 * hy and p[0] - p[1] >= 0.1
    rays = mc.view_rays(view, emitter)
    assert (np.abs(rays["o"][:, 2]) < 0.5 * h).all() and (np.sign(rays["o"][:, 2]) == view[1]).all()
    print(f"{mc.view_name(view)} {emitter}: band over reference {np.max(r['band'] / np.maximum(r['ref'], 1e-300)):.2g}")
    assert (r["band"] <= r["err"] + 1e-4 * r["ref"]).all(), (r["band"], r["err"], r["ref"])


@pytest.mark.parametrize("view", mc.ENV_VIEWS, ids=[mc.env_view_name(v) for v in mc.ENV_VIEWS])
def test_environment_cases_tell_wrong_estimators_apart(view):
    """as the area-light cases, under the image map: either half alone, env_pdf evaluated without light_to_world in the
    BSDF-sampled half's weight, and the BSDF sampled under BSDF_ALL (the environment is met along every specular direction)"""
    r = mc.env_reference(view)
    thr = _threshold(r)
    told = {"light half alone": r["bsdf"] > thr, "BSDF half alone": r["quad"] - r["bsdf"] > thr,
            "pdf without light_to_world": np.abs(r["wrong_pdf"] - r["quad"]) > thr}
    if mc.ROWS[view[0]].specular is not None:
        told["sampled under BSDF_ALL"] = r["all_extra"] > thr
    print(f"{mc.env_view_name(view)}: {r['ref']} relative error {np.max(r['err'] / r['ref']):.2g} share {r['share']:.3f} band over reference "
          f"{np.max(r['band'] / r['ref']):.2g}; wrong pdf off by {np.abs(r['wrong_pdf'] - r['quad']) / r['ref']}")
    for what, t in told.items():
        assert t.any(), what
    assert (r["err"] <= 1e-3 * r["ref"]).all()
    assert (r["band"] <= r["err"] + 1e-4 * r["ref"]).all(), (r["band"], r["err"], r["ref"])


def test_the_map_and_the_rotations_are_generic():
    """the map's bright block holds a large part of its power, light_to_world and the scene's rotation move every axis, and
    env_pdf without light_to_world is another function"""
    env, unrotated = mc.env_models()
    d, dw = env.directions(64, 128)
    power = (env.le(d) @ em.Y) * dw
    assert 0.25 < power[env.le(d)[:, 1] > 2.0].sum() / power.sum() < 0.9
    assert abs((env.pdf(d) * dw).sum() - 1.0) < 0.02
    assert np.abs(env.pdf(d) - unrotated.pdf(d)).max() > 0.1
    for m in (mc.ROTATION, mc.ENV_TO_WORLD[:3, :3].astype(np.float64)):
        np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-6)
        assert np.abs(m).max() < 0.95
