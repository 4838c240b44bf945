"""InfiniteAreaLight with an image map on the device (Scene.set_environment_map): le on escaped rays, sample_li / pdf_li
through MIS against closed forms of the float64 model (envmap_model.py), importance sampling by the map's Distribution2D,
the 1x1 map = the constant light, instanced scenes, the spatial tables rebuilt, refusals that leave the scene usable."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import envmap_model as em
from envmap_cases import (RHO, _closed_form, _escape_rays, _escape_scene, _gentle_map, _plane_camera, _plane_scene, _rot,
                          _sun_map)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("xf", ["identity", "rotation"])
def test_le_on_escaped_rays_is_the_bilinear_lookup(hip_ctx, xf):
    rgb = _gentle_map()
    L = (1.5, 1.0, 0.5)
    m = None if xf == "identity" else _rot((0.3, -0.5, 0.8), 37.0)
    sc = pbrt_hip.Scene(hip_ctx, _escape_scene(L))
    sc.set_environment_map(0, rgb, m)
    model = em.EnvModel(rgb, L, m)
    rays = _escape_rays()
    keys = np.arange(len(rays), dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    want = model.le(rays["d"].astype(np.float64))
    for integ in (pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT):
        got, _ = sc.li(rays, keys, integrator=integ, max_depth=3)
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
    got, _ = sc.li(rays, keys, integrator=pbrt_hip.INTEGRATOR_AO, ao_samples=4)
    assert not got.any()  # ao.rs:66: nothing on a miss
    # the seam is wrapped: the values at u ~ 0 and u ~ 1 blend the first and last columns
    if xf == "identity":
        seam = model.le(np.array([[1.0, 1e-4, 0.1], [1.0, -1e-4, 0.1]]))
        assert abs(seam[0, 0] - seam[1, 0]) < 1e-3 * seam[0, 0]
    sc.close()


def _check_closed_form(sc, model, integrator, strategy, w=64, h=64, spp=16, seed=1):
    film, _ = sc.render(_plane_camera(w, h), w, h, spp, integrator=integrator, max_depth=1, light_strategy=strategy, seed=seed)
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    assert np.isfinite(rgb).all()
    want = _closed_form(model)
    mean, sigma = rgb.mean(axis=0), rgb.std(axis=0) / np.sqrt(len(rgb))
    assert (np.abs(mean - want) <= 4 * sigma + 1e-4 * want).all(), (integrator, strategy, mean, want, sigma)
    return rgb


CASES = [(pbrt_hip.INTEGRATOR_PATH, 0), (pbrt_hip.INTEGRATOR_PATH, 1), (pbrt_hip.INTEGRATOR_PATH, 2), (pbrt_hip.INTEGRATOR_DIRECT, 0)]


@pytest.mark.parametrize("xf", ["identity", "rotation"])
def test_closed_form_under_a_sun_map(hip_ctx, xf):
    rgb = _sun_map()
    m = None if xf == "identity" else _rot((0.2, 0.1, 1.0), 25.0)
    model = em.EnvModel(rgb, (1, 1, 1), m)
    y = model.l0 @ em.Y
    assert y[8:10, 11:13].sum() >= 0.99 * y.sum()
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene())
    sc.set_environment_map(0, rgb, m)
    for integ, strat in CASES:
        _check_closed_form(sc, model, integ, strat)
    sc.close()


def test_importance_sampling_follows_the_map(hip_ctx):
    """DirectLightingIntegrator, UniformSampleAll, one sample: the per-pixel variance of the MIS estimator (light sample by
    the map's Distribution2D + BSDF sample by cos / pi) is what the model predicts by quadrature."""
    rgb = _sun_map()
    model = em.EnvModel(rgb)
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene(extra_zero_light=False))
    sc.set_environment_map(0, rgb)
    w = h = 128
    film, _ = sc.render(_plane_camera(w, h), w, h, 1, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0, seed=3)
    px = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    d, dw = model.directions(8 * model.l0.shape[0], 8 * model.l0.shape[1])
    cos = np.clip(d[:, 2], 0, None)
    le = model.le(d)
    p_l = model.pdf(d)
    p_b = cos / np.pi
    f = RHO / np.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        w_l = np.where(p_l > 0, p_l ** 2 / (p_l ** 2 + p_b ** 2), 0.0)
        w_b = np.where(p_b > 0, p_b ** 2 / (p_l ** 2 + p_b ** 2), 0.0)
        g_l = (f * le * (cos * w_l)[:, None])            # integrand of the light half
        g_b = (f * le * (cos * w_b)[:, None])
        m_l = (g_l * dw[:, None]).sum(0)
        m_b = (g_b * dw[:, None]).sum(0)
        s_l = np.where(p_l[:, None] > 0, g_l ** 2 / p_l[:, None], 0.0)
        s_b = np.where(p_b[:, None] > 0, g_b ** 2 / p_b[:, None], 0.0)
    var = (s_l * dw[:, None]).sum(0) - m_l ** 2 + (s_b * dw[:, None]).sum(0) - m_b ** 2
    got = px.var(axis=0)
    ratio = got / var
    assert ((ratio > 0.5) & (ratio < 1.5)).all(), (got, var)
    # what a 2 x 2 table would give: sampling by the sin-weighted constant (p = 1 / (4 pi)) instead
    var_uniform = ((f * le * cos[:, None]) ** 2 * (4 * np.pi) * dw[:, None]).sum(0) - (m_l + m_b) ** 2
    assert (var_uniform > 20 * var).all()
    sc.close()


@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_a_1x1_white_map_is_the_constant_light(hip_ctx, name):
    w = h = 64
    if name == "cornell":
        sc = scenes.with_lights(scenes.cornell_box(), scenes._lights([(scenes.LIGHT_INFINITE, (0.3, 0.4, 0.5), -1, 0, 1)]))
        cam, kw = scenes.cornell_camera(w, h), dict(max_depth=8, seed=0)
    else:
        sc = scenes.mixed_materials_scene()
        cam, kw = scenes.random_triangles_camera(w, h), dict(max_depth=16, seed=5)
    inf = int(np.nonzero(sc["lights"]["type"] == scenes.LIGHT_INFINITE)[0][0])
    plain = pbrt_hip.Scene(hip_ctx, sc)
    before, _ = plain.render(cam, w, h, 4, **kw)
    mapped = pbrt_hip.Scene(hip_ctx, sc)
    mapped.set_environment_map(inf, np.ones((1, 1, 3), np.float32))
    got, _ = mapped.render(cam, w, h, 4, **kw)
    a, b = pbrt_hip.film_to_rgb(before).astype(np.float64), pbrt_hip.film_to_rgb(got).astype(np.float64)
    rel_rmse = np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(a ** 2))
    assert rel_rmse <= 1e-6, rel_rmse
    after, _ = plain.render(cam, w, h, 4, **kw)  # another scene's map leaves this one alone
    assert np.array_equal(before, after)
    plain.close()
    mapped.close()


def test_a_300x140_map(hip_ctx):
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0.1, 1.0, size=(140, 300, 3)).astype(np.float32)
    rgb[30:34, 200:204] = 500.0
    model = em.EnvModel(rgb)
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene())
    sc.set_environment_map(0, rgb)
    for integ, strat in CASES[1:3]:
        _check_closed_form(sc, model, integ, strat)
    sc.close()


def test_instanced_scene_meets_the_closed_form(hip_ctx):
    rgb = _sun_map()
    model = em.EnvModel(rgb)
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene(instanced=True))
    sc.set_environment_map(0, rgb)
    for integ, strat in CASES:
        _check_closed_form(sc, model, integ, strat)
    sc.close()


def test_spatial_tables_are_rebuilt_after_a_new_map(hip_ctx):
    w = h = 64
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene())
    sc.render(_plane_camera(w, h), w, h, 4, max_depth=1, light_strategy=2, seed=1)  # builds the spatial tables (constant map)
    rgb = _sun_map()
    sc.set_environment_map(0, rgb)
    got = _check_closed_form(sc, em.EnvModel(rgb), pbrt_hip.INTEGRATOR_PATH, 2)
    fresh = pbrt_hip.Scene(hip_ctx, _plane_scene())
    fresh.set_environment_map(0, rgb)
    want = _check_closed_form(fresh, em.EnvModel(rgb), pbrt_hip.INTEGRATOR_PATH, 2)
    assert np.array_equal(got, want)
    # and once more, a second map on the same light replaces the first
    rgb2 = _sun_map(sun=(20, 40), level=800.0)
    sc.set_environment_map(0, rgb2)
    _check_closed_form(sc, em.EnvModel(rgb2), pbrt_hip.INTEGRATOR_PATH, 2)
    sc.close()
    fresh.close()


def test_refusals_leave_the_scene_usable(hip_ctx):
    w = h = 32
    sc = pbrt_hip.Scene(hip_ctx, _plane_scene())
    rgb = _sun_map()
    sing = np.eye(4, dtype=np.float32)
    sing[2, :3] = sing[0, :3]
    bad = rgb.copy()
    bad[3, 4, 1] = np.nan
    non_affine = np.eye(4, dtype=np.float32)
    non_affine[3, 2] = 0.5
    for args in [(1, rgb, None), (2, rgb, None), (-1, rgb, None), (0, rgb, sing), (0, bad, None), (0, rgb, non_affine),
                 (0, rgb, np.full((4, 4), np.nan, np.float32)), (0, -rgb, None)]:
        with pytest.raises(pbrt_hip.PbrtHipError):
            sc.set_environment_map(*args)
        film, _ = sc.render(_plane_camera(w, h), w, h, 2, max_depth=1, seed=2)
        assert np.isfinite(film).all() and film[..., 3].sum() > 0
    # still the constant light: the quad under a white sky radiates rho
    rgb_out = pbrt_hip.film_to_rgb(film)
    np.testing.assert_allclose(rgb_out.mean(), RHO, rtol=0.05)
    sc.close()
