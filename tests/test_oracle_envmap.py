"""The CPU oracle's InfiniteAreaLight with an image map (oracle/src/o_render.h; OracleScene.set_environment_map) held to the
float64 model (envmap_model.py) before any device is compared with it: le on escaped rays with the tolerance
test_gpu_envmap.py holds the device to, pdf_li / sample_li through the probe entry point, the sun-map closed form and the
importance-sampling variance ratio of test_gpu_envmap.py with the same margins."""
import numpy as np
import pytest
from scipy import stats

import oracle
from pbrt_hip import scenes
import envmap_model as em
from envmap_cases import RHO, _closed_form, _escape_rays, _escape_scene, _gentle_map, _plane_camera, _plane_scene, _rot, _sun_map


def _model_tables(model):
    """InfiniteAreaLight::new's tables from the numpy model instead of the library's host code"""
    return model.l0.astype(np.float32), model.func.astype(np.float32), em.power(model.pyr).astype(np.float32)


def _map_300x140():
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0.1, 1.0, size=(140, 300, 3)).astype(np.float32)
    rgb[30:34, 200:204] = 500.0
    return rgb


MAPS = dict(gentle=_gentle_map, gentle300x140=lambda: _gentle_map(140, 300), m300x140=_map_300x140,
            m1x1=lambda: np.full((1, 1, 3), 0.7, np.float32))


def _le_tolerance(model, d, want, noisy):
    """rtol 2e-6, the device's (test_gpu_envmap.py). On the noisy 300x140 map with its hot spot that alone cannot hold for any
    float32 evaluation of infinite.rs:84-88: (u, v) = (phi / 2 pi, theta / pi) carry the float32 rounding of atan2 / acos and
    of the direction itself, about 2^-22 in v and 2^-22 (1 + 1 / sin theta) in u, which the lookup multiplies by the 512 x 256
    texels and by the contrast between neighbouring texels (uniform noise in [0.1, 1], a hot spot of 500): measured against the
    float64 model 51 % of the values lie beyond 2e-6, the worst at 1.2e-4 relative. There the oracle's value must be the model's
    at coordinates within that rounding: twice the model's own change over +-delta u, +-delta v is added to the bound."""
    tol = 2e-6 * np.abs(want)
    if not noisy:
        return tol
    u, v = model.uv(d)
    dv = 2.0 ** -22
    du = dv * (1 + 1 / np.maximum(np.sin(v * np.pi), 1e-6))
    for a, b in ((du, 0), (-du, 0), (0, dv), (0, -dv)):
        tol = np.maximum(tol, 2e-6 * np.abs(want) + 2 * np.abs(em.triangle(model.l0, u + a, np.clip(v + b, 0, 1)) - want))
    return tol


@pytest.mark.parametrize("tables", ["library", "model"])
@pytest.mark.parametrize("xf", ["identity", "rotation"])
@pytest.mark.parametrize("which", list(MAPS))
def test_le_on_escaped_rays_is_the_bilinear_lookup(which, xf, tables):
    """test_gpu_envmap.py::test_le_on_escaped_rays_is_the_bilinear_lookup on the oracle (rtol 2e-6, see _le_tolerance), at the
    seam, the poles, under a rotation, for 300x140 maps (resampled to 512x256) and for the 1x1 map; with the library's tables
    and with the model's."""
    rgb = MAPS[which]()
    L = (1.5, 1.0, 0.5)
    m = None if xf == "identity" else _rot((0.3, -0.5, 0.8), 37.0)
    model = em.EnvModel(rgb, L, m)
    sc = oracle.OracleScene(_escape_scene(L))
    sc.set_environment_map(0, rgb, m, tables=_model_tables(model) if tables == "model" else None)
    rays = _escape_rays()
    keys = np.arange(len(rays), dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    want = model.le(rays["d"].astype(np.float64))
    tol = _le_tolerance(model, rays["d"].astype(np.float64), want, which == "m300x140")
    for integ in (0, 1, 2):
        got, _ = sc.li(rays, keys, integrator=integ, max_depth=3)
        assert np.all(np.abs(got - want) <= tol), np.max(np.abs(got - want) / want)
    got, _ = sc.li(rays, keys, integrator=3, ao_samples=4)
    assert not got.any()  # ao.rs:66: nothing on a miss
    probe = sc.envmap_probe(0, rays["d"], np.zeros((len(rays), 2), np.float32))
    assert np.all(np.abs(probe["le"] - want) <= tol)
    sc.close()


@pytest.mark.parametrize("xf", ["identity", "rotation"])
@pytest.mark.parametrize("which", ["sun", "m300x140", "m1x1"])
def test_pdf_li_and_sample_li_follow_the_distribution(which, xf):
    """pdf_li against the model's solid-angle density, and sample_li's directions against that density by chi^2 over the
    Distribution2D's own cells. Tolerance of pdf_li, from the formats: func, marg_int and the 2 pi^2 sin(theta) are float32
    roundings of the model's values (6e-8 each); theta = acos(z) turns the float32 rounding of z (6e-8) into 6e-8 / sin(theta),
    i.e. 6e-8 / (sin(theta) tan(theta)) relative in sin(theta): 1.5e-6 at sin(theta) = 0.2, 2.4e-5 at 0.05. Held where
    sin(theta) > 0.2, to 1e-5, which covers the sum there. Directions within 1e-5 of a cell edge (in u or v) are left out:
    there float32 and float64 may name neighbouring cells."""
    rgb = _sun_map() if which == "sun" else MAPS[which]()
    m = None if xf == "identity" else _rot((0.2, 0.1, 1.0), 25.0)
    model = em.EnvModel(rgb, (1, 1, 1), m)
    sc = oracle.OracleScene(_escape_scene())
    sc.set_environment_map(0, rgb, m)
    rng = np.random.default_rng(5)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = 400_000
    u = rng.random((n, 2)).astype(np.float32)
    q = sc.envmap_probe(0, np.resize(d.astype(np.float32), (n, 3)), u)
    d32 = d.astype(np.float32).astype(np.float64)
    uu, vv = model.uv(d32)
    edge = lambda x, k: np.abs(x * k - np.round(x * k)) < 1e-5 * k  # noqa: E731
    ok = (np.sin(vv * np.pi) > 0.2) & ~edge(uu, model.nu) & ~edge(vv, model.nv)
    assert ok.mean() > 0.8
    np.testing.assert_allclose(q["pdf"][:len(d)][ok], model.pdf(d32)[ok], rtol=1e-5)
    # sample_li: every sample has a pdf, it is pdf_li of its own direction, Li is le of it
    assert np.all(q["pdf_s"] > 0) and np.isfinite(q["pdf_s"]).all()
    back = sc.envmap_probe(0, q["wi_s"], u)
    us, vs = model.uv(q["wi_s"].astype(np.float64))
    inner = (np.sin(vs * np.pi) > 0.2) & ~edge(us, model.nu) & ~edge(vs, model.nv)
    np.testing.assert_allclose(back["pdf"][inner], q["pdf_s"][inner], rtol=1e-5)
    # le(wi_s) recomputes (u, v) from the direction; a texel's bilinear weights move by 2e-7 * W per unit of u, so the
    # looked-up value moves by that times the map's contrast: held only where the map is smooth (not the sun / hot texels)
    if which == "m1x1":
        np.testing.assert_allclose(back["le"], q["li_s"], rtol=2e-6)
    # the sampled directions are distributed by func over the nu x nv cells
    iu = np.clip((us * model.nu).astype(np.int64), 0, model.nu - 1)
    iv = np.clip((vs * model.nv).astype(np.int64), 0, model.nv - 1)
    obs = np.bincount(iv * model.nu + iu, minlength=model.nu * model.nv).astype(np.float64)
    exp = (model.func / model.func.sum()).reshape(-1) * n
    small = exp < 5
    e, o = np.append(exp[~small], exp[small].sum()), np.append(obs[~small], obs[small].sum())
    keep = e > 0
    chi2 = np.sum((o[keep] - e[keep]) ** 2 / e[keep])
    p = stats.chi2.sf(chi2, keep.sum() - 1)
    assert p > 1e-3, (chi2, keep.sum(), p)
    sc.close()


def test_a_black_map_has_no_samples():
    """D61: a black map's pdf is 0 and sample_li returns nothing."""
    sc = oracle.OracleScene(_escape_scene())
    sc.set_environment_map(0, np.zeros((4, 8, 3), np.float32))
    d = np.array([[0.3, 0.2, 0.8], [1.0, 0.0, 0.0]], np.float32)
    q = sc.envmap_probe(0, d, np.array([[0.3, 0.6], [0.9, 0.1]], np.float32))
    assert not q["pdf"].any() and not q["pdf_s"].any() and not q["li_s"].any() and not q["le"].any()
    sc.close()


def _check_closed_form(sc, model, integrator, strategy, w=64, h=64, spp=16, seed=1):
    film, _ = sc.render(scenes.camera_dict_to_floats(_plane_camera(w, h)), w, h, spp, integrator=integrator, max_depth=1,
                        light_strategy=strategy, seed=seed)
    rgb = oracle.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    assert np.isfinite(rgb).all()
    want = _closed_form(model)
    mean, sigma = rgb.mean(axis=0), rgb.std(axis=0) / np.sqrt(len(rgb))
    assert (np.abs(mean - want) <= 4 * sigma + 1e-4 * want).all(), (integrator, strategy, mean, want, sigma)
    return rgb


CASES = [(0, 0), (0, 1), (0, 2), (1, 0)]  # (integrator, light strategy) as in test_gpu_envmap.py


@pytest.mark.parametrize("instanced", [False, True])
@pytest.mark.parametrize("xf", ["identity", "rotation"])
def test_closed_form_under_a_sun_map(xf, instanced):
    rgb = _sun_map()
    m = None if xf == "identity" else _rot((0.2, 0.1, 1.0), 25.0)
    model = em.EnvModel(rgb, (1, 1, 1), m)
    sc = oracle.OracleScene(_plane_scene(instanced=instanced))
    sc.set_environment_map(0, rgb, m)
    for integ, strat in CASES:
        _check_closed_form(sc, model, integ, strat)
    sc.close()


def test_a_300x140_map():
    rgb = _map_300x140()
    model = em.EnvModel(rgb)
    sc = oracle.OracleScene(_plane_scene())
    sc.set_environment_map(0, rgb)
    for integ, strat in CASES[1:3]:
        _check_closed_form(sc, model, integ, strat)
    sc.close()


def test_importance_sampling_follows_the_map():
    """test_gpu_envmap.py::test_importance_sampling_follows_the_map on the oracle, same margins."""
    rgb = _sun_map()
    model = em.EnvModel(rgb)
    sc = oracle.OracleScene(_plane_scene(extra_zero_light=False))
    sc.set_environment_map(0, rgb)
    w = h = 128
    film, _ = sc.render(scenes.camera_dict_to_floats(_plane_camera(w, h)), w, h, 1, integrator=1, max_depth=1, light_strategy=0, seed=3)
    px = oracle.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    d, dw = model.directions(8 * model.l0.shape[0], 8 * model.l0.shape[1])
    cos = np.clip(d[:, 2], 0, None)
    le = model.le(d)
    p_l = model.pdf(d)
    p_b = cos / np.pi
    f = RHO / np.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        w_l = np.where(p_l > 0, p_l ** 2 / (p_l ** 2 + p_b ** 2), 0.0)
        w_b = np.where(p_b > 0, p_b ** 2 / (p_l ** 2 + p_b ** 2), 0.0)
        g_l = (f * le * (cos * w_l)[:, None])
        g_b = (f * le * (cos * w_b)[:, None])
        m_l = (g_l * dw[:, None]).sum(0)
        m_b = (g_b * dw[:, None]).sum(0)
        s_l = np.where(p_l[:, None] > 0, g_l ** 2 / p_l[:, None], 0.0)
        s_b = np.where(p_b[:, None] > 0, g_b ** 2 / p_b[:, None], 0.0)
    var = (s_l * dw[:, None]).sum(0) - m_l ** 2 + (s_b * dw[:, None]).sum(0) - m_b ** 2
    got = px.var(axis=0)
    ratio = got / var
    assert ((ratio > 0.5) & (ratio < 1.5)).all(), (got, var)
    var_uniform = ((f * le * cos[:, None]) ** 2 * (4 * np.pi) * dw[:, None]).sum(0) - (m_l + m_b) ** 2
    assert (var_uniform > 20 * var).all()
    sc.close()


def test_the_constant_light_is_unchanged_by_the_map_code():
    """An infinite light without a map keeps the constant path: le = L on every ray, the 2x2 table's density 1 / (4 pi)."""
    L = (0.3, 0.4, 0.5)
    sc = oracle.OracleScene(_escape_scene(L))
    rays = _escape_rays()
    q = sc.envmap_probe(0, rays["d"], np.random.default_rng(1).random((len(rays), 2)).astype(np.float32))
    assert np.array_equal(q["le"], np.broadcast_to(np.array(L, np.float32), q["le"].shape))
    assert np.array_equal(q["li_s"], q["le"])
    z = np.abs(rays["d"][:, 2].astype(np.float64))
    inner = z < 0.999
    # the 2x2 table: density sin(theta_row) / (sum of the two rows' sines) * 2 / (2 pi^2 sin(theta)), theta_row = pi/4, 3pi/4
    want = 1.0 / (2 * np.pi ** 2 * np.sqrt(1 - z[inner] ** 2))
    np.testing.assert_allclose(q["pdf"][inner], want, rtol=1e-5)
    sc.close()


def test_instanced_and_two_level_scenes_take_the_map():
    """set_environment_map on the instanced and the two-level constructors names the same light as on the device (the
    instanced oracle scene lists no area lights) and gives the light the single-level scene has: le, pdf_li and sample_li
    equal bit for bit."""
    rgb, m = _sun_map(), _rot((0.2, 0.1, 1.0), 25.0)
    rays = _escape_rays()
    u = np.random.default_rng(2).random((len(rays), 2)).astype(np.float32)
    ref_scene = oracle.OracleScene(_escape_scene((0.2, 0.25, 0.3)))
    ref_scene.set_environment_map(0, rgb, m)
    want = ref_scene.envmap_probe(0, rays["d"], u)
    two = scenes.two_level_scene()
    inst = scenes.instanced_scene(n_base_tris=200, n_instances=5, extent=1.5, env_L=(0.2, 0.25, 0.3))
    # an area light row in front of the infinite light: the device's index counts it, the instanced oracle scene's list does not
    inst = scenes.with_lights(dict(inst, lights=scenes._lights([(scenes.LIGHT_DIFFUSE_AREA, (1.0, 1.0, 1.0), 0, 0, 1)])), inst["lights"])
    for sc in (two, inst):
        light = int(np.nonzero(sc["lights"]["type"] == scenes.LIGHT_INFINITE)[0][0])
        assert tuple(sc["lights"]["L"][light]) == tuple(np.float32((0.2, 0.25, 0.3)))
        osc = oracle.OracleScene(sc)
        osc.set_environment_map(light, rgb, m)
        got = osc.envmap_probe(light, rays["d"], u)
        for k in ("le", "pdf", "wi_s", "li_s", "pdf_s"):
            assert np.array_equal(got[k], want[k]), k
        with pytest.raises(ValueError):
            osc.set_environment_map(len(sc["lights"]), rgb, m)
        osc.close()
    ref_scene.close()
