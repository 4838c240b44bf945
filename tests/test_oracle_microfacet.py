"""The CPU oracle's plastic and metal (oracle/src/o_microfacet.h, o_reflection.h) held to the float64 model
(microfacet_model.py) before any device is compared with it: orc_bsdf_query with the material table, directions, masks and
tolerances that test_gpu_glossy.py holds the device's pbrt_hip_bsdf_query to (glossy_cases.py), the chi^2 cases of its
sampler, and the closed forms through OracleScene.li / OracleScene.render with the same reference values and margins."""
import numpy as np
import pytest
from scipy import stats

import oracle
from pbrt_hip import scenes
import microfacet_model as mm
from glossy_cases import CASES, CHI2, ETA, K, _directions, _point_light_rays, _rel_check, _table_scene, _unit

BSDF_REFLECTION, BSDF_DIFFUSE, BSDF_GLOSSY = 1, 4, 8  # reflection.rs:162-170


@pytest.fixture(scope="module")
def table():
    scene = oracle.OracleScene(_table_scene([c[1] for c in CASES]))
    for i, c in enumerate(CASES):
        if c[2] is not None:
            scene.set_material_roughness(i, c[2][0], c[2][1], remap=c[2][2])
    yield scene
    scene.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bsdf_query_matches_model(table, i):
    """test_gpu_glossy.py::test_bsdf_query_matches_model with the oracle in the device's place."""
    m = CASES[i][3]
    wo, wi, u = _directions(20000, 100 + i)
    q = table.bsdf_query(i, wo, wi, u)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f_ref, pdf_ref = mm.bsdf_f(m, wo64, wi64), mm.bsdf_pdf(m, wo64, wi64)
    ok = (np.abs(wo64[:, 2]) >= 1e-3) & (np.abs(wi64[:, 2]) >= 1e-3) & (np.linalg.norm(wo64 + wi64, axis=1) > 1e-2)
    wh = _unit(wo64 + wi64 + 1e-30)
    rtol = np.where((min(m.ax, m.ay) < 0.01) & (1 - wh[:, 2] ** 2 < 0.05), 2e-2, 1e-4)
    _rel_check(q["f"], f_ref, np.repeat(ok[:, None], 3, 1), "f", np.repeat(rtol[:, None], 3, 1))
    _rel_check(q["pdf"], pdf_ref, ok, "pdf", rtol)
    wi_m, f_m, pdf_m, ok_m, glossy_m = mm.bsdf_sample_f(m, wo64, u)
    ok_d = q["pdf_s"] > 0
    sel = np.abs(wo64[:, 2]) >= 1e-3
    assert np.mean(ok_d[sel] != ok_m[sel]) < 1e-3
    both = sel & ok_d & ok_m
    assert both.sum() > 0.3 * sel.sum()
    ws = np.abs(wo64) * np.array([m.ax, m.ay, 1.0])
    normal_branch = glossy_m & (ws[:, 2] / np.linalg.norm(ws, axis=1) > 0.9999)
    cmp = both & ~normal_branch
    dw = np.abs(q["wi_s"][cmp] - wi_m[cmp]).max(axis=1)
    assert cmp.sum() > 0.2 * sel.sum() and np.mean(dw > 1e-3) < 1e-3, np.sort(dw)[-5:]
    flags = q["flags"][both]
    expect = np.where(glossy_m[both], BSDF_GLOSSY, BSDF_DIFFUSE) | BSDF_REFLECTION
    assert np.mean(flags == expect) > 0.999
    assert np.all(q["flags"][~ok_d] == 0)
    q2 = table.bsdf_query(i, wo[ok_d], q["wi_s"][ok_d], u[ok_d])
    if min(m.ax, m.ay) < 0.01:
        assert np.median(np.abs(q["pdf_s"][ok_d] / q2["pdf"] - 1)) < 1e-2
        assert np.median(np.abs(q["f_s"][ok_d] / np.maximum(q2["f"], 1e-30) - 1)) < 1e-2
    else:
        np.testing.assert_allclose(q["pdf_s"][ok_d], q2["pdf"], rtol=2e-3)
        np.testing.assert_allclose(q["f_s"][ok_d], q2["f"], rtol=2e-3, atol=1e-6 * np.abs(q2["f"]).max())


@pytest.mark.parametrize("name,i,theta_o", CHI2, ids=[f"{c[0]}-{c[2]:g}" for c in CHI2])
def test_sampler_chi2(table, name, i, theta_o):
    """test_gpu_glossy.py::test_sampler_chi2 with the oracle in the device's place."""
    n = 1_000_000
    m = CASES[i][3]
    t = np.radians(theta_o)
    wo = np.array([np.sin(t) * np.cos(0.7), np.sin(t) * np.sin(0.7), np.cos(t)])
    u = np.random.default_rng(7 + i).random((n, 2)).astype(np.float32)
    wo32 = np.broadcast_to(wo.astype(np.float32), (n, 3)).copy()
    q = table.bsdf_query(i, wo32, wo32, u)
    ok = q["pdf_s"] > 0
    expected = mm.pdf_bins(m, wo.astype(np.float32).astype(np.float64)).reshape(-1) * n
    counts = np.bincount(mm.bin_of(q["wi_s"][ok].astype(np.float64)), minlength=expected.size)
    exp = np.append(expected, max(n - expected.sum(), 0.0))
    obs = np.append(counts, n - ok.sum())
    small = exp < 5
    e = np.append(exp[~small], exp[small].sum())
    o = np.append(obs[~small], obs[small].sum())
    keep = e > 0
    assert np.all(o[~keep] == 0), "samples where the pdf has no mass"
    chi2 = np.sum((o[keep] - e[keep]) ** 2 / e[keep])
    p = stats.chi2.sf(chi2, keep.sum() - 1)
    assert p > 1e-3, (chi2, keep.sum(), p)


def test_scene_query_is_the_row_query(table):
    """OracleScene.bsdf_query = orc_bsdf_query of the row with the roughness the scene was given."""
    wo, wi, u = _directions(500, 3)
    i = [c[0] for c in CASES].index("metal_aniso")
    a = table.bsdf_query(i, wo, wi, u)
    b = oracle.bsdf_query(oracle._materials_flat(scenes._materials([CASES[i][1]]))[0], wo, wi, u, CASES[i][2])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        table.set_material_roughness(len(CASES) - 1, 0.1)  # matte
    with pytest.raises(ValueError):
        table.set_material_roughness(len(CASES), 0.1)


@pytest.mark.parametrize("which", ["plastic", "metal"])
@pytest.mark.parametrize("integrator", [0, 1, 2], ids=["path", "direct", "whitted"])
def test_point_light_closed_form(which, integrator):
    """test_gpu_glossy.py::test_point_light_closed_form on the oracle: same reference, rtol 1e-4."""
    if which == "plastic":
        row, m = scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2), mm.Material.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2)
    else:
        row, m = scenes.metal(ETA, K, 0.1), mm.Material.metal(ETA, K, 0.1)
    p_light, I = np.array([0.3, -0.2, 1.5]), np.array([2.0, 3.0, 4.0])
    scene = oracle.OracleScene(scenes.glossy_plane_point_light_scene(row, tuple(p_light), tuple(I)))
    rays = _point_light_rays()
    keys = np.arange(len(rays), dtype=np.uint64) * 7919 + 3
    rgb, _ = scene.li(rays, keys, integrator=integrator, max_depth=1, light_strategy=0)
    scene.close()
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    t = -o[:, 2] / d[:, 2]
    p = o + t[:, None] * d
    wi = p_light - p
    r2 = np.sum(wi * wi, 1)
    wi = wi / np.sqrt(r2)[:, None]
    ref = mm.bsdf_f(m, -d, wi) * I * np.abs(wi[:, 2:3]) / r2[:, None]
    assert np.all(ref > 0)
    np.testing.assert_allclose(rgb, ref, rtol=1e-4)


@pytest.mark.parametrize("which", ["plastic", "metal"])
def test_furnace_closed_form(which):
    """test_gpu_glossy.py::test_furnace_closed_form on the oracle: 4 sigma + 1e-4 of the albedo."""
    if which == "plastic":
        row, m = scenes.plastic((0.3, 0.25, 0.2), (0.5, 0.5, 0.5), 0.1), mm.Material.plastic((0.3, 0.25, 0.2), (0.5, 0.5, 0.5), 0.1)
    else:
        row, m = scenes.metal(ETA, K, 0.05), mm.Material.metal(ETA, K, 0.05)
    Le = np.array([1.0, 0.8, 0.6])
    scene = oracle.OracleScene(scenes.glossy_plane_env_scene(row, tuple(Le)))
    theta = np.radians(50.0)
    eye = (0.0, -5 * np.sin(theta), 5 * np.cos(theta))
    w = h = 64
    cam = scenes.orthographic_camera(eye, (0, 0, 0), (0, 0, 1), 1.0, w, h)
    film, _ = scene.render(scenes.camera_dict_to_floats(cam), w, h, 16, max_depth=1, seed=5)
    scene.close()
    rgb = oracle.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    wo = -_unit(np.array([0.0, 0.0, 0.0]) - np.array(eye))
    ref = Le * mm.albedo(m, wo)
    mean, se = rgb.mean(0), rgb.std(0) / np.sqrt(len(rgb))
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-4 * ref), (mean, ref, se)
