"""Plastic and metal on the device (PBRT_MAT_PLASTIC / PBRT_MAT_METAL): the BSDF pinned to the float64 model
(microfacet_model.py) through pbrt_hip_bsdf_query, a chi^2 test of its sampler, closed forms through pbrt_hip_li and a
furnace render, the films of scenes without glossy materials unchanged by the glossy kernel instantiations, shade orders and
instance overrides, and refusals that leave the scene as it was."""
import numpy as np
import pytest
from scipy import stats

import pbrt_hip
from pbrt_hip import scenes
import microfacet_model as mm
from glossy_cases import (CASES, CHI2, ETA, K, _directions, _glossy_mixed, _point_light_rays, _rel_check, _table_scene, _unit,
                          _with_glossy_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(hip_ctx):
    scene = pbrt_hip.Scene(hip_ctx, _table_scene([c[1] for c in CASES]))
    for i, c in enumerate(CASES):
        if c[2] is not None:
            scene.set_material_roughness(i, c[2][0], c[2][1], remap=c[2][2])
    yield scene
    scene.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bsdf_query_matches_model(table, i):
    m = CASES[i][3]
    wo, wi, u = _directions(20000, 100 + i)
    q = table.bsdf_query(i, wo, wi, u)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f_ref, pdf_ref = mm.bsdf_f(m, wo64, wi64), mm.bsdf_pdf(m, wo64, wi64)
    ok = (np.abs(wo64[:, 2]) >= 1e-3) & (np.abs(wi64[:, 2]) >= 1e-3) & (np.linalg.norm(wo64 + wi64, axis=1) > 1e-2)
    # 1e-4 relative; at alpha 1e-3, D of a half vector within ~0.2 rad of +z goes through the float32 1 - cos^2 theta_h of the
    # reference's formula, which alone costs ~1e-3 there: 2e-2 on those
    wh = _unit(wo64 + wi64 + 1e-30)
    rtol = np.where((min(m.ax, m.ay) < 0.01) & (1 - wh[:, 2] ** 2 < 0.05), 2e-2, 1e-4)
    _rel_check(q["f"], f_ref, np.repeat(ok[:, None], 3, 1), "f", np.repeat(rtol[:, None], 3, 1))
    _rel_check(q["pdf"], pdf_ref, ok, "pdf", rtol)
    # sample_f: the same u gives the same wi
    wi_m, f_m, pdf_m, ok_m, glossy_m = mm.bsdf_sample_f(m, wo64, u)
    ok_d = q["pdf_s"] > 0
    sel = np.abs(wo64[:, 2]) >= 1e-3
    assert np.mean(ok_d[sel] != ok_m[sel]) < 1e-3
    both = sel & ok_d & ok_m
    assert both.sum() > 0.3 * sel.sum()
    # the same direction but where float32 and float64 take different sides of one of trowbridge_reitz_sample11's branches
    # (which root of the quadratic, the tmp clamp): a few in 10^4 at most. Left out: microfacet samples whose stretched wo
    # takes the normal-incidence branch, where the rotation by its azimuth (float32 1 - cos^2 of a direction within 1e-2 of
    # +z) is arbitrary and, the slopes being isotropic there, changes nothing but which sample u gives
    ws = np.abs(wo64) * np.array([m.ax, m.ay, 1.0])
    normal_branch = glossy_m & (ws[:, 2] / np.linalg.norm(ws, axis=1) > 0.9999)
    cmp = both & ~normal_branch
    dw = np.abs(q["wi_s"][cmp] - wi_m[cmp]).max(axis=1)
    assert cmp.sum() > 0.2 * sel.sum() and np.mean(dw > 1e-3) < 1e-3, np.sort(dw)[-5:]
    flags = q["flags"][both]
    expect = np.where(glossy_m[both], pbrt_hip.BSDF_GLOSSY, pbrt_hip.BSDF_DIFFUSE) | pbrt_hip.BSDF_REFLECTION
    assert np.mean(flags == expect) > 0.999
    assert np.all(q["flags"][~ok_d] == 0)
    # pdf_s = pdf(wo, wi_s), f_s = f(wo, wi_s) on the device itself. pdf recomputes wh = normalize(wo + wi_s): at alpha 1e-3
    # the float32 1 - cos^2 theta_h of a normal that close to +z carries a relative error of ~1e-1 (the reference's arithmetic)
    # (there only the typical sample is held to it: the median relative difference)
    q2 = table.bsdf_query(i, wo[ok_d], q["wi_s"][ok_d], u[ok_d])
    if min(m.ax, m.ay) < 0.01:
        assert np.median(np.abs(q["pdf_s"][ok_d] / q2["pdf"] - 1)) < 1e-2
        assert np.median(np.abs(q["f_s"][ok_d] / np.maximum(q2["f"], 1e-30) - 1)) < 1e-2
    else:
        np.testing.assert_allclose(q["pdf_s"][ok_d], q2["pdf"], rtol=2e-3)
        np.testing.assert_allclose(q["f_s"][ok_d], q2["f"], rtol=2e-3, atol=1e-6 * np.abs(q2["f"]).max())


@pytest.mark.parametrize("name,i,theta_o", CHI2, ids=[f"{c[0]}-{c[2]:g}" for c in CHI2])
def test_sampler_chi2(table, name, i, theta_o):
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
    # Pearson chi^2 over the bins, the 'nothing sampled' bin last; bins expecting fewer than 5 pooled
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


@pytest.mark.parametrize("which", ["plastic", "metal"])
@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED])
def test_point_light_closed_form(hip_ctx, which, integrator):
    if which == "plastic":
        row, m = scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2), mm.Material.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2)
    else:
        row, m = scenes.metal(ETA, K, 0.1), mm.Material.metal(ETA, K, 0.1)
    p_light, I = np.array([0.3, -0.2, 1.5]), np.array([2.0, 3.0, 4.0])
    scene = pbrt_hip.Scene(hip_ctx, scenes.glossy_plane_point_light_scene(row, tuple(p_light), tuple(I)))
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
def test_furnace_closed_form(hip_ctx, which):
    if which == "plastic":
        row, m = scenes.plastic((0.3, 0.25, 0.2), (0.5, 0.5, 0.5), 0.1), mm.Material.plastic((0.3, 0.25, 0.2), (0.5, 0.5, 0.5), 0.1)
    else:
        row, m = scenes.metal(ETA, K, 0.05), mm.Material.metal(ETA, K, 0.05)
    Le = np.array([1.0, 0.8, 0.6])
    scene = pbrt_hip.Scene(hip_ctx, scenes.glossy_plane_env_scene(row, tuple(Le)))
    theta = np.radians(50.0)
    eye = (0.0, -5 * np.sin(theta), 5 * np.cos(theta))
    w = h = 64
    cam = scenes.orthographic_camera(eye, (0, 0, 0), (0, 0, 1), 1.0, w, h)
    film, _ = scene.render(cam, w, h, 16, max_depth=1, seed=5)
    scene.close()
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    wo = -_unit(np.array([0.0, 0.0, 0.0]) - np.array(eye))
    ref = Le * mm.albedo(m, wo)
    mean, se = rgb.mean(0), rgb.std(0) / np.sqrt(len(rgb))
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-4 * ref), (mean, ref, se)


def _render(hip_ctx, sc, integrator, shade_order, w=64, h=64, spp=4, cam=None):
    scene = pbrt_hip.Scene(hip_ctx, sc)
    cam = scenes.random_triangles_camera(w, h) if cam is None else cam
    film, st = scene.render(cam, w, h, spp, integrator=integrator, max_depth=5, seed=11, shade_order=shade_order)
    scene.close()
    return film, st


@pytest.mark.parametrize("shade_order", [0, 1, 2])
@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT])
def test_unused_glossy_rows_leave_old_films_bit_identical(hip_ctx, integrator, shade_order):
    base = scenes.mixed_materials_scene(n_tris=3000)
    f0, s0 = _render(hip_ctx, base, integrator, shade_order)
    f1, s1 = _render(hip_ctx, _with_glossy_rows(base), integrator, shade_order)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])


@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED])
def test_glossy_scene_same_film_in_every_shade_order(hip_ctx, integrator):
    sc = _glossy_mixed()
    films = [_render(hip_ctx, sc, integrator, so)[0] for so in (0, 1, 2)]
    assert all(np.array_equal(films[0].view(np.uint32), f.view(np.uint32)) for f in films[1:])
    assert np.isfinite(films[0]).all() and films[0][..., :3].mean() > 0
    # the glossy triangles matter: the same scene with them matte renders differently
    sc_m = dict(sc)
    sc_m["tri_material"] = np.where(sc["tri_material"] >= 3, 0, sc["tri_material"]).astype(np.int32)
    assert not np.array_equal(films[0], _render(hip_ctx, sc_m, integrator, 0)[0])


def test_instance_material_override_to_glossy(hip_ctx):
    sc = scenes.instanced_scene(n_base_tris=2000, n_instances=60, extent=1.5)
    sc = _with_glossy_rows(sc)
    sc["instance_material"] = (np.arange(60) % 5).astype(np.int32)
    cam = scenes.instanced_camera(64, 64, extent=1.5)
    films = [_render(hip_ctx, sc, pbrt_hip.INTEGRATOR_PATH, so, cam=cam)[0] for so in (0, 1, 2)]
    assert all(np.array_equal(films[0].view(np.uint32), f.view(np.uint32)) for f in films[1:])
    sc_m = dict(sc)
    sc_m["instance_material"] = np.where(sc["instance_material"] >= 3, 0, sc["instance_material"]).astype(np.int32)
    other = _render(hip_ctx, sc_m, pbrt_hip.INTEGRATOR_PATH, 0, cam=cam)[0]
    assert np.isfinite(films[0]).all() and not np.array_equal(films[0], other)


BAD_ROWS = [
    ((scenes.MAT_METAL, (0.0, 1.0, 1.0), K, 0.1), "eta"),
    ((scenes.MAT_METAL, (-1.0, 1.0, 1.0), K, 0.1), "eta"),
    ((scenes.MAT_METAL, (np.nan, 1.0, 1.0), K, 0.1), "eta"),
    ((scenes.MAT_METAL, ETA, (3.0, -0.1, 2.0), 0.1), "k"),
    ((scenes.MAT_METAL, ETA, (3.0, np.inf, 2.0), 0.1), "k"),
    ((scenes.MAT_PLASTIC, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), -0.1), "roughness"),
    ((scenes.MAT_PLASTIC, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), np.nan), "roughness"),
    ((scenes.MAT_METAL, ETA, K, np.inf), "roughness"),
    ((6, (0.5, 0.5, 0.5), (0, 0, 0), 1.0), "unknown material type"),
]


@pytest.mark.parametrize("row,why", BAD_ROWS)
def test_creation_refuses_bad_materials(hip_ctx, row, why):
    with pytest.raises(pbrt_hip.PbrtHipError, match=f"\\(1\\): .*{why}"):
        pbrt_hip.Scene(hip_ctx, scenes.glossy_plane_point_light_scene(row))


def test_roughness_refusals_leave_the_scene_unchanged(hip_ctx):
    rows = [scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2), scenes.metal(ETA, K, 0.1),
            (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)]
    sc = _table_scene(rows)
    sc["tri_material"] = np.array([0, 1], np.int32)
    scene = pbrt_hip.Scene(hip_ctx, sc)
    rays = _point_light_rays(4)
    keys = np.arange(len(rays), dtype=np.uint64)
    before, _ = scene.li(rays, keys, max_depth=1)
    cases = [(3, 0.1, 0.1, True, "out of range"), (-1, 0.1, 0.1, True, "out of range"), (2, 0.1, 0.1, True, "not PBRT_MAT_PLASTIC"),
             (0, 0.1, 0.2, True, "isotropic"), (1, -0.1, 0.1, True, "finite"), (1, 0.1, np.nan, True, "finite"),
             (0, np.inf, np.inf, False, "finite"), (1, 0.0, 0.1, False, "without remapping"), (0, 0.0, 0.0, False, "without remapping")]
    for m, u, v, remap, why in cases:
        with pytest.raises(pbrt_hip.PbrtHipError, match=f"\\(1\\): .*{why}"):
            scene.set_material_roughness(m, u, v, remap=remap)
    after, _ = scene.li(rays, keys, max_depth=1)
    assert np.array_equal(before, after)
    scene.set_material_roughness(1, 0.1, 0.3)  # accepted: the anisotropic metal is another BSDF
    changed, _ = scene.li(rays, keys, max_depth=1)
    assert not np.array_equal(before, changed)
    scene.close()
