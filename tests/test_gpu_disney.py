"""The Disney material on the device (pbrt_hip_scene_set_disney_material), test for test as test_gpu_bxdfs.py: the BSDF pinned to
the float64 model (disney_model.py) through pbrt_hip_bsdf_query, a chi^2 test of its sampler, closed forms through pbrt_hip_li
with eye and light on either side of the surface, furnace renders from above and below, glossy transmission not being a
specular bounce, the films of scenes without a Disney row unchanged by the level-3 kernel instantiations, shade orders and
instance overrides, ordinary descriptors over a Disney row, and refusals that leave the scene as it was."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import disney_model as dm
from bxdf_cases import KR, KT
from disney_cases import (ACCEPTED, BAND_MAX_SHARE, C, CASES, CHI2_DESC, CHI2_FIT, CHI2_MODEL, FURNACE, N_FIT, REFUSED, chi2_wo, directions,
                          furnace_reference, furnace_wo, in_band)
from glossy_cases import _glossy_mixed, _point_light_rays, _rel_check, _unit

pytestmark = pytest.mark.gpu
MATTE = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)


def _disney_scene(sc, descs):
    """sc with one matte row appended per descriptor, made a Disney row after creation; returns (scene, first new row)"""
    sc = dict(sc)
    first = len(sc["materials"])
    sc["materials"] = np.concatenate([sc["materials"], scenes._materials([MATTE] * len(descs))])
    sc["disney_descs"] = {first + k: d for k, d in enumerate(descs)}
    return sc, first


@pytest.fixture(scope="module")
def table(hip_ctx):
    sc = scenes.glossy_plane_point_light_scene(MATTE)
    sc["materials"] = scenes._materials([MATTE] * len(CASES))
    sc["disney_descs"] = {i: c[1] for i, c in enumerate(CASES)}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    yield scene
    scene.close()


def _restatement_error(m, wo, wi, mask):
    """largest relative error of the model evaluated in float32 (its constants rounded as the device holds them) against
    float64 over `mask`: (f, pdf)"""
    m32 = m.as32()
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    out = []
    for fn in (lambda a, b: dm.bsdf_f(m32, a, b)[:, 1], lambda a, b: dm.bsdf_pdf(m32, a, b)):
        lo, hi = fn(wo, wi)[mask].astype(np.float64), fn(wo64, wi64)[mask]
        nz = hi != 0
        out.append(float(np.max(np.abs(lo[nz] - hi[nz]) / np.abs(hi[nz]))) if nz.any() else 0.0)
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bsdf_query_matches_model(table, i):
    """test_gpu_bxdfs.py::test_bsdf_query_matches_model's rules: 1e-4 relative on the same side of the surface; across it,
    outside the grazing band, max(1e-4, 4 x the float32 restatement of the model on this table). The clearcoat at gloss 1
    (g = 0.001) does not need the restatement rule on the same side: its restatement error is printed (7.7e-6 for f, 4.0e-7 for
    the pdf; the device: 8.1e-6 and 4.0e-7). Measured over the 17 cases: f 6.7e-7 .. 3.6e-5, pdf 4.0e-7 .. 3.6e-6."""
    m = CASES[i][2]
    wo, wi, u = directions(m, 3000, 300 + i)
    q = table.bsdf_query(i, wo, wi, u)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f_ref, pdf_ref = dm.bsdf_f(m, wo64, wi64), dm.bsdf_pdf(m, wo64, wi64)
    ok = (np.abs(wo64[:, 2]) >= 1e-3) & (np.abs(wi64[:, 2]) >= 1e-3) & (np.linalg.norm(wo64 + wi64, axis=1) > 1e-2)
    across = wo64[:, 2] * wi64[:, 2] < 0
    band = in_band(m, wo64, wi64)
    assert band.mean() <= BAND_MAX_SHARE
    e_f, e_pdf = _restatement_error(m, wo, wi, ok & across & ~band)
    print(f"{CASES[i][0]}: band {band.mean():.3f}, float32 restatement across the surface f {e_f:.3g} pdf {e_pdf:.3g}")
    if "clearcoat" in m.lobes and m.a2 < 1e-5:
        s_f, s_pdf = _restatement_error(m, wo, wi, ok & ~across)
        print(f"  clearcoat at g = {np.sqrt(m.a2):.3g}: float32 restatement on the same side f {s_f:.3g} pdf {s_pdf:.3g}")
    rtol_f = np.where(across, max(1e-4, 4 * e_f), 1e-4)
    rtol_pdf = np.where(across, max(1e-4, 4 * e_pdf), 1e-4)
    out = ok & ~band
    for what, dev, ref in (("f", q["f"], f_ref), ("pdf", q["pdf"][:, None], pdf_ref[:, None])):
        nz = out[:, None] & (ref != 0)
        err = np.abs(dev - ref)[nz] / np.abs(ref[nz])
        print(f"  {what}: worst relative error {err.max() if err.size else 0:.3g} over {nz.sum()} values")
    _rel_check(q["f"], f_ref, np.repeat(out[:, None], 3, 1), "f", np.repeat(rtol_f[:, None], 3, 1))
    _rel_check(q["pdf"], pdf_ref, out, "pdf", rtol_pdf)
    inb = ok & band
    if inb.any():
        assert np.abs(q["f"][inb] - f_ref[inb]).max() <= 1e-4 * f_ref[ok].max()
        assert np.abs(q["pdf"][inb] - pdf_ref[inb]).max() <= 1e-4 * pdf_ref[ok].max()
    # wo.z == 0: zeros are zeros
    assert np.all(q["f"][wo[:, 2] == 0] == 0) and np.all(q["pdf"][wo[:, 2] == 0] == 0)

    # sample_f: the same u gives the same lobe and the same wi
    wi_m, f_m, pdf_m, ok_m, flags_m, comp = dm.bsdf_sample_f(m, wo64, u)
    ok_d = q["pdf_s"] > 0
    sel = np.abs(wo64[:, 2]) >= 1e-3
    print(f"  sampled: device {ok_d[sel].mean():.4f} model {ok_m[sel].mean():.4f} differ {np.mean(ok_d[sel] != ok_m[sel]):.2g}")
    assert np.mean(ok_d[sel] != ok_m[sel]) < 1e-3
    both = sel & ok_d & ok_m
    assert both.sum() > 0.3 * sel.sum()
    assert np.array_equal(q["flags"][both], flags_m[both])
    assert np.all(q["flags"][~ok_d] == 0) and np.all(q["wi_s"][~ok_d] == 0) and np.all(q["f_s"][~ok_d] == 0)
    # (left out as in test_gpu_glossy.py: the normal-incidence branch of trowbridge_reitz_sample11, whose rotation is arbitrary;
    # the reflection lobe samples with (ax, ay), the transmission lobe with its own alphas)
    lobe = np.array(m.lobes)[comp]
    normal_branch = np.zeros(len(wo), bool)
    for name, (ax, ay) in (("micro", (m.ax, m.ay)), ("trans", (m.tax, m.tay))):
        ws = np.abs(wo64) * np.array([ax, ay, 1.0])
        normal_branch |= (lobe == name) & (ws[:, 2] / np.linalg.norm(ws, axis=1) > 0.9999)
    cmp = both & ~normal_branch
    dw = np.abs(q["wi_s"][cmp] - wi_m[cmp]).max(axis=1)
    print(f"  wi_s: {cmp.sum()} compared, {np.mean(dw > 1e-3):.2g} beyond 1e-3, worst {np.sort(dw)[-3:]}")
    assert cmp.sum() > 0.2 * sel.sum() and np.mean(dw > 1e-3) < 1e-3, np.sort(dw)[-5:]
    # f_s = f(wo, wi_s) and pdf_s = pdf(wo, wi_s) on the device itself, and both against the model at the device's own wi_s:
    # test_gpu_bxdfs.py's 2e-3, plus what rounding wi_s to float32 does to a narrow lobe. The sampler's pdf_s belongs to the half
    # vector it drew; wi_s comes out of it through three float32 operations per component (<= 1.8e-7), the half vector rebuilt
    # from wo + wi_s is off by that over its length 2 |wo.wh| (about 2 |cos theta_o| where a narrow lobe has its mass), which is
    # a relative change of the slope of that over the lobe's width w (the smallest alpha, or the clearcoat's g), and D changes by
    # at most twice the slope's relative change (4 s / (1 + s^2) <= 2): 1.8e-7 / (w |cos theta_o|). At w >= 0.06 that is
    # nothing beside 2e-3 away from grazing wo; at w = 1e-3 (roughness 0, gloss 1) it is 3.6e-3 at |cos theta_o| = 0.05.
    w_min = min([m.ax, m.ay] + ([m.tax, m.tay] if "trans" in m.lobes else []) + ([np.sqrt(m.a2)] if "clearcoat" in m.lobes else []))
    round_tol = 1.8e-7 / (w_min * np.abs(wo64[:, 2]).clip(1e-3))

    def close(dev, ref, rtol, atol, what):
        err = np.abs(dev - ref) - (rtol * np.abs(ref) + atol)
        assert np.all(err <= 0), f"{what}: {np.sum(err > 0)} of {err.size} beyond, worst {np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-30)):.3g}"

    q2 = table.bsdf_query(i, wo[ok_d], q["wi_s"][ok_d], u[ok_d])
    close(q["pdf_s"][ok_d], q2["pdf"], 2e-3 + round_tol[ok_d], 0.0, "pdf_s against pdf(wo, wi_s)")
    close(q["f_s"][ok_d], q2["f"], 2e-3, 1e-6 * np.abs(q2["f"]).max(), "f_s against f(wo, wi_s)")  # (f_s is evaluated at wi_s itself)
    wis = q["wi_s"][both].astype(np.float64)
    clear = ~in_band(m, wo64[both], wis) & (np.abs(wis[:, 2]) >= 1e-3)
    tol = (max(2e-3, 4 * e_f) + round_tol[both])[clear]
    close(q["pdf_s"][both][clear], dm.bsdf_pdf(m, wo64[both], wis)[clear], tol, 0.0, "pdf_s against the model")
    fm = dm.bsdf_f(m, wo64[both], wis)[clear]
    close(q["f_s"][both][clear], fm, max(2e-3, 4 * e_f), 1e-6 * np.abs(fm).max(), "f_s against the model")


@pytest.fixture(scope="module")
def chi2_table(hip_ctx):
    names = sorted(CHI2_DESC)
    sc = scenes.glossy_plane_point_light_scene(MATTE)
    sc["materials"] = scenes._materials([MATTE] * len(names))
    sc["disney_descs"] = {k: CHI2_DESC[n] for k, n in enumerate(names)}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    yield scene, names
    scene.close()


@pytest.mark.parametrize("name,theta_o", CHI2_FIT, ids=[f"{c[0]}-{c[1]:g}" for c in CHI2_FIT])
def test_sampler_chi2(chi2_table, name, theta_o):
    """test_gpu_bxdfs.py::test_sampler_chi2's construction, 10^6 samples; disney_cases.CHI2_FIT says which case is left out and why"""
    scene, names = chi2_table
    n = N_FIT
    wo = chi2_wo(theta_o).astype(np.float32)
    u = np.random.default_rng(7).random((n, 2)).astype(np.float32)
    wo32 = np.broadcast_to(wo, (n, 3)).copy()
    q = scene.bsdf_query(names.index(name), wo32, wo32, u)
    ok = q["pdf_s"] > 0
    p, chi2, bins, stray = dm.chi2_p(CHI2_MODEL[name], wo.astype(np.float64), q["wi_s"], ok, n)
    print(f"{name} {theta_o}: chi2 {chi2:.5g} over {bins} bins, p {p:.3g}, nothing sampled {1 - ok.mean():.4f}")
    assert stray == 0, "samples where the pdf has no mass"
    assert p > 1e-3, (chi2, bins, p)


# ---- point light: Li = f(wo, wi) I |cos theta_i| / r^2 ----
# (isotropic rows: the plane's two triangles do not share dpdu; anisotropy is held by test_bsdf_query_matches_model)
POINT = {"opaque": scenes.disney(C, roughness=0.5, sheen=0.5, clearcoat=1.0, clearcoat_gloss=0.0),
         "trans": scenes.disney(C, spec_trans=0.7, roughness=0.5),
         "thin": scenes.disney(C, thin=True, flatness=0.5, diff_trans=1.0, spec_trans=0.5, roughness=0.5)}
# (material, eye side, light side)
POINT_CASES = [("opaque", 1, 1), ("opaque", -1, -1)] + [(w, e, l) for w in ("trans", "thin") for e in (1, -1) for l in (1, -1)]


@pytest.mark.parametrize("which,eye,light", POINT_CASES, ids=[f"{c[0]}-eye{c[1]:+d}-light{c[2]:+d}" for c in POINT_CASES])
@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED])
def test_point_light_closed_form(hip_ctx, which, eye, light, integrator):
    desc = POINT[which]
    m = dm.Disney(desc)
    p_light, I = np.array([0.3, -0.2, 1.5 * light]), np.array([2.0, 3.0, 4.0])
    sc = scenes.glossy_plane_point_light_scene(MATTE, tuple(p_light), tuple(I))
    sc["disney_descs"] = {0: desc}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    # test_gpu_bxdfs.py's ray table: a 6 x 6 grid of plane points seen from one eye; across the surface a tighter grid, and the
    # pairs in the grazing band or without light are left out, decided on the model before anything is rendered
    rays = _point_light_rays()
    if eye * light < 0:
        xs = np.linspace(-0.6, 0.6, 6)
        pts = np.array([(x, y, 0.0) for x in xs for y in xs])
        rays["d"] = _unit(pts - rays["o"][0].astype(np.float64)).astype(np.float32)
    if eye < 0:
        rays["o"][:, 2] *= -1
        rays["d"][:, 2] *= -1

    def reference(rays):
        o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
        t = -o[:, 2] / d[:, 2]
        p = o + t[:, None] * d
        wi = p_light - p
        r2 = np.sum(wi * wi, 1)
        wi = wi / np.sqrt(r2)[:, None]
        return dm.bsdf_f(m, -d, wi) * I * np.abs(wi[:, 2:3]) / r2[:, None], in_band(m, -d, wi)

    ref, band = reference(rays)
    rays = rays[~band & np.all(ref > 0, axis=1)]
    assert len(rays) >= 30
    ref, band = reference(rays)
    assert not band.any() and np.all(ref > 0)
    keys = np.arange(len(rays), dtype=np.uint64) * 7919 + 3
    rgb, _ = scene.li(rays, keys, integrator=integrator, max_depth=1, light_strategy=0)
    scene.close()
    print(f"worst relative difference {np.max(np.abs(rgb / ref - 1)):.3g}")
    np.testing.assert_allclose(rgb, ref, rtol=1e-4)


# ---- furnace: Le albedo(wo), from above and from below ----
@pytest.mark.parametrize("k", range(len(FURNACE)), ids=[c[0] for c in FURNACE])
def test_furnace_closed_form(hip_ctx, k):
    _, desc, m, below = FURNACE[k]
    Le = np.array([1.0, 0.8, 0.6])
    sc = scenes.glossy_plane_env_scene(MATTE, tuple(Le))
    sc["disney_descs"] = {0: desc}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    wo = furnace_wo(below)
    w = h = 64
    cam = scenes.orthographic_camera(tuple(5 * wo), (0, 0, 0), (0, 0, 1), 1.0, w, h)
    film, _ = scene.render(cam, w, h, 16, max_depth=1, seed=5)
    scene.close()
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    albedo, err = furnace_reference(m, wo)
    ref = Le * albedo
    mean, se = rgb.mean(0), rgb.std(0) / np.sqrt(len(rgb))
    print(f"mean {mean} ref {ref} se {se} quadrature error {Le * err}")
    assert np.all(Le * err < se / 4), (err, se)  # the reference's own error (a doubled quadrature grid) against the render's
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-4 * ref), (mean, ref, se)


# ---- glossy transmission through a Disney row is not a specular bounce ----
def test_glossy_transmission_is_not_a_specular_bounce(hip_ctx):
    """test_gpu_bxdfs.py's construction: the plane of a transmissive Disney row over a two-sided emitter that fills the lower
    hemisphere, max_depth 2. The emitter is counted once, by next-event estimation at the Disney hit; the path that goes on
    through the glossy lobe and hits it does not add Le again (path.rs:80)."""
    Le = np.array([1.0, 0.8, 0.6])
    desc = scenes.disney(C, spec_trans=0.7, roughness=0.5)
    pos, idx = scenes._plane_z0(1e3)
    low = pos.copy()
    low[:, 2] = -1.0
    sc = dict(positions=np.concatenate([pos, low]), indices=np.concatenate([idx, idx + 4]), tri_material=np.array([0, 0, 1, 1], np.int32),
              materials=scenes._materials([MATTE, (scenes.MAT_MATTE, (0, 0, 0), (0, 0, 0), 1.0)]), tri_light=np.array([-1, -1, 0, 1], np.int32),
              lights=scenes._lights([(scenes.LIGHT_DIFFUSE_AREA, tuple(Le), 2, 1, 1), (scenes.LIGHT_DIFFUSE_AREA, tuple(Le), 3, 1, 1)]))
    sc["disney_descs"] = {0: desc}
    wo = furnace_wo(False)
    w = h = 64
    cam = scenes.orthographic_camera(tuple(5 * wo), (0, 0, 0), (0, 0, 1), 1.0, w, h)
    scene = pbrt_hip.Scene(hip_ctx, sc)
    film, _ = scene.render(cam, w, h, 16, max_depth=2, seed=9)
    scene.close()
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    mean, se = rgb.mean(0), rgb.std(0) / np.sqrt(len(rgb))
    nee_only = Le * dm.albedo_parts(dm.Disney(desc), wo)[1]  # what crosses the surface; nothing lights the upper side
    print(f"mean {mean} se {se} NEE only {nee_only} NEE + emission {2 * nee_only}")
    assert np.all(np.abs(mean - nee_only) < 4 * se + 1e-4 * nee_only)
    assert np.all(np.abs(mean - 2 * nee_only) > 4 * se)


# ---- old films unchanged ----
def _render(hip_ctx, sc, integrator, shade_order, w=64, h=64, spp=4, cam=None):
    scene = pbrt_hip.Scene(hip_ctx, sc)
    cam = scenes.random_triangles_camera(w, h) if cam is None else cam
    film, st = scene.render(cam, w, h, spp, integrator=integrator, max_depth=5, seed=11, shade_order=shade_order)
    scene.close()
    return film, st


LEVEL2_ROWS = [scenes.rough_glass(KR, KT, 1.5, 0.2, remap=False), scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.1, 0.3),
               scenes.matte_sigma((0.6, 0.5, 0.4), 40.0)]
DISNEY_ROWS = [CASES[k][1] for k in (0, 5, 8, 16)]  # defaults, clearcoat, spec_trans 0.7, everything (thin)


def _level2_mixed():
    """test_gpu_bxdfs.py's mixed scene: matte, mirror, glass, rough glass, substrate, Oren-Nayar"""
    sc = dict(scenes.mixed_materials_scene(n_tris=3000))
    first = len(sc["materials"])
    sc["materials"] = np.concatenate([sc["materials"], scenes._materials([MATTE] * 3)])
    sc["material_descs"] = {first + k: d for k, d in enumerate(LEVEL2_ROWS)}
    tm = sc["tri_material"].copy()
    tm[:3000] = np.arange(3000) % 6
    sc["tri_material"] = tm
    return sc


@pytest.mark.parametrize("shade_order", [0, 1, 2])
@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT])
@pytest.mark.parametrize("base", ["mixed", "glossy_mixed", "level2_mixed"])
def test_unused_disney_row_leaves_old_films_bit_identical(hip_ctx, base, integrator, shade_order):
    """a Disney row no triangle uses selects the level-3 kernels: the rows of levels 0, 1 and 2 render what they rendered"""
    sc = {"mixed": lambda: scenes.mixed_materials_scene(n_tris=3000), "glossy_mixed": _glossy_mixed, "level2_mixed": _level2_mixed}[base]()
    f0, s0 = _render(hip_ctx, sc, integrator, shade_order)
    f1, s1 = _render(hip_ctx, _disney_scene(sc, DISNEY_ROWS[:1])[0], integrator, shade_order)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])


# ---- a mixed scene with Disney rows ----
def _disney_mixed():
    sc, first = _disney_scene(scenes.mixed_materials_scene(n_tris=3000), DISNEY_ROWS)
    tm = sc["tri_material"].copy()
    tm[:3000] = np.arange(3000) % (3 + len(DISNEY_ROWS))  # matte, mirror, glass, four Disney rows
    sc["tri_material"] = tm
    return sc, first


@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED])
def test_mixed_scene_same_film_in_every_shade_order(hip_ctx, integrator):
    sc, first = _disney_mixed()
    films = [_render(hip_ctx, sc, integrator, so)[0] for so in (0, 1, 2)]
    assert all(np.array_equal(films[0].view(np.uint32), f.view(np.uint32)) for f in films[1:])
    assert np.isfinite(films[0]).all() and films[0][..., :3].mean() > 0
    sc_m = dict(sc)  # the Disney rows matter: the same scene with them matte renders differently
    sc_m.pop("disney_descs")
    assert not np.array_equal(films[0], _render(hip_ctx, sc_m, integrator, 0)[0])


def test_instance_material_override_to_disney_rows(hip_ctx):
    sc, first = _disney_scene(scenes.instanced_scene(n_base_tris=2000, n_instances=60, extent=1.5), DISNEY_ROWS)
    sc["instance_material"] = (np.arange(60) % (3 + len(DISNEY_ROWS))).astype(np.int32)
    cam = scenes.instanced_camera(64, 64, extent=1.5)
    films = [_render(hip_ctx, sc, pbrt_hip.INTEGRATOR_PATH, so, cam=cam)[0] for so in (0, 1, 2)]
    assert all(np.array_equal(films[0].view(np.uint32), f.view(np.uint32)) for f in films[1:])
    sc_m = dict(sc)
    sc_m.pop("disney_descs")
    other = _render(hip_ctx, sc_m, pbrt_hip.INTEGRATOR_PATH, 0, cam=cam)[0]
    assert np.isfinite(films[0]).all() and films[0][..., :3].mean() > 0 and not np.array_equal(films[0], other)


@pytest.mark.parametrize("integrator", [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED])
def test_ordinary_descriptor_over_a_disney_row(hip_ctx, integrator):
    """pbrt_hip_scene_set_material turns a Disney row back into an ordinary one: the film of the scene that never had the
    Disney row, bit for bit, for a level-0 row (matte with sigma 0) and a level-2 row (substrate)"""
    cam = scenes.random_triangles_camera(64, 64)
    for desc in (scenes.matte_sigma((0.6, 0.5, 0.4), 0.0), LEVEL2_ROWS[1]):
        sc = dict(scenes.mixed_materials_scene(n_tris=3000))
        sc["material_descs"] = {0: desc}
        want, s0 = _render(hip_ctx, sc, integrator, 0)
        scene = pbrt_hip.Scene(hip_ctx, sc)
        scene.set_disney_material(0, DISNEY_ROWS[3])
        as_disney, _ = scene.render(cam, 64, 64, 4, integrator=integrator, max_depth=5, seed=11, shade_order=0)
        scene.set_material(0, desc)
        got, s1 = scene.render(cam, 64, 64, 4, integrator=integrator, max_depth=5, seed=11, shade_order=0)
        scene.close()
        assert not np.array_equal(as_disney, want)
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
        assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])


# ---- refusals ----
def test_refusals_leave_the_scene_unchanged(hip_ctx):
    sc = scenes.glossy_plane_point_light_scene(MATTE)
    sc["materials"] = scenes._materials([MATTE, MATTE])
    sc["disney_descs"] = {0: CASES[5][1]}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    rays = _point_light_rays(4)
    keys = np.arange(len(rays), dtype=np.uint64)
    before, _ = scene.li(rays, keys, max_depth=1)
    for row, desc, why in REFUSED:
        with pytest.raises(pbrt_hip.PbrtHipError, match=f"\\(1\\): pbrt_hip_scene_set_disney_material: .*{why}"):
            scene.set_disney_material(row, desc)
        if 0 <= row < 2:
            assert scenes.disney_invalid(desc) is not None
    after, _ = scene.li(rays, keys, max_depth=1)
    assert np.array_equal(before, after)
    seen = [before]
    for desc in ACCEPTED:  # accepted, and each another BSDF
        assert scenes.disney_invalid(desc) is None
        scene.set_disney_material(0, desc)
        now, _ = scene.li(rays, keys, max_depth=1)
        assert np.isfinite(now).all() and now.mean() > 0
        assert all(not np.array_equal(now, s) for s in seen)
        seen.append(now)
    with pytest.raises(pbrt_hip.PbrtHipError, match="not PBRT_MAT_PLASTIC"):
        scene.set_material_roughness(0, 0.1)  # the roughness setter stays with plastic and metal
    scene.close()
