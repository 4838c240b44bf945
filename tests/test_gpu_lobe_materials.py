"""Uber, translucent and mix materials on the device (pbrt_hip_scene_set_lobe_material; csrc/wf_lobes.h), as test_gpu_disney.py
holds the Disney rows: the lobe-list BSDF pinned to the float64 model (lobe_model.py) through pbrt_hip_bsdf_query, specular picks
included; a chi^2 test of its sampler; closed forms through pbrt_hip_li with eye and light on either side; furnace renders; an
exact pass-through that pins the specular-bounce flag and the specular branches; the matte row's film from a one-lobe list; the
films of scenes without a used lobe row unchanged by the lobe-list kernels; a mix keeping its operands' lists; replacement in
both directions; instance overrides; refusals that leave the scene as it was."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import lobe_model as lm
import microfacet_model as mm
from lobe_cases import (ACCEPTED, BAND_MAX_SHARE, CASES, FURNACE, KD, MATTE, REFUSED, chi2_wo, directions, furnace_reference, furnace_wo, in_band,
                        install, refusal_scene)
from glossy_cases import _glossy_mixed, _point_light_rays, _rel_check, _unit

pytestmark = pytest.mark.gpu
PATH, DIRECT, WHITTED = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED
INTEGRATORS = [PATH, DIRECT, WHITTED]


def _single(fn_s, fn_m, **kw):
    return dict(name="case", operands=[], desc=lambda rows: fn_s(**kw), model=fn_m(**kw))


def _scene_with(hip_ctx, base, case):
    """the scene `base` with its row 0 made the case's lobe row (operand rows appended)"""
    sc, rows = install(base, [case])
    # row 0 is what the geometry names: set it from the installed row's descriptor with the operands' new indices
    sc["lobe_descs"][0] = sc["lobe_descs"].pop(rows[0])
    return pbrt_hip.Scene(hip_ctx, sc)


@pytest.fixture(scope="module")
def table(hip_ctx):
    sc, rows = install(scenes.glossy_plane_point_light_scene(MATTE), CASES)
    scene = pbrt_hip.Scene(hip_ctx, sc)
    yield scene, rows
    scene.close()


def _restatement_error(m, wo, wi, mask):
    """largest relative error of the model evaluated in float32 (its constants rounded as the device holds them) against
    float64 over `mask`: (f, pdf)"""
    m32 = m.as32()
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    out = []
    for fn in (lambda a, b: lm.bsdf_f(m32, a, b)[:, 1], lambda a, b: lm.bsdf_pdf(m32, a, b)):
        lo, hi = fn(wo, wi)[mask].astype(np.float64), fn(wo64, wi64)[mask]
        nz = hi != 0
        out.append(float(np.max(np.abs(lo[nz] - hi[nz]) / np.abs(hi[nz]))) if nz.any() else 0.0)
    return out


def _specular_restatement_error(m, wo):
    """largest relative error of the specular lobes' sampled f in float32 (constants rounded as the device holds them) against
    float64, over the directions wo (float32)"""
    worst = 0.0
    for l, l32 in zip(m.lobes, m.as32().lobes):
        if not l.type & lm.SPECULAR:
            continue
        _, hi, p_hi = lm.specular_sample(l, wo.astype(np.float64))
        _, lo, p_lo = lm.specular_sample(l32, wo)
        nz = (p_hi != 0) & (p_lo != 0) & np.all(hi != 0, axis=1)
        if nz.any():
            worst = max(worst, float(np.max(np.abs(lo[nz].astype(np.float64) - hi[nz]) / np.abs(hi[nz]))))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_bsdf_query_matches_model(table, i):
    """test_gpu_disney.py::test_bsdf_query_matches_model's rules and tolerances: 1e-4 relative on the same side of the surface;
    across it, outside the grazing band, max(1e-4, 4 x the float32 restatement of the model on this table). New here: the same u
    picks the same lobe as the model, specular ones included; a specular pick carries bit 16, the mirror or refracted direction and
    the lobe's pdf over the number of lobes."""
    scene, rows = table
    m = CASES[i]["model"]
    wo, wi, u = directions(m, 3000, 300 + i)
    q = scene.bsdf_query(rows[i], wo, wi, u)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f_ref, pdf_ref = lm.bsdf_f(m, wo64, wi64), lm.bsdf_pdf(m, wo64, wi64)
    ok = (np.abs(wo64[:, 2]) >= 1e-3) & (np.abs(wi64[:, 2]) >= 1e-3) & (np.linalg.norm(wo64 + wi64, axis=1) > 1e-2)
    across = wo64[:, 2] * wi64[:, 2] < 0
    band = in_band(m, wo64, wi64)
    assert band.mean() <= BAND_MAX_SHARE
    e_f, e_pdf = _restatement_error(m, wo, wi, ok & across & ~band)
    print(f"{CASES[i]['name']}: band {band.mean():.3f}, float32 restatement across the surface f {e_f:.3g} pdf {e_pdf:.3g}")
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
    assert np.all(q["f"][wo[:, 2] == 0] == 0) and np.all(q["pdf"][wo[:, 2] == 0] == 0)

    # sample_f: the same u gives the same lobe (its BxDFType), specular ones included, and the same wi
    wi_m, f_m, pdf_m, ok_m, flags_m, index = lm.bsdf_sample_f(m, wo64, u)
    ok_d = q["pdf_s"] > 0
    sel = np.abs(wo64[:, 2]) >= 1e-3
    print(f"  sampled: device {ok_d[sel].mean():.4f} model {ok_m[sel].mean():.4f} differ {np.mean(ok_d[sel] != ok_m[sel]):.2g}")
    assert np.mean(ok_d[sel] != ok_m[sel]) < 1e-3
    both = sel & ok_d & ok_m
    if m.n == 0:
        assert not ok_d.any()
        return
    assert both.sum() > 0.3 * sel.sum()
    assert np.array_equal(q["flags"][both], flags_m[both])
    assert np.all(q["flags"][~ok_d] == 0) and np.all(q["wi_s"][~ok_d] == 0) and np.all(q["f_s"][~ok_d] == 0)
    spec = both & ((flags_m & lm.SPECULAR) != 0)
    print(f"  specular picks: {spec.sum()} of {both.sum()}")
    if any(l.type & lm.SPECULAR for l in m.lobes):
        assert spec.sum() > 0
        assert np.all((q["flags"][spec] & 16) != 0)
        # the mirror or the refracted direction. refract() takes cos theta_t = sqrt(1 - sin^2 theta_t): sin^2 theta_t comes out of
        # four float32 operations on values <= 1 (4 ulp of 1 = 4.8e-7), the square root halves that and divides by cos theta_t,
        # so wi_s.z is off by up to 2.4e-7 / |cos theta_t| near grazing; 2e-6 covers the three components' own rounding
        cos_t = np.abs(wi_m[spec][:, 2:3])
        assert np.all(np.abs(q["wi_s"][spec] - wi_m[spec]) <= 2e-6 + 5e-7 / cos_t)
        np.testing.assert_allclose(q["pdf_s"][spec], 1.0 / m.n, rtol=1e-6)          # the lobe's pdf (1) over the number of lobes
        # f_s = R F / |cos| or T (1 - F) eta^2 / |cos|, held by the rule of the values across the surface: max(1e-4, 4 x the
        # float32 restatement of the model's specular lobes on this table). Near grazing wo, 1 - F is a difference of numbers
        # near 1 and cos theta_t carries the error above: the restatement says how much of f_s float32 leaves there.
        e_s = _specular_restatement_error(m, wo[sel])
        err = np.abs(q["f_s"][spec] - f_m[spec])
        tol = max(1e-4, 4 * e_s) * np.abs(f_m[spec]) + 1e-6 * np.abs(f_m[spec]).max()
        print(f"  specular f_s: float32 restatement {e_s:.3g}, worst relative error {np.max(err / np.maximum(np.abs(f_m[spec]), 1e-30)):.3g}, "
              f"worst error over its bound {np.max(err / tol):.3g}")
        assert np.all(err <= tol)
    # non-specular picks, as test_gpu_disney.py: the normal-incidence branch of trowbridge_reitz_sample11 is left out
    normal_branch = np.zeros(len(wo), bool)
    for k, l in enumerate(m.lobes):
        if l.kind in (lm.MICRO_R, lm.MICRO_T, lm.BLEND):
            ws = np.abs(wo64) * np.array([l.ax, l.ay, 1.0])
            normal_branch |= (index == k) & (ws[:, 2] / np.linalg.norm(ws, axis=1) > 0.9999)
    cmp = both & ~spec & ~normal_branch
    if cmp.any():
        dw = np.abs(q["wi_s"][cmp] - wi_m[cmp]).max(axis=1)
        print(f"  wi_s: {cmp.sum()} compared, {np.mean(dw > 1e-3):.2g} beyond 1e-3, worst {np.sort(dw)[-3:]}")
        assert np.mean(dw > 1e-3) < 1e-3, np.sort(dw)[-5:]
    w_all = [a for l in m.lobes if l.kind in (lm.MICRO_R, lm.MICRO_T, lm.BLEND) for a in (l.ax, l.ay)]
    round_tol = 1.8e-7 / (min(w_all) * np.abs(wo64[:, 2]).clip(1e-3)) if w_all else np.zeros(len(wo))

    def close(dev, ref, rtol, atol, what):
        err = np.abs(dev - ref) - (rtol * np.abs(ref) + atol)
        assert np.all(err <= 0), f"{what}: {np.sum(err > 0)} of {err.size} beyond, worst {np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-30)):.3g}"

    ns_d = ok_d & ((q["flags"] & 16) == 0)
    if ns_d.any():
        q2 = scene.bsdf_query(rows[i], wo[ns_d], q["wi_s"][ns_d], u[ns_d])
        close(q["pdf_s"][ns_d], q2["pdf"], 2e-3 + round_tol[ns_d], 0.0, "pdf_s against pdf(wo, wi_s)")
        close(q["f_s"][ns_d], q2["f"], 2e-3, 1e-6 * np.abs(q2["f"]).max(), "f_s against f(wo, wi_s)")
    nb = both & ~spec
    if nb.any():
        wis = q["wi_s"][nb].astype(np.float64)
        clear = ~in_band(m, wo64[nb], wis) & (np.abs(wis[:, 2]) >= 1e-3)
        tol = (max(2e-3, 4 * e_f) + round_tol[nb])[clear]
        close(q["pdf_s"][nb][clear], lm.bsdf_pdf(m, wo64[nb], wis)[clear], tol, 0.0, "pdf_s against the model")
        fm = lm.bsdf_f(m, wo64[nb], wis)[clear]
        close(q["f_s"][nb][clear], fm, max(2e-3, 4 * e_f), 1e-6 * np.abs(fm).max(), "f_s against the model")


# ---- chi^2 of the sampler: specular picks taken out, their share compared with the model's ----
CHI2 = [("uber_kd_ks", _single(scenes.uber, lm.uber, kd=KD, ks=0.5, kr=0.3, u_roughness=0.4, v_roughness=0.4, remap=False), 35.0),
        ("translucent_above", _single(scenes.translucent, lm.translucent, kd=KD, ks=0.5, roughness=0.5, remap=False), 40.0),
        ("translucent_below", _single(scenes.translucent, lm.translucent, kd=KD, ks=0.5, roughness=0.5, remap=False), 140.0),
        ("mix", CASES[[c["name"] for c in CASES].index("mix_plastic_uber")], 50.0)]
N_CHI2 = 1_000_000


@pytest.mark.parametrize("k", range(len(CHI2)), ids=[c[0] for c in CHI2])
def test_sampler_chi2(hip_ctx, k):
    """test_gpu_bxdfs.py::test_sampler_chi2's construction (16 x 32 bins of (cos theta, phi), the 'nothing sampled' bin last, bins
    expecting fewer than 5 pooled, p > 1e-3) over the non-specular picks against pdf(wo, ., non-specular) scaled to their share;
    the specular picks' share is the model's: the number of specular lobes over the number of lobes, within 4 binomial sigmas."""
    from scipy import stats
    name, case, theta_o = CHI2[k]
    m = case["model"]
    sc, rows = install(scenes.glossy_plane_point_light_scene(MATTE), [case])
    scene = pbrt_hip.Scene(hip_ctx, sc)
    n = N_CHI2
    wo = chi2_wo(theta_o).astype(np.float32)
    u = np.random.default_rng(7).random((n, 2)).astype(np.float32)
    wo32 = np.broadcast_to(wo, (n, 3)).copy()
    q = scene.bsdf_query(rows[0], wo32, wo32, u)
    scene.close()
    ok = q["pdf_s"] > 0
    spec = ok & ((q["flags"] & 16) != 0)
    n_spec_lobes = sum(1 for l in m.lobes if l.type & lm.SPECULAR)
    # u0 picks uniformly among the lobes; a specular lobe picked may still sample nothing (total internal reflection): from above
    # and for reflection it always samples
    share = n_spec_lobes / m.n
    sigma = np.sqrt(share * (1 - share) / n)
    print(f"{name}: specular share {spec.mean():.5f}, model {share:.5f} +- {sigma:.2g}")
    assert abs(spec.mean() - share) <= 4 * sigma + 1e-12
    n_ns = n - int(spec.sum())
    ns_lobes = m.n - n_spec_lobes
    # among the draws that picked a non-specular lobe, directions follow the non-specular pdf
    expected = lm.pdf_bins(m, wo.astype(np.float64), lm.NON_SPECULAR).reshape(-1) * n_ns
    pick_ns = ok & ~spec
    counts = np.bincount(mm.bin_of(q["wi_s"][pick_ns].astype(np.float64)), minlength=expected.size)
    exp = np.append(expected, max(n_ns - expected.sum(), 0.0))
    obs = np.append(counts, n_ns - pick_ns.sum())
    small = exp < 5
    e = np.append(exp[~small], exp[small].sum())
    o = np.append(obs[~small], obs[small].sum())
    keep = e > 0
    chi2 = float(np.sum((o[keep] - e[keep]) ** 2 / e[keep]))
    p = float(stats.chi2.sf(chi2, keep.sum() - 1))
    print(f"  chi2 {chi2:.5g} over {keep.sum()} bins, p {p:.3g}, nothing sampled {1 - ok.mean():.4f}, {ns_lobes} non-specular lobes")
    assert o[~keep].sum() == 0, "samples where the pdf has no mass"
    assert p > 1e-3, (chi2, int(keep.sum()), p)


# ---- point light: Li = f(wo, wi) I |cos theta_i| / r^2 ----
POINT = {"uber": _single(scenes.uber, lm.uber, kd=KD, ks=0.4, kr=0.3, kt=0.2, opacity=0.8, u_roughness=0.4, v_roughness=0.4, remap=False),
         "translucent": _single(scenes.translucent, lm.translucent, kd=KD, ks=0.5, roughness=0.5, remap=False),
         "mix": CASES[[c["name"] for c in CASES].index("mix_matte_metal")]}
POINT_CASES = [("uber", 1, 1), ("uber", -1, -1), ("mix", 1, 1)] + [("translucent", e, l) for e in (1, -1) for l in (1, -1)]


@pytest.mark.parametrize("which,eye,light", POINT_CASES, ids=[f"{c[0]}-eye{c[1]:+d}-light{c[2]:+d}" for c in POINT_CASES])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_point_light_closed_form(hip_ctx, which, eye, light, integrator):
    case = POINT[which]
    m = case["model"]
    p_light, I = np.array([0.3, -0.2, 1.5 * light]), np.array([2.0, 3.0, 4.0])
    scene = _scene_with(hip_ctx, scenes.glossy_plane_point_light_scene(MATTE, tuple(p_light), tuple(I)), case)
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
        return lm.bsdf_f(m, -d, wi) * I * np.abs(wi[:, 2:3]) / r2[:, None], in_band(m, -d, wi)

    ref, band = reference(rays)
    rays = rays[~band & np.all(ref > 0, axis=1)]
    assert len(rays) >= 30
    ref, band = reference(rays)
    keys = np.arange(len(rays), dtype=np.uint64) * 7919 + 3
    rgb, _ = scene.li(rays, keys, integrator=integrator, max_depth=1, light_strategy=0)
    scene.close()
    print(f"worst relative difference {np.max(np.abs(rgb / ref - 1)):.3g}")
    np.testing.assert_allclose(rgb, ref, rtol=1e-4)


# ---- furnace: Le albedo(wo), specular lobes included ----
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("k", range(len(FURNACE)), ids=[c[0] for c in FURNACE])
def test_furnace_closed_form(hip_ctx, k, integrator):
    """path at max_depth 1 (the escaped specular ray adds the environment before the depth test), direct lighting and Whitted at 2
    (their specular branches; Whitted samples the environment once per vertex with f under BSDF_ALL, where specular lobes give 0)."""
    _, case, below = FURNACE[k]
    m = case["model"]
    Le = np.array([1.0, 0.8, 0.6])
    scene = _scene_with(hip_ctx, scenes.glossy_plane_env_scene(MATTE, tuple(Le)), case)
    wo = furnace_wo(below)
    w = h = 64
    cam = scenes.orthographic_camera(tuple(5 * wo), (0, 0, 0), (0, 0, 1), 1.0, w, h)
    film, _ = scene.render(cam, w, h, 16, integrator=integrator, max_depth=1 if integrator == PATH else 2, seed=5, light_strategy=0)
    scene.close()
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    albedo, err = furnace_reference(m, wo)
    ref = Le * albedo
    mean, se = rgb.mean(0), rgb.std(0) / np.sqrt(len(rgb))
    print(f"mean {mean} ref {ref} se {se} quadrature error {Le * err}")
    assert np.all(Le * err < se / 4 + 1e-12), (err, se)
    assert np.all(np.abs(mean - ref) < 4 * se + 1e-4 * ref), (mean, ref, se)


# ---- exact pass-through ----
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("opacity", [0.0, 0.25])
def test_exact_pass_through(hip_ctx, opacity, integrator):
    """the camera looks through an uber plane with Kd = Ks = Kr = Kt = 0 straight at an emitter: every pixel is (1 - o) Le. The
    path integrator only adds Le at the second hit after a SPECULAR bounce; the other two only get there through their
    specular transmit branch."""
    Le = np.array([1.0, 0.8, 0.6])
    pos, idx = scenes._plane_z0(1e3)
    low = pos.copy()
    low[:, 2] = -1.0
    sc = dict(positions=np.concatenate([pos, low]), indices=np.concatenate([idx, idx + 4]), tri_material=np.array([0, 0, 1, 1], np.int32),
              materials=scenes._materials([MATTE, (scenes.MAT_MATTE, (0, 0, 0), (0, 0, 0), 1.0)]), tri_light=np.array([-1, -1, 0, 1], np.int32),
              lights=scenes._lights([(scenes.LIGHT_DIFFUSE_AREA, tuple(Le), 2, 1, 1), (scenes.LIGHT_DIFFUSE_AREA, tuple(Le), 3, 1, 1)]))
    sc["lobe_descs"] = {0: scenes.uber(kd=0.0, ks=0.0, kr=0.0, kt=0.0, opacity=opacity)}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    w = h = 64
    cam = scenes.orthographic_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 1.0, w, h)
    film, _ = scene.render(cam, w, h, 4, integrator=integrator, max_depth=5 if integrator == PATH else 2, seed=3)
    scene.close()
    rgb = pbrt_hip.film_to_rgb(film).reshape(-1, 3).astype(np.float64)
    want = (1.0 - opacity) * Le
    print(f"opacity {opacity}: worst relative difference {np.max(np.abs(rgb / want - 1)):.3g}")
    np.testing.assert_allclose(rgb, np.broadcast_to(want, rgb.shape), rtol=1e-6)


# ---- one-lobe lists do the matte row's work ----
def _render(hip_ctx, sc, integrator, shade_order, w=64, h=64, spp=4, cam=None):
    scene = pbrt_hip.Scene(hip_ctx, sc)
    cam = scenes.random_triangles_camera(w, h) if cam is None else cam
    film, st = scene.render(cam, w, h, spp, integrator=integrator, max_depth=5, seed=11, shade_order=shade_order)
    scene.close()
    return film, st


@pytest.mark.parametrize("shade_order", [0, 1, 2])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_one_lambertian_lobe_renders_the_matte_row(hip_ctx, integrator, shade_order):
    """uber(Kd, everything else 0, opacity 1) and translucent(Kd, Ks 0, reflect 1, transmit 0) are LambertianReflection(Kd): the
    film of the PBRT_MAT_MATTE row with equal ray counts, within 1e-5 relative per pixel"""
    sc = scenes.mixed_materials_scene(n_tris=3000)
    kd = tuple(float(c) for c in sc["materials"][0]["kd"])
    assert sc["materials"][0]["type"] == scenes.MAT_MATTE and max(kd) <= 1.0
    want, s0 = _render(hip_ctx, sc, integrator, shade_order)
    for desc in (scenes.uber(kd=kd, ks=0.0, kr=0.0, kt=0.0, opacity=1.0), scenes.translucent(kd=kd, ks=0.0, reflect=1.0, transmit=0.0)):
        sc1 = dict(sc)
        sc1["lobe_descs"] = {0: desc}
        got, s1 = _render(hip_ctx, sc1, integrator, shade_order)
        print(f"bit for bit: {np.array_equal(want.view(np.uint32), got.view(np.uint32))}")
        assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


# ---- old rows unchanged beside a lobe row ----
def _disney_mixed():
    sc = dict(scenes.mixed_materials_scene(n_tris=3000))
    first = len(sc["materials"])
    sc["materials"] = np.concatenate([sc["materials"], scenes._materials([MATTE])])
    sc["disney_descs"] = {first: scenes.disney((0.8, 0.5, 0.3), sheen=0.5, clearcoat=1.0, spec_trans=0.3)}
    tm = sc["tri_material"].copy()
    tm[:3000] = np.arange(3000) % 4
    sc["tri_material"] = tm
    return sc


def _level2_mixed():
    from test_gpu_disney import _level2_mixed as f
    return f()


@pytest.mark.parametrize("shade_order", [0, 1, 2])
@pytest.mark.parametrize("integrator", [PATH, DIRECT])
@pytest.mark.parametrize("base", ["mixed", "glossy_mixed", "level2_mixed", "disney_mixed"])
def test_unused_uber_row_leaves_old_films_bit_identical(hip_ctx, base, integrator, shade_order):
    """an uber row no triangle uses selects the lobe-list kernels: the rows of levels 0 to 3 render what they rendered"""
    sc = {"mixed": lambda: scenes.mixed_materials_scene(n_tris=3000), "glossy_mixed": _glossy_mixed, "level2_mixed": _level2_mixed,
          "disney_mixed": _disney_mixed}[base]()
    f0, s0 = _render(hip_ctx, sc, integrator, shade_order)
    sc1 = dict(sc)
    first = len(sc["materials"])
    sc1["materials"] = np.concatenate([sc["materials"], scenes._materials([MATTE])])
    sc1["lobe_descs"] = {first: scenes.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5)}
    f1, s1 = _render(hip_ctx, sc1, integrator, shade_order)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert (s0["rays_closest"], s0["rays_shadow"]) == (s1["rays_closest"], s1["rays_shadow"])


# ---- a mix copies its operands ----
def test_mix_copies_its_operands(hip_ctx):
    sc = scenes.glossy_plane_point_light_scene(MATTE)
    sc["materials"] = scenes._materials([(scenes.MAT_MATTE, (0.6, 0.5, 0.4), (0, 0, 0), 1.0), scenes.metal((0.2, 0.9, 1.1), (3.0, 2.5, 2.0), 0.2), MATTE])
    sc["lobe_descs"] = {2: scenes.mix(0, 1, 0.3)}
    scene = pbrt_hip.Scene(hip_ctx, sc)
    m = CASES[[c["name"] for c in CASES].index("mix_matte_metal")]["model"]
    wo, wi, u = directions(m, 500, 5)
    before = scene.bsdf_query(2, wo, wi, u)
    scene.set_material(0, scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.25))
    scene.set_lobe_material(1, scenes.uber())
    after = scene.bsdf_query(2, wo, wi, u)
    assert not np.array_equal(scene.bsdf_query(0, wo, wi, u)["f"], before["f"])
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    scene.set_lobe_material(2, scenes.mix(0, 1, 0.3))  # set again: the operands as they are now
    assert not np.array_equal(scene.bsdf_query(2, wo, wi, u)["f"], before["f"])
    scene.close()


# ---- replacement in both directions ----
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_replacement(hip_ctx, integrator):
    """set_material and set_disney_material over a lobe row give the film of the scene that never had it, and a lobe row over
    either gives the lobe row's film"""
    cam = scenes.random_triangles_camera(64, 64)
    kw = dict(integrator=integrator, max_depth=5, seed=11, shade_order=0)
    uber = scenes.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5)
    sub, dis = scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.1, 0.3), scenes.disney((0.8, 0.5, 0.3), clearcoat=1.0)
    base = scenes.mixed_materials_scene(n_tris=3000)
    want = {}
    for name, key, desc in (("sub", "material_descs", sub), ("dis", "disney_descs", dis), ("uber", "lobe_descs", uber)):
        sc = dict(base)
        sc[key] = {0: desc}
        want[name] = _render(hip_ctx, sc, integrator, 0)[0]
    scene = pbrt_hip.Scene(hip_ctx, base)
    steps = [("uber", lambda: scene.set_lobe_material(0, uber)), ("sub", lambda: scene.set_material(0, sub)),
             ("uber", lambda: scene.set_lobe_material(0, uber)), ("dis", lambda: scene.set_disney_material(0, dis)),
             ("uber", lambda: scene.set_lobe_material(0, uber))]
    for name, step in steps:
        step()
        got, _ = scene.render(cam, 64, 64, 4, **kw)
        assert np.array_equal(want[name].view(np.uint32), got.view(np.uint32)), name
    scene.close()
    assert not np.array_equal(want["uber"], want["sub"]) and not np.array_equal(want["uber"], want["dis"])


# ---- instances ----
def test_instance_material_override_names_a_lobe_row(hip_ctx):
    sc = dict(scenes.instanced_scene(n_base_tris=2000, n_instances=60, extent=1.5))
    first = len(sc["materials"])
    sc["materials"] = np.concatenate([sc["materials"], scenes._materials([MATTE, MATTE])])
    sc["lobe_descs"] = {first: scenes.uber(kd=KD, ks=0.3, kr=0.2, kt=0.3, opacity=0.5), first + 1: scenes.mix(0, first, 0.5)}
    sc["instance_material"] = (np.arange(60) % (first + 2)).astype(np.int32)
    cam = scenes.instanced_camera(64, 64, extent=1.5)
    films = [_render(hip_ctx, sc, PATH, so, cam=cam)[0] for so in (0, 1, 2)]
    assert all(np.array_equal(films[0].view(np.uint32), f.view(np.uint32)) for f in films[1:])
    sc_m = dict(sc)
    sc_m.pop("lobe_descs")
    other = _render(hip_ctx, sc_m, PATH, 0, cam=cam)[0]
    assert np.isfinite(films[0]).all() and films[0][..., :3].mean() > 0 and not np.array_equal(films[0], other)


# ---- refusals ----
def test_refusals_leave_the_scene_unchanged(hip_ctx):
    scene = pbrt_hip.Scene(hip_ctx, refusal_scene(scenes.glossy_plane_point_light_scene(MATTE)))
    rays = _point_light_rays(4)
    keys = np.arange(len(rays), dtype=np.uint64)
    m = lm.uber()
    wo, wi, u = directions(m, 200, 9)
    before, _ = scene.li(rays, keys, max_depth=1)
    q_before = [scene.bsdf_query(r, wo, wi, u)["f"] for r in range(7)]
    for row, desc, why in REFUSED:
        with pytest.raises(pbrt_hip.PbrtHipError, match=f"\\(1\\): pbrt_hip_scene_set_lobe_material: .*{why}"):
            scene.set_lobe_material(row, desc)
    after, _ = scene.li(rays, keys, max_depth=1)
    assert np.array_equal(before, after)
    for r in range(7):
        assert np.array_equal(q_before[r], scene.bsdf_query(r, wo, wi, u)["f"])
    for desc in ACCEPTED:
        scene.set_lobe_material(6, desc)
        assert np.isfinite(scene.bsdf_query(6, wo, wi, u)["f"]).all()
    with pytest.raises(pbrt_hip.PbrtHipError, match="not PBRT_MAT_PLASTIC"):
        scene.set_material_roughness(6, 0.1)
    now, _ = scene.li(rays, keys, max_depth=1)
    assert np.array_equal(before, now)  # row 0 is what the plane names
    scene.close()


def test_scenes_with_shapes_or_map_lights_refuse_lobe_rows(hip_ctx):
    """their shading builds stay at level 3: a stated limit"""
    from test_gpu_shapes import shape_scene
    sc = scenes.glossy_plane_point_light_scene(MATTE)
    sc["lights"] = scenes._lights([scenes.goniometric_light(None, (2.0, 3.0, 4.0))])
    scene = pbrt_hip.Scene(hip_ctx, sc)
    with pytest.raises(pbrt_hip.PbrtHipError, match="projection or goniometric light"):
        scene.set_lobe_material(0, scenes.uber())
    scene.close()
    scene = pbrt_hip.Scene(hip_ctx, shape_scene([scenes.disk(0.0, 0.5)]))
    with pytest.raises(pbrt_hip.PbrtHipError, match="general quadric shapes"):
        scene.set_lobe_material(0, scenes.uber())
    scene.close()
