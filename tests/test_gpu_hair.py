"""HairMaterial on the device (pbrt_hip_scene_set_hair_material): the BSDF pinned to the float64 model (hair_model.py) through
pbrt_hip_bsdf_query_hair, closed forms through pbrt_hip_li on single strands, white and brown hair in a white furnace, the films
of curve scenes without a hair row unchanged by the hair builds, and refusals and replacements that leave scene and context
usable."""
import re
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import curve_cases as cc
import curve_model as cm
import hair_model as hm
from hair_cases import BROWN, CASES, DESCS, LEFT_OUT_MAX_SHARE, MODELS, N_ZERO, left_out, points
from test_cpp_example import _build
from test_gpu_curves import STRIP_CP, as_rays, curve_scene

pytestmark = pytest.mark.gpu
PATH, DIRECT, WHITTED, AO = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO
GREY = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
HAIR_FLAGS = pbrt_hip.BSDF_GLOSSY | pbrt_hip.BSDF_REFLECTION | pbrt_hip.BSDF_TRANSMISSION


def hair_scene(curves, descs, lights=(), extra_rows=0):
    """a curve scene whose row 0 (the far triangle's) is grey and whose rows 1.. are hair rows; the curves name rows >= 1"""
    sc = curve_scene(curves, materials=scenes._materials([GREY] * (1 + len(descs) + extra_rows)), lights=lights)
    sc["hair_descs"] = {1 + k: d for k, d in enumerate(descs)}
    return sc


@pytest.fixture(scope="module")
def table(hip_ctx):
    strand = scenes.curve(STRIP_CP, 0.5, 0.5, type="flat", material=1, split_depth=0)
    scene = pbrt_hip.Scene(hip_ctx, hair_scene([strand], DESCS))
    yield scene
    scene.close()


def _rel(dev, ref):
    return np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300)


def _restatement(m, h, wo, wi, mask):
    """largest relative error of the model in float32 (constants as the device holds them) against float64 over mask: (f, pdf).
    Values below 1e-30 of the largest are left to the absolute check (float32 underflows where float64 does not)."""
    m32 = m.as32()
    h64, wo64, wi64 = h.astype(np.float64), wo.astype(np.float64), wi.astype(np.float64)
    out = []
    for fn in (lambda mm, a, b, c: hm.bsdf_f(mm, a, b, c), lambda mm, a, b, c: hm.bsdf_pdf(mm, a, b, c)[:, None]):
        lo, hi = fn(m32, h, wo, wi).astype(np.float64)[mask], fn(m, h64, wo64, wi64)[mask]
        big = np.abs(hi) > 1e-30 * np.abs(hi).max()
        out.append(float(_rel(lo[big], hi[big]).max()))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bsdf_query_hair_matches_model(table, i):
    """f and pdf within max(1e-4, 4 x the float32 restatement of the model on the same inputs), relative, outside the points
    hair_cases.left_out names (at most 2 %); zeros at wo.z == 0; the same u gives the same lobe p (wi_s within 1e-3 on all but 1e-3
    of the points); flags GLOSSY | REFLECTION | TRANSMISSION; f_s and pdf_s equal the device's own f and pdf at wi_s to 2e-3.
    Measured over the 12 cases: the float32 restatement 7.5e-7 .. 1.51e-4 for f and 7.6e-7 .. 1.51e-4 for the pdf (the largest at
    beta_m = 0.1, where Mp's exponent is a difference of terms near 600), so bounds of 1e-4 .. 6.1e-4; the device 1.07e-6 ..
    1.51e-4 and 1.1e-6 .. 1.51e-4, within 1.5 x the restatement in every case. wi_s: none of 4065 .. 4079 points beyond 1e-3
    (worst 1.0e-4); f_s / pdf_s against the device's own f / pdf at wi_s: 5.0e-7 .. 2.9e-5."""
    m = MODELS[i]
    h, wo, wi, u = points(300 + i)
    q = table.bsdf_query_hair(1 + i, h, wo, wi, u)
    h64, wo64, wi64 = h.astype(np.float64), wo.astype(np.float64), wi.astype(np.float64)
    f_ref, pdf_ref = hm.bsdf_f(m, h64, wo64, wi64), hm.bsdf_pdf(m, h64, wo64, wi64)
    out = left_out(wo, wi)
    assert out.mean() <= LEFT_OUT_MAX_SHARE
    keep = ~out
    e_f, e_pdf = _restatement(m, h, wo, wi, keep)
    rtol_f, rtol_pdf = max(1e-4, 4 * e_f), max(1e-4, 4 * e_pdf)
    for what, dev, ref, rtol in (("f", q["f"], f_ref, rtol_f), ("pdf", q["pdf"][:, None], pdf_ref[:, None], rtol_pdf)):
        assert np.isfinite(dev[keep]).all()
        big = keep[:, None] & (np.abs(ref) > 1e-30 * np.abs(ref[keep]).max())
        err = _rel(dev.astype(np.float64), ref)
        print(f"{CASES[i][0]} {what}: float32 restatement {e_f if what == 'f' else e_pdf:.3g}, bound {rtol:.3g}, device worst {err[big].max():.3g} "
              f"over {big.sum()} values")
        assert err[big].max() <= rtol, (what, err[big].max(), rtol)
        small = keep[:, None] & ~big
        assert np.all(np.abs(dev[small]) <= 1e-29 * np.abs(ref[keep]).max())
    zero = wo[:, 2] == 0
    assert zero.sum() == N_ZERO and np.all(q["f"][zero] == 0) and np.all(q["pdf"][zero] == 0) and np.all(q["pdf_s"][zero] == 0)

    # sample_f: the same u gives the same p and the same wi
    wi_m, f_m, pdf_m, ok_m, p_m = hm.bsdf_sample_f(m, h64, wo64, u.astype(np.float64))
    ok_d = q["pdf_s"] > 0
    assert np.mean(ok_d[keep] != ok_m[keep]) < 1e-3
    both = keep & ok_d & ok_m
    assert both.sum() > 0.9 * keep.sum()
    assert np.all(q["flags"][ok_d] == HAIR_FLAGS) and np.all(q["flags"][~ok_d] == 0)
    dw = np.abs(q["wi_s"][both] - wi_m[both]).max(axis=1)
    print(f"  wi_s: {both.sum()} compared, {np.mean(dw > 1e-3):.2g} beyond 1e-3, worst {np.sort(dw)[-3:]}, p counts {np.bincount(p_m[both], minlength=4)}")
    assert np.mean(dw > 1e-3) <= 1e-3
    sel = ok_d & ~left_out(wo, q["wi_s"])
    q2 = table.bsdf_query_hair(1 + i, h[sel], wo[sel], q["wi_s"][sel], u[sel])
    for what, a, b in (("pdf_s", q["pdf_s"][sel], q2["pdf"]), ("f_s", q["f_s"][sel], q2["f"])):
        err = np.abs(a - b) - (2e-3 * np.abs(b) + 1e-6 * np.abs(b).max())
        print(f"  {what} against the device's own value at wi_s: worst relative {(_rel(a.astype(np.float64), b.astype(np.float64)))[np.abs(b) > 1e-6 * np.abs(b).max()].max():.3g}")
        assert np.all(err <= 0), (what, np.sum(err > 0))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one ray, one strand: closed form through li
# ---------------------------------------------------------------------------------------------------------------------
LIGHT_I = (6.0, 5.0, 4.0)
STRAND_W = 0.5
# in the strips' own space: a flat strip along x at y = +1.5 and a cylinder strip at y = -1.5, the eye above them, the light above
# and to the side. Straight strips three widths apart: a ray that leaves one meets neither again (the model says so ray by ray)
STRAND_EYE, STRAND_LIGHT = (0.3, -0.2, 5.0), (1.5, 0.4, 3.0)
MIRROR = np.diag([1.0, -1.0, 1.0, 1.0])
VARIANTS = {"rigid": (cc.transform("rigid"), False), "reversed": (cc.transform("rigid"), True), "mirrored": (cc.transform("rigid") @ MIRROR, False)}


def _strands(m, reverse):
    """8 records: a flat and a cylinder strip of four segments each, under to_world = m"""
    recs = []
    for kind, y in (("flat", 1.5), ("cylinder", -1.5)):
        recs.append(scenes.curve(STRIP_CP + np.array([0.0, y, 0.0]), STRAND_W, STRAND_W, type=kind, to_world=m, material=1, split_depth=2,
                                 reverse_orientation=reverse))
    return scenes.curves(*recs)


def _strand_rays(m, n=1024):
    """the same n rays for every variant in the strips' own space, taken to the world by m: (o, d, the light's position)"""
    rng = np.random.default_rng(77)
    to_world = lambda p: np.asarray(p) @ m[:3, :3].T + m[:3, 3]
    target = np.stack([rng.uniform(-2.0, 2.0, n), np.where(np.arange(n) % 2 == 0, 1.5, -1.5) + rng.uniform(-0.2, 0.2, n), np.zeros(n)], -1)
    o = np.asarray(STRAND_EYE) + rng.uniform(-0.3, 0.3, (n, 3))
    o_w = to_world(o).astype(np.float32)
    return o_w, (to_world(target) - o_w).astype(np.float32), to_world(np.asarray(STRAND_LIGHT))


def _surface(curves, o, d, model, dtype):
    """curve_cases.surface_of in float64 or in float32 (the float32 restatement of the curve model's surface)"""
    R = len(o)
    s = dict(n=np.zeros((R, 3)), p=np.zeros((R, 3)), dpdu=np.zeros((R, 3)), v=np.zeros(R))
    for j, rec in enumerate(np.asarray(curves).reshape(-1)):
        mine = model["hit"] & (model["prim"] == j)
        if mine.any():
            r = cm.intersect(rec, o[mine], d[mine], np.full(mine.sum(), np.inf), dtype=dtype)
            for k in s:
                s[k][mine] = np.asarray(r[k], np.float64)
    return s


def _closed_form(m, surf, keep, d, p_light, v, mirror_h=False):
    sign = -1.0 if mirror_h else 1.0
    return cc.point_light_radiance(surf, keep, d, p_light, LIGHT_I, lambda wo, wi: hm.bsdf_f(m, sign * (-1.0 + 2.0 * v), wo, wi))


@pytest.mark.parametrize("integrator", [DIRECT, PATH, WHITTED], ids=["direct", "path", "whitted"])
def test_point_light_closed_form_on_strands(hip_ctx, integrator):
    """L = f(wo, wi; h = -1 + 2 v) |wi . n| I / d^2 at depth 1 on a flat and a cylinder strip (8 records) under a point light, no
    environment, in float64 from the curve model's surface frame and v, for the default hair row, on 1024 explicit rays.

    Tolerance: test 1's rule, max(1e-4, 4 x the float32 restatement of the model on the same inputs), relative, where the model
    is this closed form, so its restatement is the curve model's surface in float32 followed by the BSDF in float32; plus what
    moving v one float32 ulp does to f on the model; plus a millionth of the largest value for the rays whose f is 0. No ray is
    left out but those the float64 model does not decide clearly (a hit or a way to the light within 5 % of hit_width of a
    decision) and hair_cases.left_out's; at least 80 % of the rays are compared.
    Measured: 989 of 1024 rays compared; the restatement 2.9e-5 .. 3.0e-5, so a bound of 1.2e-4; the device 3.0e-5 .. 3.8e-5
    relative, at most 0.27 of the allowance.

    reverse_orientation gives the same radiance ray by ray (the normal turns, both directions turn with it by pi about the
    fibre, d phi and h stay). The mirrored to_world does NOT give the same radiance ray by ray, on pbrt-v3 either: the rays are the
    same in the strips' own space, so u, v and h are the same, while in the world the azimuths change sign and h does not. By
    the BSDF's symmetry f(h, d phi) = f(-h, -d phi) the mirrored strip shows what the plain one shows at -h, which is asserted
    ray by ray from the plain variant's surface; over a strip, whose h is symmetric, the two look alike."""
    desc, m = scenes.hair(), MODELS[4]
    got, want, kept = {}, {}, {}
    for name, (xf, reverse) in VARIANTS.items():
        curves = _strands(xf, reverse)
        assert len(curves) == 8
        o, d, p_light = _strand_rays(xf)
        g = pbrt_hip.Scene(hip_ctx, hair_scene(curves, [desc], lights=[scenes.point_light(tuple(p_light), LIGHT_I)]))
        rgb, _ = g.li(as_rays(o, d), np.arange(len(o), dtype=np.uint64), integrator=integrator, max_depth=1)
        g.close()
        model = cm.intersect_many(curves, o, d)
        surf = cc.surface_of(curves, o, d, np.inf, model)
        hit = model["hit"] & (model["margin"] >= 0.05)
        way = cc.leaving(curves, surf, hit, p_light - surf["p"][hit], 1.0 - 1e-4)
        keep = np.flatnonzero(hit)[(way["margin"] >= 0.05) & ~way["hit"]]
        v = model["v"][keep]
        w64 = _closed_form(m, surf, keep, d, p_light, v)
        moved = _closed_form(m, surf, keep, d, p_light, np.nextafter(v.astype(np.float32), np.float32(2)).astype(np.float64))
        # the float32 restatement: the surface by the curve model in float32, the BSDF in float32
        s32 = _surface(curves, o, d, model, np.float32)
        ss, ts, n = cc.local_frame(s32, keep)
        wo_w = -d[keep].astype(np.float64)
        wo_w /= np.linalg.norm(wo_w, axis=1, keepdims=True)
        wi_w = p_light - s32["p"][keep]
        r2 = (wi_w * wi_w).sum(-1)
        wi_w /= np.sqrt(r2)[:, None]
        loc = lambda w: np.stack([(w * ss).sum(-1), (w * ts).sum(-1), (w * n).sum(-1)], -1).astype(np.float32)
        wo_l, wi_l = loc(wo_w), loc(wi_w)
        f32 = hm.bsdf_f(m.as32(), (np.float32(-1.0) + np.float32(2.0) * s32["v"][keep].astype(np.float32)), wo_l, wi_l).astype(np.float64)
        w32 = f32 * np.asarray(LIGHT_I) * (np.abs(wi_l[:, 2].astype(np.float64)) / r2)[:, None]
        clear = ~left_out(wo_l, wi_l)
        scale = np.abs(w64[clear]).max()
        big = clear[:, None] & (np.abs(w64) > 1e-4 * scale)
        e = float((np.abs(w32 - w64) / np.abs(w64))[big].max())
        rtol = max(1e-4, 4 * e)
        allowed = rtol * np.abs(w64) + np.abs(moved - w64) + 1e-6 * scale
        dev = rgb[keep].astype(np.float64)
        worst = (np.abs(dev - w64) / allowed)[clear].max()
        print(f"{name}: compared {clear.sum()} of {len(o)} ({model['hit'].sum()} hit), float32 restatement {e:.3g}, rtol {rtol:.3g}, "
              f"largest {scale:.3g}, worst relative error {(np.abs(dev - w64) / np.abs(w64))[big].max():.3g}, worst error over allowance {worst:.3f}")
        assert np.isfinite(rgb).all() and clear.sum() >= 0.8 * len(o) and (w64[clear] > 0).all(-1).mean() > 0.5
        assert worst <= 1.0
        got[name], want[name], kept[name] = dev, (w64, allowed, surf, d, p_light, v, keep), (keep, clear)
    # across the variants, ray by ray (the rays are the same in the strips' own space)
    k0, c0 = kept["rigid"]
    w0, a0 = want["rigid"][0], want["rigid"][1]
    k1, c1 = kept["reversed"]
    both, i0, i1 = np.intersect1d(k0[c0], k1[c1], return_indices=True)
    assert len(both) >= 0.8 * 1024
    assert np.all(np.abs(got["reversed"][c1][i1] - got["rigid"][c0][i0]) <= 2 * a0[c0][i0])
    # mirrored: the plain variant's closed form at -h
    _, _, surf0, d0, pl0, v0, keep0 = want["rigid"]
    flipped = _closed_form(m, surf0, keep0, d0, pl0, v0, mirror_h=True)
    k2, c2 = kept["mirrored"]
    both, i0, i2 = np.intersect1d(k0[c0], k2[c2], return_indices=True)
    assert len(both) >= 0.8 * 1024
    a2 = want["mirrored"][1]
    assert np.all(np.abs(got["mirrored"][c2][i2] - flipped[c0][i0]) <= a0[c0][i0] + a2[c2][i2])
    differs = np.abs(flipped[c0][i0] - w0[c0][i0]) > 10 * a0[c0][i0]
    print(f"mirrored: equals the plain closed form at -h on {len(both)} rays; at +h it would differ on {differs.mean():.2f} of them")
    assert differs.mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 3. white hair in a white furnace
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", [0, 2], ids=["uniform", "spatial"])
@pytest.mark.parametrize("kind", ["flat", "cylinder"])
def test_white_hair_in_a_white_furnace(hip_ctx, kind, strategy):
    """one wide strand, sigma_a = 0, beta_m = beta_n = 0.3, alpha = 0, under a constant environment L = 1: path integrator, depth
    16, roulette off, 32 x 32 x 64 spp. Every pixel wholly inside the strand is 1 within 5 standard errors of its own samples plus
    2e-3. With brown sigma_a the same pixels are below 1 and ordered as sigma_a is (red absorbs least)."""
    W = H = 32
    spp = 64
    strand = scenes.curve(STRIP_CP, 1.5, 1.5, type=kind, material=1, split_depth=1)
    cam = scenes.orthographic_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, W, H)
    env = [(scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1)]
    inside = np.zeros((H, W), bool)
    inside[H // 2 - 8:H // 2 + 8, :] = True  # |y| <= 0.5 of a strand 1.5 wide (the cylinder's silhouette as well)
    means = {}
    for name, sa in (("white", 0.0), ("brown", BROWN)):
        g = pbrt_hip.Scene(hip_ctx, hair_scene([strand], [scenes.hair(sigma_a=sa, alpha=0.0)], lights=env))
        rays, keys, _, pix = g.camera_rays(cam, W, H, spp, seed=3)
        rgb, _ = g.li(rays, keys, integrator=PATH, max_depth=16, light_strategy=strategy, rr_threshold=0.0)
        g.close()
        assert np.isfinite(rgb).all()
        px = pix[:, 1].astype(int) * W + pix[:, 0].astype(int)
        cnt = np.bincount(px, minlength=W * H).astype(np.float64)
        mean = np.stack([np.bincount(px, weights=rgb[:, c].astype(np.float64), minlength=W * H) for c in range(3)], 1) / cnt[:, None]
        sq = np.stack([np.bincount(px, weights=rgb[:, c].astype(np.float64) ** 2, minlength=W * H) for c in range(3)], 1) / cnt[:, None]
        se = np.sqrt(np.maximum(sq - mean * mean, 0) / (cnt[:, None] - 1))
        sel = inside.ravel() & (cnt == spp)
        assert sel.sum() == inside.sum()
        means[name] = (mean[sel], se[sel])
        print(f"{kind} strategy {strategy} {name}: mean over the pixels {mean[sel].mean(0)}, largest |mean - 1| / (5 se + 2e-3) "
              f"{(np.abs(mean[sel] - 1) / (5 * se[sel] + 2e-3)).max():.3f}")
    mean, se = means["white"]
    assert np.all(np.abs(mean - 1) <= 5 * se + 2e-3)
    mean, se = means["brown"]
    assert np.all(mean < 1) and np.all(mean[:, 0] > mean[:, 1]) and np.all(mean[:, 1] > mean[:, 2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. old scenes are untouched
# ---------------------------------------------------------------------------------------------------------------------
def _mixed_curve_scene(with_hair_row):
    recs = [scenes.curve(cc.BENT, 0.3, 0.2, type=k, material=1 + j % 2, split_depth=1,
                         to_world=np.array([[1, 0, 0, 0], [0, 1, 0, 0.6 * j - 0.6], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64))
            for j, k in enumerate(("flat", "cylinder", "flat"))]
    rows = [GREY, (scenes.MAT_MATTE, (0.6, 0.4, 0.2), (0, 0, 0), 1.0), scenes.plastic((0.3, 0.5, 0.3), (0.3, 0.3, 0.3), 0.2), GREY]
    sc = curve_scene(recs, materials=scenes._materials(rows),
                     lights=[scenes.distant_light((0.2, 0.3, 1.0), (2.0, 2.0, 2.0)), (scenes.LIGHT_INFINITE, (0.3, 0.3, 0.4), -1, 0, 1)])
    if with_hair_row:
        sc["hair_descs"] = {3: scenes.hair()}  # nothing names row 3
    return sc


@pytest.mark.parametrize("integrator,kw", [(PATH, dict(shade_order=0)), (PATH, dict(shade_order=1)), (PATH, dict(shade_order=2)),
                                           (DIRECT, {}), (WHITTED, {}), (AO, dict(ao_samples=4))], ids=lambda v: str(v))
def test_unused_hair_row_leaves_curve_films_bit_identical(hip_ctx, integrator, kw):
    """the pattern of test_unused_shape_leaves_old_films_bit_identical: a hair row nobody names switches the render to the hair
    builds, which shade every other row through the curve builds' code. That the switch happens, and only in the scene with the
    row, is read from Scene.shading_needs (pbrt_hip_scene_shading_needs: the SceneNeeds that kernel_select.h's direct_kernel and
    path_kernel pick the builds from: curves and hair together select k_shade_hair / k_shade_direct<., 3 + kDirectCurves +
    kDirectHair>, curves alone the curve builds)."""
    cam = scenes.perspective_camera((0.6, 0.2, 4.0), (0.6, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, 64, 64)
    out = []
    for with_row in (False, True):
        g = pbrt_hip.Scene(hip_ctx, _mixed_curve_scene(with_row))
        needs = g.shading_needs()
        assert needs["curves"] and needs["shapes"] and needs["hair"] == with_row and not (needs["lobes"] or needs["moving"]), needs
        film, st = g.render(cam, 64, 64, 4, integrator=integrator, max_depth=3, seed=5, **kw)
        assert g.shading_needs() == needs
        g.close()
        out.append((film, (st["camera_samples"], st["rays_closest"], st["rays_shadow"])))
    assert out[0][0][..., :3].mean() > 0.01
    assert out[0][1] == out[1][1]
    assert out[0][0].tobytes() == out[1][0].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals and replacement
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_replacement_leave_the_context_usable(hip_ctx):
    strand = scenes.curve(STRIP_CP, 1.5, 1.5, type="cylinder", material=1, split_depth=1)
    sun = [scenes.distant_light((0.2, 0.3, 1.0), (2.0, 2.0, 2.0))]
    cam = scenes.orthographic_camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 32, 32)
    g = pbrt_hip.Scene(hip_ctx, hair_scene([strand], [scenes.hair()], lights=sun, extra_rows=1))
    render = lambda: g.render(cam, 32, 32, 4, max_depth=3, seed=2)[0].tobytes()
    before = render()
    refused = [
        (lambda: g.set_hair_material(1, scenes.hair(beta_m=1.5)), "beta_m must be in"),
        (lambda: g.set_hair_material(1, scenes.hair(beta_n=-0.5)), "beta_n must be in"),
        (lambda: g.set_hair_material(1, scenes.hair(eta=0.0)), "eta must be > 0"),
        (lambda: g.set_hair_material(1, scenes.hair(sigma_a=(-1.0, 0.0, 0.0))), "sigma_a must be >= 0"),
        (lambda: g.set_hair_material(1, scenes.hair(eumelanin=-1.0)), "eumelanin and pheomelanin must be >= 0"),
        (lambda: g.set_hair_material(1, scenes.hair(color=(0.0, 0.5, 0.5))), "color must be in"),
        (lambda: g.set_hair_material(1, dict(scenes.hair(), absorption=9)), "unknown absorption"),
        (lambda: g.set_hair_material(1, scenes.hair(alpha=float("inf"))), "every field must be finite"),
        (lambda: g.set_hair_material(0, scenes.hair()), "a triangle or a quadric shape names the row"),
        (lambda: g.set_hair_material(7, scenes.hair()), "material index out of range"),
        (lambda: g.set_hair_material(1, None), "null desc"),
        # (a hair row lives in a scene with curves, and such a scene takes no lobe rows at all: the mix is refused for that)
        (lambda: g.set_lobe_material(2, scenes.mix(1, 0, 0.5)), "take no lobe rows"),
        (lambda: g.bsdf_query(1, np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 2))), "pbrt_hip_bsdf_query_hair"),
        (lambda: g.bsdf_query_hair(0, np.zeros(1), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 2))), "not a hair row"),
        (lambda: g.set_material_roughness(1, 0.2), "a hair row has no roughness"),
    ]
    for call, why in refused:
        with pytest.raises(pbrt_hip.PbrtHipError, match=why):
            call()
        assert render() == before, why
    # a scene without curves takes no hair row, and stays usable
    plain = pbrt_hip.Scene(hip_ctx, scenes.cornell_box())
    with pytest.raises(pbrt_hip.PbrtHipError, match="the scene holds no curves"):
        plain.set_hair_material(1, scenes.hair())
    plain.close()
    # replacement, both ways: matte over the hair row is the matte scene's film, hair over it again the first film
    assert g.shading_needs()["hair"]
    g.set_material(1, scenes.matte_sigma((0.5, 0.5, 0.5), 0.0))
    assert not g.shading_needs()["hair"]  # the last hair row is gone: the curve builds run again
    matte = render()
    ref = pbrt_hip.Scene(hip_ctx, curve_scene([strand], materials=scenes._materials([GREY] * 3), lights=sun))
    assert matte == ref.render(cam, 32, 32, 4, max_depth=3, seed=2)[0].tobytes() and matte != before
    ref.close()
    g.set_disney_material(1, scenes.disney((0.5, 0.3, 0.2)))
    assert render() not in (matte, before)
    g.set_hair_material(1, scenes.hair())
    assert render() == before
    g.set_hair_material(1, scenes.hair(sigma_a=0.0))
    assert render() != before
    g.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C++ example
# ---------------------------------------------------------------------------------------------------------------------
def _hair_strands():
    """the scene of examples/render_hair_strands.cpp, array for array (the same 31-bit generator, in float32)"""
    state = [2024]

    def unit():
        state[0] = (state[0] * 1103515245 + 12345) & 0x7FFFFFFF
        return np.float32(state[0] >> 7) / np.float32(16777216.0)

    f = np.float32
    n, recs = 48, []
    for i in range(n):
        x = f(-0.8) + f(1.6) * (f(i) + unit()) / f(n)
        z = f(0.3) * (unit() - f(0.5))
        sway = f(0.5) * (unit() - f(0.5))
        curl = f(0.4) * (unit() - f(0.5))
        cp = np.array([(x, f(0.9), z), (x + f(0.3) * sway, f(0.3), z + curl), (x + sway, f(-0.3), z - curl),
                       (x + f(1.5) * sway, f(-0.9), z + f(0.5) * curl)], dtype=np.float32)
        recs.append(scenes.curve(cp, 0.03, 0.012, type="cylinder", material=1, split_depth=1))
    sun = scenes.distant_light((0.4, 0.5, 1.0), (3.0, 3.0, 3.0))
    ln = np.sqrt(f(0.4) * f(0.4) + f(0.5) * f(0.5) + f(1.0))
    sun["pos"] = (f(0.4) / ln, f(0.5) / ln, f(1.0) / ln)
    sc = curve_scene(scenes.curves(*recs), materials=scenes._materials([GREY] * 2), lights=[sun, (scenes.LIGHT_INFINITE, (0.35, 0.4, 0.5), -1, 0, 1)])
    sc["hair_descs"] = {1: scenes.hair(eumelanin=0.8, pheomelanin=0.2)}
    return sc


def test_cpp_hair_strands_render_what_the_python_binding_renders(tmp_path, hip_ctx):
    W = H = 32
    png, raw = tmp_path / "hair.png", tmp_path / "film.raw"
    r = subprocess.run([_build(tmp_path, "render_hair_strands.cpp"), str(png), str(W), str(H), str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"hair strands: 96 curve segments, (\d+) camera samples, (\d+) closest-hit \+ (\d+) shadow rays", r.stdout)
    assert m and int(m.group(1)) == W * H * 16, r.stdout
    g = pbrt_hip.Scene(hip_ctx, _hair_strands())
    film, st = g.render(scenes.perspective_camera((0.0, 0.0, 3.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 36.0, W, H), W, H, 16, max_depth=5, seed=7,
                        light_strategy=2)  # PathIntegrator::new's default: "spatial"
    g.close()
    assert (st["camera_samples"], st["rays_closest"], st["rays_shadow"]) == tuple(int(m.group(k)) for k in (1, 2, 3))
    assert film[..., :3].mean() > 0.01 and np.isfinite(film).all()
    assert raw.read_bytes() == film.tobytes()
    ref = tmp_path / "ref.png"
    pbrt_hip.write_png(str(ref), pbrt_hip.film_to_rgb(film))
    assert png.read_bytes() == ref.read_bytes()
