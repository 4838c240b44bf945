"""The Curve shape on the CPU: the float64 model (tests/curve_model.py) against closed forms, the shared cases' exclusion cap and
float32 spread (tests/curve_cases.py), the edge cases' margins, caps, hit shares and depths, how far a reversed normal or a turned
frame moves what test_gpu_curve_shading.py expects, and the host surface of the feature (record layout, symbols,
pbrt_hip_curve_world_bounds)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import curve_cases as cc
import curve_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, W = 1.2, 0.05  # the straight test curve: along +x from the origin, constant width


def _straight(kind, normals=None, width1=W):
    return scenes.curve(cc.STRAIGHT, W, width1, type=kind, normals=normals, split_depth=0)[0]


def _rays(n, seed, spread=2.0):
    """rays from a shell of radius 3 aimed at points within `spread` widths of the axis"""
    rng = np.random.default_rng(seed)
    axis_pt = np.stack([rng.uniform(-0.1, L + 0.1, n), np.zeros(n), np.zeros(n)], -1)
    off = rng.normal(size=(n, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    target = axis_pt + off * (rng.uniform(0, spread, (n, 1)) * W)
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    o = target + 3.0 * away
    d = (target - o) * rng.uniform(0.2, 1.5, (n, 1))
    return o, d


def _line_line(o, d):
    """closest approach of the line o + t d and the x axis: (s on the axis, t on the ray, distance)"""
    e = np.array([1.0, 0.0, 0.0])
    dd, de, ee = (d * d).sum(-1), d @ e, 1.0
    wo = o  # o - a with a = 0
    den = dd * ee - de * de
    s = (dd * (wo @ e) - de * (wo * d).sum(-1)) / den
    t = (de * (wo @ e) - ee * (wo * d).sum(-1)) / den
    gap = o + t[:, None] * d - s[:, None] * e
    return s, t, np.linalg.norm(gap, axis=1)


def test_straight_flat_curve_against_the_closed_form():
    """a hit iff the ray passes within w / 2 of the axis in its own perpendicular plane, between the two ends; t is the ray
    parameter of the axis point nearest to the ray in that plane"""
    rec = _straight("flat")
    o, d = _rays(6000, 1)
    r = cm.intersect(rec, o, d)
    s, t, gap = _line_line(o, d)
    want = (gap <= W / 2) & (s >= 0) & (s <= L) & (t >= 0)
    clear = (np.abs(gap - W / 2) > 1e-7) & (np.abs(s) > 1e-6) & (np.abs(s - L) > 1e-6)
    assert want[clear].mean() > 0.2
    np.testing.assert_array_equal(r["hit"][clear], want[clear])
    h = r["hit"] & clear
    # t: (P - o) . d / |d|^2 for the axis point P = (s, 0, 0)
    tp = ((np.stack([s, 0 * s, 0 * s], -1) - o) * d).sum(-1) / (d * d).sum(-1)
    # (the record holds float32 control points and widths: 1.2, 0.8, 0.4 and 0.05 are each off by up to 6e-8 of themselves)
    np.testing.assert_allclose(r["t"][h], tp[h], rtol=0, atol=2e-7)
    np.testing.assert_allclose(r["u"][h], s[h] / L, rtol=0, atol=2e-7)
    np.testing.assert_allclose(np.abs(r["v"][h] - 0.5), gap[h] / W, rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["p_error"][h], 2 * W)
    assert (r["depth"] == 0).all()


def test_straight_cylinder_normal_follows_v():
    """n = the flat strip's normal (the ray direction with its part along the axis removed) turned about the axis by
    theta = lerp(v, -90, 90) degrees: no part along the axis, cos(theta) along the flat normal, sin(theta) to one fixed side"""
    rec = _straight("cylinder")
    o, d = _rays(4000, 2)
    r = cm.intersect(rec, o, d)
    h = r["hit"]
    assert h.sum() > 500
    a = np.array([1.0, 0.0, 0.0])
    dn = d[h] / np.linalg.norm(d[h], axis=1, keepdims=True)
    flat = dn - (dn @ a)[:, None] * a
    flat /= np.linalg.norm(flat, axis=1, keepdims=True)
    side = np.cross(a, flat)
    theta = np.radians(-90.0 + 180.0 * r["v"][h])
    n = r["n"][h]
    np.testing.assert_allclose(n @ a, 0, atol=1e-12)
    np.testing.assert_allclose((n * flat).sum(-1), np.cos(theta), atol=1e-12)
    along_side = (n * side).sum(-1)
    np.testing.assert_allclose(np.abs(along_side), np.abs(np.sin(theta)), atol=1e-12)
    big = np.abs(np.sin(theta)) > 1e-6
    turn = np.sign(along_side[big] * np.sin(theta[big]))
    assert (turn == turn[0]).all()
    # the flat type's own normal is `flat`
    rf = cm.intersect(_straight("flat"), o, d)
    np.testing.assert_allclose(rf["n"][h], flat, atol=1e-12)


def test_ribbon_with_equal_normals_scales_the_width():
    nrm = np.array([0.0, 0.3, 1.0])
    rec = _straight("ribbon", normals=[nrm, nrm])
    o, d = _rays(6000, 3)
    r = cm.intersect(rec, o, d)
    s, t, gap = _line_line(o, d)
    scale = np.abs((d / np.linalg.norm(d, axis=1, keepdims=True)) @ (nrm / np.linalg.norm(nrm)))
    want = (gap <= W * scale / 2) & (s >= 0) & (s <= L) & (t >= 0)
    clear = (np.abs(gap - W * scale / 2) > 1e-7) & (np.abs(s) > 1e-6) & (np.abs(s - L) > 1e-6)
    np.testing.assert_array_equal(r["hit"][clear], want[clear])
    h = r["hit"] & clear
    assert h.sum() > 300 and np.isfinite(r["v"][h]).all()
    np.testing.assert_allclose(r["width"][h], W * scale[h], rtol=1e-6)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: "-".join(c))
def test_hit_points_lie_in_the_world_bounds(case):
    curves, (o, d, t_max), m64, _ = cc.case_model(*case)
    lo, hi = pbrt_hip.curve_world_bounds(curves)
    checked = 0
    for j, rec in enumerate(curves):
        r = cm.intersect(rec, o, d, t_max)
        h = r["hit"]
        checked += int(h.sum())
        # p_error is an object-space bound: through the transform's linear part
        m = np.abs(np.asarray(rec["to_world"], dtype=np.float64).reshape(4, 4)[:3, :3])
        grow = r["p_error"][h][:, None] * m.sum(1)[None, :]
        assert (r["p"][h] >= lo[j] - grow).all() and (r["p"][h] <= hi[j] + grow).all()
        mlo, mhi = cm.world_bound(rec)
        np.testing.assert_allclose(lo[j], mlo, rtol=0, atol=2e-6)
        np.testing.assert_allclose(hi[j], mhi, rtol=0, atol=2e-6)
    assert checked > 500


def test_segments_hit_where_the_unsplit_curve_hits():
    """Segments and the unsplit curve refine the same cubic, each until its leaves are flat to within eps = w_max / 20. Away from
    the acceptance boundary (a twentieth of hit_width here) they agree about the hit. Their leaves differ, so u may differ by up
    to two of the finer leaves, v by the two flatness errors over the smallest width, and the two hit points, both on the ray and
    within w_max / 2 of the curve points at their u, lie no further apart than the curve runs between the two u (its speed is at
    most three times the longest leg of the control polygon) plus w_max."""
    whole = scenes.curve(cc.BENT, 0.05, 0.02, type="flat", split_depth=0)
    parts = scenes.curve(cc.BENT, 0.05, 0.02, type="flat", split_depth=2)
    o, d, t_max = cc.case_rays("flat", "bent", "rigid")
    m = cc.transform("rigid")
    mi = np.linalg.inv(m)
    o, d = o @ mi[:3, :3].T + mi[:3, 3], d @ mi[:3, :3].T  # the case's rays, in the curve's own space
    a = cm.intersect_many(whole, o, d, t_max)
    b = cm.intersect_many(parts, o, d, t_max)
    depth = int(cm.intersect(whole[0], o, d, t_max)["depth"].max())
    assert depth >= 2 and cm.intersect(parts[0], o, d, t_max)["depth"].max() >= 1
    keep = (a["margin"] >= 0.05) & (b["margin"] >= 0.05)
    assert keep.mean() > 0.8 and a["hit"][keep].mean() > 0.2
    np.testing.assert_array_equal(a["hit"][keep], b["hit"][keep])
    h = keep & a["hit"]
    du = np.abs(a["u"][h] - b["u"][h])
    assert du.max() < 2.0 / (1 << depth)
    assert np.abs(a["v"][h] - b["v"][h]).max() < 2 * (0.05 / 20) / 0.02
    speed = 3 * np.linalg.norm(np.diff(cc.BENT, axis=0), axis=1).max()
    assert (np.abs(a["t"][h] - b["t"][h]) * np.linalg.norm(d[h], axis=1) <= speed * du + 0.05).all()


def test_a_bent_curve_is_refined():
    """max_depth = clamp(Log2(sqrt2 * 6 L0 / (8 eps)) / 2, 0, 10) with pbrt-v3's integer Log2; the reference's closure returns
    0 or 1 there, which halves to depth 0 and tests a bent curve as one straight segment"""
    assert [int(cm.log2_int(v)) for v in (0.5, 1.0, 1.4, 1.6, 2.0, 3.0, 93.0, 1024.0)] == [0, 0, 0, 1, 1, 2, 6, 10]
    assert [int(cm.max_depth_of(v)) for v in (2.9, 3.1, 11.9, 12.1, 93.0, 930.0, 1e9)] == [0, 1, 1, 2, 3, 5, 10]
    rec = scenes.curve(cc.BENT, 0.05, 0.02, split_depth=0)[0]
    o, d, t_max = cc.case_rays("flat", "bent", "rigid")
    r = cm.intersect(rec, o, d, t_max)
    assert r["depth"].min() > 0
    # the straight chord of the bent curve is a different shape: with depth 0 rays through the bend's belly would miss
    chord = rec.copy()
    chord["cp"] = np.linspace(cc.BENT[0], cc.BENT[3], 4)
    assert (r["hit"] != cm.intersect(chord, o, d, t_max)["hit"]).mean() > 0.02


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: "-".join(c))
def test_cases_leave_out_few_rays_and_hit_often(case):
    _, _, m64, m32 = cc.case_model(*case)
    assert (m64["margin"] < cc.MARGIN).mean() <= cc.MAX_LEFT_OUT
    assert 0.1 < m64["hit"].mean() < 0.9
    keep = m64["margin"] >= cc.MARGIN
    np.testing.assert_array_equal(m32["hit"][keep], m64["hit"][keep])
    sp = cc.case_spread(*case)
    assert sp["t"] < 1e-4 and sp["u"] < 1e-4 and sp["v"] < 1e-2, sp


@pytest.mark.parametrize("case", cc.EDGE_CASES, ids=lambda c: "-".join(c))
def test_edge_cases_are_decided_by_the_model(case):
    """what test_gpu_curve_edges.py relies on: a margin among EDGE_MARGINS at which the float32 run gives the float64 run's
    verdict on every kept ray, few rays left out, hits and misses both present (but where the case is built to have one of
    them only), the refinement depth the case is there for, finite records, and each case's own property"""
    name, kind = case
    curves, (o, d, t_max), m64, m32, margin = cc.edge_model(*case)
    _, depth_wanted, _ = cc.EDGE_NAMES[name]
    assert margin in cc.EDGE_MARGINS, "no margin decides the case"
    by_margin = m64["margin"] >= margin
    np.testing.assert_array_equal(m32["hit"][by_margin], m64["hit"][by_margin])
    keep, dt = cc.edge_keep(*case)   # the device's origin push takes out a few more
    print("-".join(case), "origin push dt up to %.2e, takes out %.4f of the rays" % (dt.max(), (by_margin & ~keep).mean()))
    depth = max(int(cm.intersect(rec, o, d, t_max)["depth"].max()) for rec in curves)
    sp = cc.edge_spread(*case)
    print("-".join(case), "margin %g left out %.4f hits %.3f depth %d spread t %.2e u %.2e v %.2e" % (
        margin, 1 - keep.mean(), m64["hit"].mean(), depth, sp["t"], sp["u"], sp["v"]))
    assert 1 - keep.mean() <= cc.EDGE_MAX_LEFT_OUT[margin]
    for k in ("t", "u", "v"):
        assert np.isfinite(m64[k][m64["hit"]]).all() and np.isfinite(m32[k][m32["hit"]]).all() and np.isfinite(sp[k])
    if depth_wanted is not None:
        assert depth == depth_wanted
    if name == "parallel_exact":
        assert not m64["hit"].any() and not m32["hit"].any()
    elif name in ("loop", "loop_tmax"):   # chords of the curve: all but the edge-on ribbon's hit
        assert m64["hit"].mean() > 0.5
    else:
        assert 0.1 < m64["hit"].mean() < 0.9
    if name == "taper":   # rays aimed past the tip of zero width (u > 1 by up to 0.05) are there, and hits end before it
        assert m64["u"][m64["hit"]].max() < 1.0
    if name == "loop":
        crossings = sum((cm.intersect(rec, o, d)["hit"]).astype(int) for rec in curves)
        share = (crossings[keep] >= 2).mean()
        print("  rays hit on two or more of the %d records: %.3f" % (len(curves), share))
        assert len(curves) == 8 and share >= 0.5
    if name == "loop_tmax":   # the finite t_max lies past the first crossing: the same hit as without it
        stopped = np.isfinite(t_max)
        free = cm.intersect_many(curves, o, d)
        assert stopped.mean() > 0.5
        np.testing.assert_array_equal(m64["hit"][stopped & keep], free["hit"][stopped & keep])
        np.testing.assert_array_equal(m64["t"][stopped & keep], free["t"][stopped & keep])
    if name == "parallel_chord":   # d along the chord to float32's rounding: the float64 model finds a residue, never zero
        cp = curves[0]["cp"].astype(np.float64)
        dx = np.linalg.norm(np.cross(d.astype(np.float64), cp[3] - cp[0]), axis=1)
        assert (dx > 0).all() and (dx < 1e-6 * np.linalg.norm(d, axis=1) * np.linalg.norm(cp[3] - cp[0])).all()


@pytest.mark.parametrize("kind", cc.TYPES)
def test_the_orientation_test_can_fail(kind):
    """test_gpu_curve_shading.py holds kCurveFlipNormal with a rough-glass row under a point light. Here: with the normal
    reversed, the value that test expects moves by more than ten times its tolerance on at least half of the rays it keeps, for
    every orientation and both lights; and with the tangents turned by 90 degrees the anisotropic metal row's does likewise."""
    import bxdf_model as bm
    import microfacet_model as mm
    glass = bm.rough_glass(cc.GLASS["kr"], cc.GLASS["kt"], cc.GLASS["eta"], cc.GLASS["roughness"])
    metal = mm.Material.metal(cc.METAL["eta"], cc.METAL["k"], cc.METAL["u_roughness"], cc.METAL["v_roughness"])
    for xform, reverse in cc.ORIENTATIONS:
        _, (_, d), _, surf, lights = cc.orient_case(kind, xform, reverse)
        for light in lights:
            keep, clear = cc.orient_kept(kind, xform, reverse, light)
            assert len(keep) >= 128 and clear.mean() > 0.9
            f = lambda wo, wi: bm.bsdf_f(glass, wo, wi)
            want = cc.point_light_radiance(surf, keep, d, lights[light], cc.ORIENT_INTENSITY, f)
            flipped = cc.point_light_radiance(surf, keep, d, lights[light], cc.ORIENT_INTENSITY, f, flip=True)
            moved = (np.abs(flipped - want) > 10 * cc.GLOSSY_RTOL * np.abs(want)).any(-1)
            print(f"{kind} {xform} reverse {int(reverse)} light {light}: kept {len(keep)}, moved by a reversed normal {moved.mean():.3f}")
            assert moved.mean() >= 0.5
        if xform == "scaled":
            keep, _ = cc.orient_kept(kind, xform, reverse, "front")
            g = lambda wo, wi: mm.bsdf_f(metal, wo, wi)
            want = cc.point_light_radiance(surf, keep, d, lights["front"], cc.ORIENT_INTENSITY, g)
            turned = cc.point_light_radiance(surf, keep, d, lights["front"], cc.ORIENT_INTENSITY, g, turn=True)
            moved = (np.abs(turned - want) > 10 * cc.GLOSSY_RTOL * np.abs(want)).any(-1)
            print(f"{kind} {xform} metal: moved by a frame turned by 90 degrees {moved.mean():.3f}")
            assert moved.mean() >= 0.5


def test_record_layout_and_symbols(tmp_path):
    d = scenes.CURVE_DTYPE
    fields = ("type", "reverse_orientation", "material", "cp", "width0", "width1", "u_min", "u_max", "n0", "n1", "to_world", "to_object")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_hip.h"\nint main(void) { printf("%zu ' + "%zu " * len(fields) +
                   '%d %d %d\\n", sizeof(PbrtCurve), ' + ", ".join(f"offsetof(PbrtCurve, {f})" for f in fields) +
                   ', (int)PBRT_CURVE_FLAT, (int)PBRT_CURVE_CYLINDER, (int)PBRT_CURVE_RIBBON); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:-3] == [d.itemsize] + [d.fields[k][1] for k in fields] == [228, 0, 4, 8, 12, 60, 64, 68, 72, 76, 88, 100, 164]
    assert got[-3:] == [scenes.CURVE_FLAT, scenes.CURVE_CYLINDER, scenes.CURVE_RIBBON] == [0, 1, 2]
    lib = ctypes.CDLL(pbrt_hip.LIB_PATH)
    for name in ("pbrt_hip_curve_world_bounds", "pbrt_hip_scene_create_with_curves"):
        assert hasattr(lib, name) and name in pbrt_hip.EXPORTS, name


def test_curve_helper_makes_the_segments_of_create_curve_shape():
    rec = scenes.curve(cc.BENT, 0.05, 0.02, type="cylinder", to_world=cc.transform("scaled"), material=3, split_depth=3)
    assert rec.shape == (8,) and rec.dtype == scenes.CURVE_DTYPE
    np.testing.assert_array_equal(rec["u_min"], np.arange(8, dtype=np.float32) / 8)
    np.testing.assert_array_equal(rec["u_max"], np.arange(1, 9, dtype=np.float32) / 8)
    assert (rec["type"] == scenes.CURVE_CYLINDER).all() and (rec["material"] == 3).all()
    assert (rec["cp"] == cc.BENT.astype(np.float32)).all() and (rec["width0"] == np.float32(0.05)).all()
    prod = rec["to_world"][0].reshape(4, 4).astype(np.float64) @ rec["to_object"][0].reshape(4, 4).astype(np.float64)
    np.testing.assert_allclose(prod, np.eye(4), atol=1e-6)
    both = scenes.curves(rec, scenes.curve(cc.STRAIGHT, 0.1, 0.1, split_depth=0))
    assert both.shape == (9,) and scenes.curves().shape == (0,)


def test_curve_world_bounds_refuses_bad_arguments():
    rec = scenes.curve(cc.STRAIGHT, 0.1, 0.1, split_depth=0)
    out = np.zeros(6, np.float32)
    f = pbrt_hip.lib().pbrt_hip_curve_world_bounds
    assert f(rec.ctypes.data, 1, out.ctypes.data) == 0
    np.testing.assert_allclose(out, [-0.05, -0.05, -0.05, 1.25, 0.05, 0.05], atol=1e-7)
    assert f(rec.ctypes.data, -1, out.ctypes.data) != 0
    assert f(None, 1, out.ctypes.data) != 0 and f(rec.ctypes.data, 1, None) != 0
    assert f(None, 0, None) == 0
    bad = rec.copy()
    bad["type"] = 3
    with pytest.raises(pbrt_hip.PbrtHipError):
        pbrt_hip.curve_world_bounds(bad)
