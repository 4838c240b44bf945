"""The Curve shape's hit test on the device at the inputs the 18 shared cases never reach (curve_cases.EDGE_CASES): Scene.intersect
and intersect_p against the float64 model of curve_model.py, as test_gpu_curves.py::test_hits_against_the_model does it, and curves
among triangles and quadric shapes in one tree.

Each (case, type) has a margin of its own: the smallest of 1e-3, 0.02 and 0.05 of hit_width at which the model's float32 run
gives its float64 run's verdict on every kept ray. test_curve_model.py asserts that one exists, the share it leaves out, the hit
share and the depths. Each has a tolerance of its own too: SPREAD_FACTOR times its own float32-against-float64 spread of t, u
and v (curve_cases.edge_spread; test_edge_tolerances_are_the_measured_spread prints them all). None of it enters
test_gpu_curves.tolerance().

Two things the model does not do are accounted for beside it (curve_cases.edge_keep, origin_push):
  - the device moves the object-space origin along the ray by dt = |d| . o_err / |d|^2 before the hit test (shape_object_ray)
    and reports t from there: t is compared with the model's t - dt, and a ray is left out where its hit lies within 2 dt of
    its origin or of its t_max. dt is 1e-6 near the world's origin and 1.2e-3 for placed_far, 0.05 of the width there: the
    seven rays of that case on which the device first differed from the model (all starting inside the bound, with hits at
    t = 6e-5..8e-4) are these.
  - v's half of the strip is the sign of a cross product that vanishes near the axis and past a leaf's end. Where its lever
    |side| |v - 0.5| is within v's tolerance, the distance |v - 0.5| is compared and not the half: the float64 model itself
    gives 1 - v there after a move of the origin by two ulps. Compared as they stand, hair-cylinder's v was off by 0.085
    (allowed 0.067) and placed_far-cylinder's by 0.0282 (allowed 0.0271), on one mirrored ray each; by distance 0.008 and 0.004.

As measured on the CPU, flat / cylinder / ribbon (test_curve_model.py prints the figures of the run at hand):

    case              what it reaches                                        depth margin           left out              hits            spread of v
    thin              widths 2e-3 / 1e-3: 128 leaves                             7 1e-3             0.0010/0.0015/0       0.43/0.42/0.26  3.5e-4/2.5e-4/2.1e-3
    hair              widths 1e-4 / 5e-5: 512 leaves, subtrees skipped           9 0.02/1e-3/0.02   0.026/0.0024/0.014    0.44/0.43/0.26  0.012/0.017/0.095
    clamp             width 1.2e-5: the clamp at kCurveMaxDepth, 1024 rays      10 0.02             0.035/-/0.024         0.52/-/0.31     0.021/-/0.58: not compared
    taper             width 0.05 -> 0 (D106), scaled, reversed, 4 records        3 1e-3             0.005/0.003/0.002     0.31/0.30/0.16  7e-5/6e-5/9e-5
    loop              a self-crossing curve in 8 records, chords as rays         2 1e-3             0.006/0.007/0.004     1.0/1.0/0.95    1.2e-5/1.0e-5/3.1e-5
                        (0.84 / 0.82 / 0.64 of the kept rays hit two or more records)
    loop_tmax         half of those rays, t_max between the two crossings        2 1e-3             0.005/0.006/0.005     1.0/1.0/0.95    8e-6/1.0e-5/3.0e-5
    u_range           one record with u_min 0.13, u_max 0.71                     4 1e-3             0.0005                0.26/0.26/0.16  1.1e-5/1.3e-5/1.0e-4
    split3            eight records, each refined to its own depth               2 1e-3             0.004/0.004/0.003     0.44/0.42/0.24  2.3e-5/1.7e-5/4.4e-5
    cp0_is_cp1        coincident end control points: curve_eval's                3 1e-3             0.0015/0.0015/0.0010  0.43/0.43/0.25  1.2e-5/1.6e-5/4.9e-5
    cp2_is_cp3          p3 - p0 fallback                                         3 1e-3             0.003/0.002/0.001     0.43/0.42/0.25  1.8e-5/1.4e-5/3.6e-5
    normals_equal     ribbon: n0 == n1 after normalisation (D103)                4 1e-3             0.0015                0.25            3.9e-5
    normals_square    ribbon: 90 degrees between n0 and n1                       4 1e-3             0.0015                0.24            5.1e-5
    grazing_straight  rays at 0.2-5 degrees to the tangent (the ribbon's         0 1e-3             0.005/0.0005/0        0.37/0.34/0.13  8e-6/7e-6/2.3e-3
    grazing_bent        aimed within 0.3 widths, not 1.5)                        4 1e-3             0.008/0.006/0.003     0.48/0.47/0.48  1.4e-5/2.4e-5/2.1e-4
    parallel_exact    d x (cp3 - cp0) == 0 exactly: no hit, finite records       0 1e-3             0                     0
    parallel_chord    d along the chord up to float32's rounding (the ribbon's   5 1e-3             0.002/0.004/0.001     0.55/0.52/0.19  5e-6/4e-6/6.8e-5
                        aimed within 0.5 widths)
    placed_far        moved by (1000, -800, 600): t spread 5e-4/2e-3/4e-4        4 1e-3/1e-3/0.02   0.006/0.004/0.020     0.42/0.42/0.26  0.047/0.007/0.013
    placed_small      scaled by 1e-3: t spread 2e-9/2e-9/4e-9                    4 1e-3             0.003/0.004/0.003     0.44/0.38/0.24  1.4e-5/1.8e-5/1.1e-4
    placed_large      scaled by 1e3: t spread 2.4e-3/1.6e-3/1.6e-3               4 1e-3             0.0015/0.003/0.002    0.42/0.40/0.25  1.7e-5/1.7e-5/7e-5
(t scales with the placement, and so does its spread: relative to the scale, placed_small's and placed_large's are the rigid
case's 2e-6.)

The issue's comparison of split_depth=3 against split_depth=0 on the device "within the case tolerance" is not made: the float64
model gives 5 (ribbon 16) of 2048 rays another verdict and moves t by up to 3e-2, u by 3e-2 and v by 0.8 between the two, because
a record refines to the flatness of its own part and the two sets of leaves differ. split3 is held against its own model instead.
The clamp's ribbon rays take the fourth seed of its family: with the first, one float32 verdict differs even at 0.05, on a ray that
sees the ribbon edge-on at a width of 6e-7."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

import curve_cases as cc
import curve_model as cm
import quadric_model as qm
from test_gpu_curves import SPREAD_FACTOR, as_rays, curve_scene, tolerance
from test_gpu_shapes import T_TOL

pytestmark = pytest.mark.gpu


def edge_tolerance(case):
    """SPREAD_FACTOR times the case's own float32-against-float64 spread (computed once per case, on the CPU)"""
    spread = cc.edge_spread(*case)
    return spread, {k: SPREAD_FACTOR * spread[k] for k in spread}


def test_edge_tolerances_are_the_measured_spread():
    for case in cc.EDGE_CASES:
        spread, tol = edge_tolerance(case)
        print("%-26s margin %-5g spread t %.2e u %.2e v %.2e   tolerance t %.2e u %.2e v %.2e" % (
            "-".join(case), cc.edge_model(*case)[4], spread["t"], spread["u"], spread["v"], tol["t"], tol["u"], tol["v"]))
        assert all(np.isfinite(v) for v in tol.values())


@pytest.mark.parametrize("case", cc.EDGE_CASES, ids=lambda c: "-".join(c))
def test_edge_hits_against_the_model(hip_ctx, case):
    name, kind = case
    curves, (o, d, t_max), m64, _, margin = cc.edge_model(*case)
    _, _, compare_v = cc.EDGE_NAMES[name]
    spread, tol = edge_tolerance(case)
    keep, dt = cc.edge_keep(*case)
    g = pbrt_hip.Scene(hip_ctx, curve_scene(curves))
    rays = as_rays(o, d, t_max)
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    g.close()
    dev_hit = hits["prim_id"] >= 1          # curve j is primitive n_tris + j
    assert ((hits["prim_id"] >= -1) & (hits["prim_id"] <= len(curves))).all()
    for f in ("t", "b0", "b1", "b2"):
        assert not np.isnan(hits[f]).any() and np.isfinite(hits[f][dev_hit]).all(), f
    both = keep & dev_hit & m64["hit"]
    # the device reports t from the origin it moved along the ray by dt (curve_cases.origin_push)
    want = dict(t=m64["t"] - dt, u=m64["u"], v=m64["v"])
    err = {k: np.abs(hits[f][both].astype(np.float64) - want[k][both]) for k, f in (("t", "t"), ("u", "b0"), ("v", "b1"))}
    # v's half of the strip is the sign of a cross product across the ray: the offset of the curve point (|v - 0.5| widths long)
    # against the tangent. Where that product's lever, |side| |v - 0.5|, is within v's own tolerance (near the axis, and past a
    # leaf's end, where the offset runs along the tangent), the half is no decision of float32's, and the float64 model itself
    # gives 1 - v after a move of the origin by an ulp or two: there the distance from the axis is compared, not the half.
    no_side = np.abs(m64["side"][both]) * np.abs(m64["v"][both] - 0.5) <= tol["v"]
    err["v"] = np.where(no_side, np.abs(np.abs(hits["b1"][both].astype(np.float64) - 0.5) - np.abs(m64["v"][both] - 0.5)), err["v"])
    worst = {k: (e.max() if len(e) else 0.0) for k, e in err.items()}
    print("-".join(case), "margin %g kept %.4f hits %.3f spread t %.2e u %.2e v %.2e worst t %.2e u %.2e v %.2e (allowed %.2e %.2e %.2e)%s" % (
        margin, keep.mean(), m64["hit"].mean(), spread["t"], spread["u"], spread["v"], worst["t"], worst["u"], worst["v"],
        tol["t"], tol["u"], tol["v"], "" if compare_v else " v not compared"), "v's half undecided on %.4f of the hits" % (no_side.mean() if len(no_side) else 0.0))
    assert np.array_equal(dev_hit[keep], m64["hit"][keep]), np.flatnonzero(keep & (dev_hit != m64["hit"]))[:5]
    assert np.array_equal(hits["prim_id"][both] - 1, m64["prim"][both])
    assert (hits["b2"][dev_hit] == 0).all()
    if name == "parallel_exact":
        assert not dev_hit.any() and not anyhit.any()
    else:
        assert both.sum() > 150
    if name == "taper":   # past the tip of zero width: no hit
        assert hits["b0"][dev_hit].max() < 1.0
    # the clamp's v is not compared: at a width of 1.2e-5 the float32 rounding of the ray-space position is about 1 % of the width,
    # and the model's own float32 v is off by a fifth to a half of the strip
    for k in ("t", "u", "v") if compare_v else ("t", "u"):
        assert worst[k] <= tol[k], (k, worst[k], tol[k])
    assert np.array_equal(anyhit.astype(bool), dev_hit)


# ---------------------------------------------------------------------------------------------------------------------
# curves among triangles and quadric shapes
# ---------------------------------------------------------------------------------------------------------------------
def _moller_trumbore(positions, indices, o, d):
    """float64: (t, index) of the nearest triangle hit per ray, inf / -1 without one, the second nearest t, and whether the ray
    passes some triangle's plane within 1e-4 (in barycentric units) of one of its edges, where float32 may decide otherwise"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    best, which, second, near = np.full(len(o), np.inf), np.full(len(o), -1), np.full(len(o), np.inf), np.zeros(len(o), bool)
    for j, (a, b, c) in enumerate(positions[indices].astype(np.float64)):
        e1, e2 = b - a, c - a
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            tv = o - a
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1)
            v = (d * qv).sum(-1) / det
            t = (qv @ e2) / det
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        near |= (t > 0) & (np.minimum(np.minimum(u, v), 1 - u - v) > -1e-4) & (np.abs(np.minimum(np.minimum(u, v), 1 - u - v)) < 1e-4)
        t = np.where(ok, t, np.inf)
        second = np.minimum(second, np.maximum(t, best))
        better = t < best
        best, which = np.where(better, t, best), np.where(better, j, which)
    return best, which, second, near


def test_curves_among_triangles_and_quadric_shapes(hip_ctx):
    """32 triangles, 6 quadric shapes and 32 curves of all three types in one box and one tree: the leaf dispatch between a
    shape's row (>= 0) and a curve's (~row < 0). The nearest of the three models' hits, primitive for primitive."""
    rng = np.random.default_rng(123)
    corner = rng.uniform(-0.6, 0.6, (32, 3))
    positions = (corner[:, None, :] + np.concatenate([np.zeros((32, 1, 3)), rng.uniform(-0.35, 0.35, (32, 2, 3))], axis=1)).reshape(-1, 3).astype(np.float32)
    indices = np.arange(96, dtype=np.int32).reshape(32, 3)

    def placed(scale=(1.0, 1.0, 1.0)):
        m = np.eye(4)
        m[:3, :3] = cc._rotation(rng.normal(size=3), rng.uniform(0, 180)) @ np.diag(scale)
        m[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        return m

    shapes = scenes.shapes(scenes.sphere_shape(0.25, to_world=placed()), scenes.disk(0.0, 0.3, to_world=placed()),
                           scenes.cylinder(0.12, -0.3, 0.3, to_world=placed()), scenes.sphere_shape(0.2, to_world=placed((1.6, 0.7, 1.0))),
                           scenes.cylinder(0.1, -0.25, 0.25, to_world=placed((0.8, 1.5, 1.2))), scenes.disk(0.0, 0.25, 0.08, to_world=placed()))
    recs = []
    for j in range(32):
        cp = rng.uniform(-0.5, 0.5, 3) + np.cumsum(np.vstack([np.zeros(3), rng.uniform(-0.4, 0.4, (3, 3))]), axis=0)
        kind = cc.TYPES[j % 3]
        recs.append(scenes.curve(cp, rng.uniform(0.06, 0.12), rng.uniform(0.03, 0.08), type=kind,
                                 normals=rng.normal(size=(2, 3)) if kind == "ribbon" else None, split_depth=0))
    curves = scenes.curves(*recs)
    n = 8192
    target = rng.uniform(-0.6, 0.6, (n, 3))
    away = cc._unit(rng, n)
    # origins near the box: the band the quadric model calls `near` about a silhouette grows with the square of the distance
    o = (target + 1.0 * away).astype(np.float32)
    d = (-away * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)

    t_tol = tolerance()["t"]
    t_tri, i_tri, t_tri2, tri_near = _moller_trumbore(positions, indices, o, d)
    q_shapes = [qm.from_record(r) for r in shapes]
    q_prim, t_q, q_near = qm.intersect_scene(q_shapes, o, d)
    mc = cm.intersect_many(curves, o, d)
    t_c = np.where(mc["hit"], mc["t"], np.inf)
    # the runner-up inside the curves and inside the shapes
    t_c2, t_q2 = np.full(n, np.inf), np.full(n, np.inf)
    for j, rec in enumerate(curves):
        r = cm.intersect(rec, o, d)
        t_c2 = np.where(r["hit"] & (mc["prim"] != j), np.minimum(t_c2, r["t"]), t_c2)
    for j, s in enumerate(q_shapes):
        r = qm.intersect(s, o, d)
        t_q2 = np.where(r["hit"] & (q_prim != j), np.minimum(t_q2, r["t"]), t_q2)
    cand = np.sort(np.stack([t_tri, t_tri2, t_q, t_q2, t_c, t_c2]), axis=0)
    nearest = np.stack([t_tri, t_q, t_c]).argmin(0)   # 0 a triangle, 1 a shape, 2 a curve
    any_hit = np.isfinite(cand[0])
    with np.errstate(invalid="ignore"):
        apart = ~np.isfinite(cand[1]) | (cand[1] - cand[0] > 10 * t_tol)
    print("left out: curves' margin %.4f, the quadric model's near %.4f, a triangle's edge %.4f, two candidates close %.4f" % (
        (mc["margin"] < cc.MARGIN).mean(), q_near.mean(), tri_near.mean(), 1 - apart.mean()))
    assert q_near.mean() <= 0.01   # the cap test_gpu_shapes.py holds the quadric model's exclusions to
    keep = (mc["margin"] >= cc.MARGIN) & ~q_near & ~tri_near & apart
    want_prim = np.where(~any_hit, -1, np.where(nearest == 0, i_tri, np.where(nearest == 1, 32 + q_prim, 32 + len(shapes) + mc["prim"])))
    share = [float((nearest == k)[keep & any_hit].mean()) for k in range(3)]
    print("kept %.3f, hit %.3f, nearest: triangles %.3f shapes %.3f curves %.3f" % (keep.mean(), any_hit[keep].mean(), *share))
    assert keep.mean() > 0.8 and min(share) >= 0.05

    sc = curve_scene(curves, extra=dict(positions=positions, indices=indices, tri_material=np.zeros(32, np.int32), tri_light=np.full(32, -1, np.int32)),
                     shapes=shapes)
    g = pbrt_hip.Scene(hip_ctx, sc, max_prims_in_node=4)
    rays = as_rays(o, d)
    hits, anyhit = g.intersect(rays), g.intersect_p(rays)
    assert len(g.nodes) > 16
    g.close()
    dev_hit = hits["prim_id"] >= 0
    assert np.array_equal(dev_hit[keep], any_hit[keep])
    assert np.array_equal(hits["prim_id"][keep], want_prim[keep]), np.flatnonzero(keep & (hits["prim_id"] != want_prim))[:5]
    both = keep & any_hit
    err = np.abs(hits["t"][both] - cand[0][both])
    on_curve = nearest[both] == 2
    # a curve's t within the 18 cases' tolerance; a shape's and a triangle's within test_gpu_shapes.py's T_TOL, relative to t or,
    # where the origin lies nearer to the hit than to the world's origin, to the time the ray takes to travel |o| (the rounding
    # of o's products is what t inherits: quadric_model.py's t_scale)
    scale = np.maximum(cand[0], np.linalg.norm(o, axis=1) / np.linalg.norm(d, axis=1))[both]
    allowed = np.where(on_curve, t_tol, T_TOL * scale)
    print("worst t error %.2e on curves (allowed %.2e), worst relative %.2e elsewhere (allowed %.2e)" % (
        err[on_curve].max(), t_tol, (err / scale)[~on_curve].max(), T_TOL))
    assert (err <= allowed).all()
    assert np.array_equal(anyhit.astype(bool), dev_hit)
