"""numpy model of the Curve shape (pbrt-v3's Curve::Intersect with the rules of DESIGN.md D98-D106), vectorised over rays.

One PbrtCurve record (scenes.CURVE_DTYPE) against a batch of world-space rays, in float64 or, with dtype=np.float32, in the
kernels' precision. The algorithm is the one csrc/shapes_curve.h walks: the ray to object space, the segment's control points
(blossoms of the whole curve's) to the ray's frame, max_depth from pbrt-v3's integer Log2, every leaf at that depth whose
ancestors' boxes pass the culling tests, the leaf test of curve.rs:196-243, and inside one curve the hit with the smallest t
(ties to the smaller u). Not modelled: the 3-ulp push of the object-space origin along the ray (Ray::from, geometry.rs:1089-1093),
which moves t by about 1e-7 of the origin's distance.

intersect() returns a dict of arrays: hit, t, u, v, width (hit_width), p / n / dpdu / dpdv (world space), p_error (2 hit_width),
depth (max_depth of the ray), side (the sine of the angle between the curve's tangent and the offset of the curve point from the
ray, both across the ray: the sign of it picks v's half of the strip, so that where |side| |v - 0.5| is within the rounding of the
position, in widths, v may come out as 1 - v) and margin: how far the ray is from the nearest decision of the algorithm that would change the
answer (an edge test, the width test, the z range, the depth's threshold), in units of hit_width; a ray with a small margin is
one where float32 and float64 may legitimately disagree about hit or miss.
"""
import numpy as np


def _lerp(t, a, b):
    return (1 - t) * a + t * b


def _blossom(p, u0, u1, u2):
    a = [_lerp(u0, p[i], p[i + 1]) for i in range(3)]
    b = [_lerp(u1, a[i], a[i + 1]) for i in range(2)]
    return _lerp(u2, b[0], b[1])


def _eval(p, u):
    """EvalBezier of pbrt-v3: the point and the derivative (3 (b1 - b0), or p3 - p0 where that vanishes). u: (R, 1)."""
    a = [_lerp(u, p[i], p[i + 1]) for i in range(3)]
    b = [_lerp(u, a[i], a[i + 1]) for i in range(2)]
    db = b[1] - b[0]
    zero = (db * db).sum(-1, keepdims=True) > 0
    return _lerp(u, b[0], b[1]), np.where(zero, 3 * db, p[3] - p[0])


def log2_int(v):
    """pbrt-v3's integer Log2 of a float32: exponent, plus one from a mantissa of 1.5 up; 0 below 1"""
    v32 = np.asarray(v, dtype=np.float32)
    bits = v32.view(np.uint32).astype(np.int64)
    r = (bits >> 23) - 127 + ((bits >> 22) & 1)
    return np.where(v32 < 1, 0, r)


def max_depth_of(arg):
    return np.clip(log2_int(arg) // 2, 0, 10)


def segment_points(rec, dtype=np.float64):
    cp = np.asarray(rec["cp"], dtype=dtype).reshape(4, 3)
    u0, u1 = dtype(rec["u_min"]), dtype(rec["u_max"])
    return [_blossom(cp, a, b, c) for a, b, c in ((u0, u0, u0), (u0, u0, u1), (u0, u1, u1), (u1, u1, u1))]


def object_bound(rec):
    s = np.array(segment_points(rec))
    w0, w1 = float(rec["width0"]), float(rec["width1"])
    grow = 0.5 * max(_lerp(float(rec["u_min"]), w0, w1), _lerp(float(rec["u_max"]), w0, w1))
    return s.min(0) - grow, s.max(0) + grow


def world_bound(rec):
    lo, hi = object_bound(rec)
    m = np.asarray(rec["to_world"], dtype=np.float64).reshape(4, 4)
    corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)])
    w = corners @ m[:3, :3].T + m[:3, 3]
    return w.min(0), w.max(0)


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _culled(pts, half_width, z_max):
    """pts: four (R, 3) arrays; True where the box grown by half_width misses x = y = 0, 0 <= z <= z_max"""
    p = np.stack(pts)
    hi, lo = p.max(0), p.min(0)
    out = (hi[:, 1] + half_width < 0) | (lo[:, 1] - half_width > 0)
    out |= (hi[:, 0] + half_width < 0) | (lo[:, 0] - half_width > 0)
    out |= (hi[:, 2] + half_width < 0) | (lo[:, 2] - half_width > z_max)
    return out


def intersect(rec, o, d, t_max=np.inf, dtype=np.float64):
    rec = np.asarray(rec).reshape(-1)[0]
    f = dtype
    o = np.asarray(o, dtype=f).reshape(-1, 3)
    d = np.asarray(d, dtype=f).reshape(-1, 3)
    R = len(o)
    t_max = np.broadcast_to(np.asarray(t_max, dtype=f), (R,)).copy()
    m = np.asarray(rec["to_world"], dtype=f).reshape(4, 4)
    mi = np.asarray(rec["to_object"], dtype=f).reshape(4, 4)
    oo = o @ mi[:3, :3].T + mi[:3, 3]
    od = d @ mi[:3, :3].T
    kind = int(rec["type"])
    w0, w1 = f(rec["width0"]), f(rec["width1"])
    u_min, u_max = f(rec["u_min"]), f(rec["u_max"])
    cp_all = np.asarray(rec["cp"], dtype=f).reshape(4, 3)
    seg = segment_points(rec, f)
    # object_to_ray = look_at(o, o + d, dx)
    dx = np.cross(od, (seg[3] - seg[0])[None, :])
    degenerate = (dx * dx).sum(-1) == 0
    if degenerate.any():
        v = od[degenerate]
        alt = np.where((np.abs(v[:, :1]) > np.abs(v[:, 1:2])), np.stack([-v[:, 2], 0 * v[:, 0], v[:, 0]], -1),
                       np.stack([0 * v[:, 0], v[:, 2], -v[:, 1]], -1))
        dx[degenerate] = alt
    ray_length = np.sqrt((od * od).sum(-1))
    dirv = od / ray_length[:, None]
    right = _normalize(np.cross(_normalize(dx), dirv))
    up = np.cross(dirv, right)

    def to_ray(p):
        e = p - oo
        return np.stack([(right * e).sum(-1), (up * e).sum(-1), (dirv * e).sum(-1)], -1)

    s = [to_ray(p[None, :]) for p in seg]
    z_max = ray_length * t_max
    seg_width = max(_lerp(u_min, w0, w1), _lerp(u_max, w0, w1))
    alive = ~_culled(s, f(0.5) * seg_width, z_max)
    l0 = np.maximum(np.abs(s[0] - 2 * s[1] + s[2]).max(-1), np.abs(s[1] - 2 * s[2] + s[3]).max(-1))
    eps = max(w0, w1) * f(0.05)  # width / 20, as pbrt-v3 has it
    arg = (f(1.41421356237) * f(6.0) * l0 / (f(8.0) * eps)).astype(f)
    depth = max_depth_of(arg)
    # the depth's decision: it changes where arg crosses 3 * 4^k
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.round(np.log(np.maximum(arg.astype(np.float64), 1e-30) / 3.0) / np.log(4.0))
        depth_margin = np.abs(arg.astype(np.float64) / (3.0 * 4.0 ** np.clip(k, 0, 10)) - 1.0)

    out = dict(hit=np.zeros(R, bool), t=np.full(R, np.inf, f), u=np.zeros(R, f), v=np.zeros(R, f), width=np.zeros(R, f), side=np.zeros(R, f),
               n_hit=np.zeros((R, 3), f), depth=depth.astype(np.int32), margin=np.full(R, np.inf))
    out["margin"] = np.where(depth_margin < 1e-4, 0.0, np.inf)
    if kind == 2:
        n0 = _normalize(np.asarray(rec["n0"], dtype=np.float64)).astype(f)
        n1 = _normalize(np.asarray(rec["n1"], dtype=np.float64)).astype(f)
        angle = f(np.arccos(np.clip(np.dot(n0.astype(np.float64), n1.astype(np.float64)), 0.0, 1.0)))
        if np.array_equal(n0, n1):
            angle = f(0.0)
    for D in np.unique(depth[alive]):
        idx = np.nonzero(alive & (depth == D))[0]
        sp = [p[idx] for p in s]
        zm, rl, dd = z_max[idx], ray_length[idx], od[idx]
        n_leaf = 1 << int(D)
        cull_cache = {}

        def node(j, span):
            t0, t1 = f(j * span) / f(n_leaf), f((j + 1) * span) / f(n_leaf)
            pts = [_blossom(sp, a, b, c) for a, b, c in ((t0, t0, t0), (t0, t0, t1), (t0, t1, t1), (t1, t1, t1))]
            return pts, _lerp(t0, u_min, u_max), _lerp(t1, u_min, u_max)

        best_t = np.full(len(idx), np.inf, f)
        got = np.zeros(len(idx), bool)
        res = {k: np.zeros(len(idx), f) for k in ("u", "v", "width", "side")}
        res_n = np.zeros((len(idx), 3), f)
        margin = np.full(len(idx), np.inf)
        for i in range(n_leaf):
            reach = np.ones(len(idx), bool)
            for level in range(1, int(D) + 1):
                span = n_leaf >> level
                j = i // span
                if (level, j) not in cull_cache:
                    pts, a0, a1 = node(j, span)
                    cull_cache[(level, j)] = _culled(pts, f(0.5) * np.maximum(_lerp(a0, w0, w1), _lerp(a1, w0, w1)), zm)
                reach &= ~cull_cache[(level, j)]
            (a, b, c, e), u0, u1 = node(i, 1)
            edge0 = (b[:, 1] - a[:, 1]) * -a[:, 1] + a[:, 0] * (a[:, 0] - b[:, 0])
            edge1 = (c[:, 1] - e[:, 1]) * -e[:, 1] + e[:, 0] * (e[:, 0] - c[:, 0])
            sx, sy = e[:, 0] - a[:, 0], e[:, 1] - a[:, 1]
            denom = sx * sx + sy * sy
            with np.errstate(divide="ignore", invalid="ignore"):
                w = (sx * -a[:, 0] + sy * -a[:, 1]) / denom
                u = np.clip(_lerp(w, u0, u1), u0, u1)
                hw = _lerp(u, w0, w1)
                n_hit = np.zeros((len(idx), 3), f)
                if kind == 2:
                    if angle == 0:
                        n_hit = np.broadcast_to(n0, (len(idx), 3)).astype(f)
                    else:
                        inv = f(1.0) / np.sin(angle)
                        n_hit = (np.sin((1 - u) * angle) * inv)[:, None] * n0 + (np.sin(u * angle) * inv)[:, None] * n1
                    hw = hw * np.abs((n_hit * dd).sum(-1)) / rl
                pc, dpcdw = _eval([a, b, c, e], np.clip(w, 0, 1)[:, None])
                dist2 = pc[:, 0] ** 2 + pc[:, 1] ** 2
                dist = np.sqrt(dist2)
                ok = reach & (edge0 >= 0) & (edge1 >= 0) & (denom != 0) & (hw > 0) & (dist2 <= hw * hw * f(0.25)) & (pc[:, 2] >= 0) & (pc[:, 2] <= zm)
                t = pc[:, 2] / rl
                edge_func = dpcdw[:, 0] * -pc[:, 1] + pc[:, 0] * dpcdw[:, 1]
                v = np.where(edge_func > 0, f(0.5) + dist / hw, f(0.5) - dist / hw)
                side = edge_func / np.sqrt((dpcdw[:, 0] ** 2 + dpcdw[:, 1] ** 2) * dist2)
                # signed margins of the leaf's tests in units of hit_width (positive: passes)
                l_ab = np.sqrt((b[:, 0] - a[:, 0]) ** 2 + (b[:, 1] - a[:, 1]) ** 2)
                l_ce = np.sqrt((c[:, 0] - e[:, 0]) ** 2 + (c[:, 1] - e[:, 1]) ** 2)
                ms = np.stack([edge0 / l_ab, edge1 / l_ce, hw * f(0.5) - dist, pc[:, 2], zm - pc[:, 2]]).astype(np.float64) / hw.astype(np.float64)
                ms = np.where(np.isnan(ms), np.inf, ms)
                neg = ms < 0
                leaf_margin = np.where(neg.any(0), np.where(neg, -ms, 0).max(0), ms.min(0))
                margin = np.where(reach, np.minimum(margin, leaf_margin), margin)
            better = ok & (t < best_t)
            best_t = np.where(better, t, best_t)
            got |= better
            for key, val in (("u", u), ("v", v), ("width", hw), ("side", np.where(np.isfinite(side), side, 0))):
                res[key] = np.where(better, val, res[key])
            res_n = np.where(better[:, None], n_hit, res_n)
        out["hit"][idx] = got
        out["t"][idx] = best_t
        for key in res:
            out[key][idx] = res[key]
        out["n_hit"][idx] = res_n
        out["margin"][idx] = np.minimum(out["margin"][idx], margin)

    # ---- the surface (curve.rs:243-276) ----
    h = out["hit"]
    u, v, hw = out["u"], out["v"], out["width"]
    _, dpdu = _eval([np.broadcast_to(p, (R, 3)) for p in cp_all], u[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == 2:
            dpdv = _normalize(np.cross(out["n_hit"], dpdu)) * hw[:, None]
        else:
            du = np.stack([(right * dpdu).sum(-1), (up * dpdu).sum(-1), (dirv * dpdu).sum(-1)], -1)
            dv = _normalize(np.stack([-du[:, 1], du[:, 0], 0 * du[:, 0]], -1)) * hw[:, None]
            if kind == 1:
                theta = np.radians(-_lerp(v, f(-90.0), f(90.0)))
                ax = _normalize(du)
                cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
                dv = dv * cs + np.cross(ax, dv) * sn + ax * ((ax * dv).sum(-1, keepdims=True) * (1 - cs))
            dpdv = right * dv[:, :1] + up * dv[:, 1:2] + dirv * dv[:, 2:3]
        n = _normalize(np.cross(dpdu, dpdv))
        flip = bool(rec["reverse_orientation"]) != (np.linalg.det(m[:3, :3].astype(np.float64)) < 0)
        if flip:
            n = -n
        p_obj = oo + od * np.where(h, out["t"], 0)[:, None]
        out["p"] = p_obj @ m[:3, :3].T + m[:3, 3]
        out["n"] = _normalize(n @ mi[:3, :3])  # (M^-1)^T n
        out["dpdu"] = dpdu @ m[:3, :3].T
        out["dpdv"] = dpdv @ m[:3, :3].T
    out["p_error"] = 2 * hw
    return out


def intersect_many(recs, o, d, t_max=np.inf, dtype=np.float64):
    """The brute-force aggregate: every record against every ray; the nearest hit, ties to the lower record index.
    Returns (hit, t, record index, u, v, side, margin)."""
    recs = np.asarray(recs).reshape(-1)
    R = len(np.asarray(o).reshape(-1, 3))
    best = dict(hit=np.zeros(R, bool), t=np.full(R, np.inf), prim=np.full(R, -1), u=np.zeros(R), v=np.zeros(R), side=np.zeros(R),
                margin=np.full(R, np.inf))
    for j, rec in enumerate(recs):
        r = intersect(rec, o, d, t_max, dtype)
        better = r["hit"] & (r["t"] < best["t"])
        best["hit"] |= better
        for key in ("t", "u", "v", "side"):
            best[key] = np.where(better, r[key], best[key])
        best["prim"] = np.where(better, j, best["prim"])
        best["margin"] = np.minimum(best["margin"], r["margin"])
    return best
