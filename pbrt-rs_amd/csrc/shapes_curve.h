// shapes_curve.h — Curve: flat, cylinder and ribbon cubic Bezier segments (included at the end of trace.h, behind shapes_quadric.h).
//
// pbrt-v3's Curve::Intersect / recursiveIntersect, of which src/shapes/curve.rs:130-373 is a transcription with slips (DESIGN.md
// D98-D106: the depth, the sign and the extent of the culling tests, eval_bezier's second level, the ribbon's angle). The ray goes
// to object space as for the quadrics (shape_object_ray), the segment's control points to the ray's own frame (look_at from the
// origin along the direction, x / y across it), and the cubic is refined to max_depth = clamp(log2(sqrt2 * 6 L0 / (8 eps)) / 2,
// 0, 10) levels. The reference recurses with seven control points per level; here the 2^max_depth leaves are walked by index:
// a leaf's control points are blossoms of the segment's (the de Casteljau halves of the recursion are those blossoms), and at a
// leaf index that starts subtrees, their boxes are tested coarsest first, so that a subtree the recursion would not enter is
// stepped over whole. Every node the recursion tests is tested once, in the same order, and nothing is kept on a stack.
// Inside one curve the hit with the smallest t is reported, ties to the smaller u (D101); any-hit rays stop at the first.
#pragma once

namespace pb {

constexpr int kCurveFlat = 0, kCurveCylinder = 1, kCurveRibbon = 2;  // PbrtCurveType
constexpr int kCurveTypeMask = 3;
constexpr int kCurveFlipNormal = 4;  // reverse_orientation ^ transform_swaps_handedness (SurfaceInteraction::new)
constexpr int kCurveMaxDepth = 10;

// One row per curve record (DevSceneData::curves). A curve's leaf slot carries kPrimSphere and ~row in the third float4's .x
// (a shape's row is >= 0), so the kernels of scenes without curves never meet one.
struct DevCurve {
    float w2o[12];  // world_to_object rows 0-2
    float o2w[12];  // object_to_world rows 0-2
    float cp[12];   // the whole curve's control points, object space
    float width0, width1, u_min, u_max;
    float n0[3], n1[3];                        // ribbon: normalised
    float normal_angle, inv_sin_normal_angle;  // ribbon: acos(clamp(n0 . n1, 0, 1)) and 1 / sin of it; 0, 0 when n0 == n1 (D103)
    int flags;                                 // type | kCurveFlipNormal
};

struct CurveHit {
    float t, u, v, width;  // width: hit_width, the ribbon's already scaled by |n . d| / |d|
};
// what the surface past the hit test needs of the ray's frame
struct CurveFrame {
    V3 o, d;             // the object-space ray
    V3 right, up, dir;   // rows of object_to_ray's rotation (ray space x, y, z)
    float ray_length;
    V3 n_hit;            // ribbon: the interpolated orientation at the hit
};

PB_DEV float curve_lerp(float t, float a, float b) { return (1.0f - t) * a + t * b; }
PB_DEV V3 curve_lerp3(float t, V3 a, V3 b) { return a * (1.0f - t) + b * t; }
// BlossomBezier (curve.rs:82-90)
PB_DEV V3 curve_blossom(V3 p0, V3 p1, V3 p2, V3 p3, float u0, float u1, float u2) {
    V3 a0 = curve_lerp3(u0, p0, p1), a1 = curve_lerp3(u0, p1, p2), a2 = curve_lerp3(u0, p2, p3);
    V3 b0 = curve_lerp3(u1, a0, a1), b1 = curve_lerp3(u1, a1, a2);
    return curve_lerp3(u2, b0, b1);
}
// EvalBezier of pbrt-v3 (curve.rs:102-119 takes the second level's second point from the wrong row: D102)
PB_DEV V3 curve_eval(V3 p0, V3 p1, V3 p2, V3 p3, float u, V3* deriv) {
    V3 a0 = curve_lerp3(u, p0, p1), a1 = curve_lerp3(u, p1, p2), a2 = curve_lerp3(u, p2, p3);
    V3 b0 = curve_lerp3(u, a0, a1), b1 = curve_lerp3(u, a1, a2);
    V3 db = b1 - b0;
    *deriv = len2(db) > 0.0f ? db * 3.0f : p3 - p0;
    return curve_lerp3(u, b0, b1);
}
// the box of four ray-space control points, grown by half the width, against the ray: x = y = 0, 0 <= z <= z_max
// (pbrt-v3: y, x, then z; max + w/2 < 0 || min - w/2 > 0, on all four points: D99, D100)
PB_DEV bool curve_culled(V3 a, V3 b, V3 c, V3 d, float half_width, float z_max) {
    float hi = fmaxr(fmaxr(a.y, b.y), fmaxr(c.y, d.y)), lo = fminr(fminr(a.y, b.y), fminr(c.y, d.y));
    bool out = hi + half_width < 0.0f || lo - half_width > 0.0f;
    hi = fmaxr(fmaxr(a.x, b.x), fmaxr(c.x, d.x));
    lo = fminr(fminr(a.x, b.x), fminr(c.x, d.x));
    out = out || hi + half_width < 0.0f || lo - half_width > 0.0f;
    hi = fmaxr(fmaxr(a.z, b.z), fmaxr(c.z, d.z));
    lo = fminr(fminr(a.z, b.z), fminr(c.z, d.z));
    return out || hi + half_width < 0.0f || lo - half_width > z_max;
}
// pbrt-v3's integer Log2 of a float (curve.rs:348-359 returns 0 or 1 instead: D98)
PB_DEV int curve_log2(float v) {
    if (v < 1.0f) return 0;
    const uint32_t bits = __builtin_bit_cast(uint32_t, v);
    return (int)(bits >> 23) - 127 + ((bits & (1u << 22)) ? 1 : 0);
}

// Curve::intersect / intersect_p up to the hit record; tmax is the world ray's. any: stop at the first leaf that hits.
PB_DEV bool curve_test(const DevCurve& c, const TravRay& r, float tmax, bool any, CurveHit* hit, CurveFrame* frame) {
    const SphereRay q = shape_object_ray(c.w2o, r);
    const V3 o = V3{q.ox, q.oy, q.oz}, d = V3{q.dx, q.dy, q.dz};
    const float width0 = c.width0, width1 = c.width1, u_min = c.u_min, u_max = c.u_max;
    V3 s0, s1, s2, s3;  // the segment's control points (curve.rs:121-128), then in ray space
    {
        const V3 w0 = V3{c.cp[0], c.cp[1], c.cp[2]}, w1 = V3{c.cp[3], c.cp[4], c.cp[5]}, w2 = V3{c.cp[6], c.cp[7], c.cp[8]},
                 w3 = V3{c.cp[9], c.cp[10], c.cp[11]};
        s0 = curve_blossom(w0, w1, w2, w3, u_min, u_min, u_min);
        s1 = curve_blossom(w0, w1, w2, w3, u_min, u_min, u_max);
        s2 = curve_blossom(w0, w1, w2, w3, u_min, u_max, u_max);
        s3 = curve_blossom(w0, w1, w2, w3, u_max, u_max, u_max);
    }
    // object_to_ray = look_at(o, o + d, dx) with dx across both the ray and the segment's chord (curve.rs:307-311)
    V3 dx = cross(d, s3 - s0);
    if (len2(dx) == 0.0f) {
        V3 dy;
        coordinate_system(d, &dx, &dy);
    }
    const float ray_length = length(d);
    const V3 dir = d / ray_length;
    const V3 right = normalize(cross(normalize(dx), dir));
    const V3 up = cross(dir, right);
    auto to_ray = [&](V3 p) {
        V3 e = p - o;
        return V3{dot(right, e), dot(up, e), dot(dir, e)};
    };
    s0 = to_ray(s0);
    s1 = to_ray(s1);
    s2 = to_ray(s2);
    s3 = to_ray(s3);
    float z_max = ray_length * tmax;
    if (curve_culled(s0, s1, s2, s3, 0.5f * fmaxr(curve_lerp(u_min, width0, width1), curve_lerp(u_max, width0, width1)), z_max)) return false;
    // the refinement depth (pbrt-v3; D98)
    float l0 = 0.0f;
    {
        V3 e0 = vabs(s0 - s1 * 2.0f + s2), e1 = vabs(s1 - s2 * 2.0f + s3);
        l0 = fmaxr(fmaxr(max3(e0.x, e0.y, e0.z), max3(e1.x, e1.y, e1.z)), 0.0f);
    }
    const float eps = fmaxr(width0, width1) * 0.05f;  // width / 20 (pbrt-v3; curve.rs:347 has width / 2: D98)
    int depth = curve_log2(1.41421356237f * 6.0f * l0 / (8.0f * eps)) / 2;
    depth = depth < 0 ? 0 : (depth > kCurveMaxDepth ? kCurveMaxDepth : depth);
    const int n_leaf = 1 << depth;
    const float inv_n = 1.0f / (float)n_leaf;
    const int type = c.flags & kCurveTypeMask;
    bool found = false;
    int i = 0;
    while (i < n_leaf) {
        // the subtrees that start at leaf i, coarsest first (the root was tested above); span = leaves under the node
        int span = i == 0 ? (n_leaf >> 1) : (i & -i);
        span = span < 1 ? 1 : span;
        V3 a, b, cc, dd;
        float u0, u1;
        bool skip;
        for (;;) {
            const float t0 = (float)i * inv_n, t1 = (float)(i + span) * inv_n;
            a = curve_blossom(s0, s1, s2, s3, t0, t0, t0);
            b = curve_blossom(s0, s1, s2, s3, t0, t0, t1);
            cc = curve_blossom(s0, s1, s2, s3, t0, t1, t1);
            dd = curve_blossom(s0, s1, s2, s3, t1, t1, t1);
            u0 = curve_lerp(t0, u_min, u_max);
            u1 = curve_lerp(t1, u_min, u_max);
            skip = depth > 0 && curve_culled(a, b, cc, dd, 0.5f * fmaxr(curve_lerp(u0, width0, width1), curve_lerp(u1, width0, width1)), z_max);
            if (skip || span == 1) break;
            span >>= 1;
        }
        i += span;
        if (skip) continue;
        // ---- the leaf (curve.rs:196-243) ----
        float edge = (b.y - a.y) * -a.y + a.x * (a.x - b.x);
        if (edge < 0.0f) continue;
        edge = (cc.y - dd.y) * -dd.y + dd.x * (dd.x - cc.x);
        if (edge < 0.0f) continue;
        const float sx = dd.x - a.x, sy = dd.y - a.y;
        const float denom = sx * sx + sy * sy;
        if (denom == 0.0f) continue;
        const float w = (sx * -a.x + sy * -a.y) / denom;
        const float u = clampf(curve_lerp(w, u0, u1), u0, u1);
        float hit_width = curve_lerp(u, width0, width1);
        V3 n_hit = V3{0.0f, 0.0f, 0.0f};
        if (type == kCurveRibbon) {
            const V3 n0 = V3{c.n0[0], c.n0[1], c.n0[2]}, n1 = V3{c.n1[0], c.n1[1], c.n1[2]};
            if (c.normal_angle == 0.0f) {
                n_hit = n0;  // n0 == n1: the limit of the weights below (pbrt-v3 divides 0 by 0 there: D103)
            } else {
                const float sin0 = det_sin((1.0f - u) * c.normal_angle) * c.inv_sin_normal_angle;
                const float sin1 = det_sin(u * c.normal_angle) * c.inv_sin_normal_angle;
                n_hit = n0 * sin0 + n1 * sin1;
            }
            hit_width *= absdot(n_hit, d) / ray_length;
        }
        // a width of zero (the tip of a curve that tapers to nothing, a ribbon seen exactly edge-on) has no surface: both sources
        // accept a ray through the axis itself there and divide 0 by 0 for v (D106)
        if (!(hit_width > 0.0f)) continue;
        V3 dpcdw;
        const V3 pc = curve_eval(a, b, cc, dd, clampf(w, 0.0f, 1.0f), &dpcdw);
        const float dist2 = pc.x * pc.x + pc.y * pc.y;
        if (dist2 > hit_width * hit_width * 0.25f) continue;
        if (pc.z < 0.0f || pc.z > z_max) continue;
        const float t = pc.z / ray_length;
        if (found && !(t < hit->t)) continue;  // the nearest leaf hit, ties to the smaller u (D101)
        const float dist = __builtin_sqrtf(dist2);
        const float edge_func = dpcdw.x * -pc.y + pc.x * dpcdw.y;
        hit->t = t;
        hit->u = u;
        hit->v = edge_func > 0.0f ? 0.5f + dist / hit_width : 0.5f - dist / hit_width;
        hit->width = hit_width;
        if (frame) frame->n_hit = n_hit;
        found = true;
        if (any) break;
        z_max = pc.z;  // a later leaf wins only with a smaller t: boxes wholly behind this hit are stepped over
    }
    if (frame) {
        frame->o = o;
        frame->d = d;
        frame->right = right;
        frame->up = up;
        frame->dir = dir;
        frame->ray_length = ray_length;
    }
    return found;
}

}  // namespace pb
