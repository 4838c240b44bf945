// wf_surface.h — SurfaceInteraction from a hit record, shading frames, matte BSDF, distributions, ShadeConsts (part of wavefront.h)
#pragma once
#include "wf_generate_trace.h"

namespace pb {

// ---- shading helpers ----
struct Surf {  // the parts of SurfaceInteraction the path needs
    V3 p, p_error, n, dpdu, wo;
    V3 ns, sdpdu;         // shading.n, shading.dpdu (= n, dpdu without per-vertex normals)
    int material, light;  // light = index or -1
};

PB_DEV void tri_vertices(const DevBVH& bvh, int slot, V3* p0, V3* p1, V3* p2, int* prim, int* mat, int* light) {
    float4 a = bvh.tris[3 * (size_t)slot], b = bvh.tris[3 * (size_t)slot + 1], c = bvh.tris[3 * (size_t)slot + 2];
    *p0 = V3{a.x, a.y, a.z};
    *p1 = V3{a.w, b.x, b.y};
    *p2 = V3{b.z, b.w, c.x};
    *prim = __float_as_int(c.y);
    *mat = __float_as_int(c.z);
    *light = (__float_as_int(c.w) & kPrimLightMask) - 1;
}

// Triangle::intersect past the hit test (triangle.rs:193-316): dpdu from the (default or per-vertex) uvs, the
// geometric normal, and with per-vertex normals the shading frame of :252-312 with
// set_shading_geometry(.., orientation_is_authoritative = true) (interaction.rs:302-316), which also flips
// the geometric normal to the shading normal's side. Outputs: n, shading.n, dpdu, shading.dpdu.
PB_DEV void tri_shading_geometry(const DevBVH& bvh, int slot, V3 p0, V3 p1, V3 p2, float b0, float b1, float b2, V3* n_out,
                                 V3* ns_out, V3* dpdu_out, V3* sdpdu_out) {
    float uv0x = 0.0f, uv0y = 0.0f, uv1x = 1.0f, uv1y = 0.0f, uv2x = 1.0f, uv2y = 1.0f;  // triangle.rs:66-70
    float4 s0 = make_float4(0, 0, 0, 0), s1 = s0, s2 = s0, s3 = s0, s4 = s0;
    if (bvh.tri_shading) {
        const float4* sh = bvh.tri_shading + 6 * (size_t)slot;
        s0 = sh[0];
        s1 = sh[1];
        s2 = sh[2];
        s3 = sh[3];
        s4 = sh[4];
        if (bvh.has_uvs) {
            float4 s5 = sh[5];
            uv0x = s4.z;
            uv0y = s4.w;
            uv1x = s5.x;
            uv1y = s5.y;
            uv2x = s5.z;
            uv2y = s5.w;
        }
    }
    float duv02x = uv0x - uv2x, duv02y = uv0y - uv2y, duv12x = uv1x - uv2x, duv12y = uv1y - uv2y;
    V3 dp02 = p0 - p2, dp12 = p1 - p2;
    float determinant = duv02x * duv12y - duv02y * duv12x;
    bool degenerate_uv = __builtin_fabsf(determinant) < 1e-8f;
    V3 dpdu = V3{0.0f, 0.0f, 0.0f}, dpdv = V3{0.0f, 0.0f, 0.0f};
    if (!degenerate_uv) {
        float inv_det = 1.0f / determinant;
        dpdu = (dp02 * duv12y - dp12 * duv02y) * inv_det;
        dpdv = (dp02 * -duv12x + dp12 * duv02x) * inv_det;
    }
    if (degenerate_uv || len2(cross(dpdu, dpdv)) == 0.0f) {
        V3 ng = cross(p2 - p0, p1 - p0);  // zero only for triangles flagged kTriDegenerate, which never get here
        coordinate_system(normalize(ng), &dpdu, &dpdv);
    }
    V3 n = normalize(cross(dp02, dp12));  // triangle.rs:244-245 (no orientation flip: D14)
    V3 ns = n, sdpdu = dpdu;
    if (bvh.tri_shading && (bvh.has_normals || bvh.has_tangents)) {
        V3 nsi = n;
        if (bvh.has_normals) {
            V3 n0 = V3{s0.x, s0.y, s0.z}, n1 = V3{s0.w, s1.x, s1.y}, n2 = V3{s1.z, s1.w, s2.x};
            nsi = n0 * b0 + n1 * b1 + n2 * b2;
            nsi = len2(nsi) > 0.0f ? normalize(nsi) : n;
        }
        V3 ss = normalize(dpdu);
        if (bvh.has_tangents) {  // triangle.rs:265-275
            V3 t0 = V3{s2.y, s2.z, s2.w}, t1 = V3{s3.x, s3.y, s3.z}, t2 = V3{s3.w, s4.x, s4.y};
            V3 si = t0 * b0 + t1 * b1 + t2 * b2;
            if (len2(si) > 0.0f) ss = normalize(si);
        }
        V3 ts = cross(ss, nsi);
        if (len2(ts) > 0.0f) {
            ts = normalize(ts);
            ss = cross(ts, nsi);
        } else {
            coordinate_system(nsi, &ss, &ts);
        }
        ns = normalize(cross(ss, ts));          // set_shading_geometry: shading.n = normalize(dpdu x dpdv)
        if (dot(n, ns) < 0.0f) n = -n;          // n = n.face_forward(shading.n)
        sdpdu = ss;
    }
    *n_out = n;
    *ns_out = ns;
    *dpdu_out = dpdu;
    *sdpdu_out = sdpdu;
}
PB_DEV Surf make_surface(const DevBVH& bvh, int slot, float b0, float b1, float b2, V3 ray_d) {
    V3 p0, p1, p2;
    int prim;
    Surf s;
    tri_vertices(bvh, slot, &p0, &p1, &p2, &prim, &s.material, &s.light);
    tri_shading_geometry(bvh, slot, p0, p1, p2, b0, b1, b2, &s.n, &s.ns, &s.dpdu, &s.sdpdu);
    float xs = __builtin_fabsf(b0 * p0.x) + __builtin_fabsf(b1 * p1.x) + __builtin_fabsf(b2 * p2.x);
    float ys = __builtin_fabsf(b0 * p0.y) + __builtin_fabsf(b1 * p1.y) + __builtin_fabsf(b2 * p2.y);
    float zs = __builtin_fabsf(b0 * p0.z) + __builtin_fabsf(b1 * p1.z) + __builtin_fabsf(b2 * p2.z);
    s.p_error = V3{xs, ys, zs} * kGamma7;
    s.p = p0 * b0 + p1 * b1 + p2 * b2;
    s.wo = -ray_d;
    return s;
}
// Transform::operator()(SurfaceInteraction) of pbrt-v3 (transform.rs:620-627 is a TODO in the reference, D6):
// object-space hit -> world space through the instance's matrices (primitive.rs:145-147).
// o0..o2: to_object rows (= inverse of to_world), w0..w2: to_world rows, mat: the instance's material override or -1
PB_DEV void instance_to_world_rows(float4 o0, float4 o1, float4 o2, float4 w0, float4 w1, float4 w2, int mat, Surf* s) {
    V3 p = s->p, pe = s->p_error;
    // point with incoming absolute error (geometry.rs:936-1000)
    float xp = w0.x * p.x + w0.y * p.y + w0.z * p.z + w0.w;
    float yp = w1.x * p.x + w1.y * p.y + w1.z * p.z + w1.w;
    float zp = w2.x * p.x + w2.y * p.y + w2.z * p.z + w2.w;
    const float g3 = kGamma3;
    V3 err;
    err.x = (g3 + 1.0f) * (__builtin_fabsf(w0.x * pe.x) + __builtin_fabsf(w0.y * pe.y) + __builtin_fabsf(w0.z * pe.z)) +
            g3 * (__builtin_fabsf(w0.x * p.x) + __builtin_fabsf(w0.y * p.y) + __builtin_fabsf(w0.z * p.z) + __builtin_fabsf(w0.w));
    err.y = (g3 + 1.0f) * (__builtin_fabsf(w1.x * pe.x) + __builtin_fabsf(w1.y * pe.y) + __builtin_fabsf(w1.z * pe.z)) +
            g3 * (__builtin_fabsf(w1.x * p.x) + __builtin_fabsf(w1.y * p.y) + __builtin_fabsf(w1.z * p.z) + __builtin_fabsf(w1.w));
    err.z = (g3 + 1.0f) * (__builtin_fabsf(w2.x * pe.x) + __builtin_fabsf(w2.y * pe.y) + __builtin_fabsf(w2.z * pe.z)) +
            g3 * (__builtin_fabsf(w2.x * p.x) + __builtin_fabsf(w2.y * p.y) + __builtin_fabsf(w2.z * p.z) + __builtin_fabsf(w2.w));
    s->p = V3{xp, yp, zp};
    s->p_error = err;
    // normal: (M^-1)^T n (transform.rs:387-403, intended form), then normalised
    V3 n = s->n;
    s->n = normalize(V3{o0.x * n.x + o1.x * n.y + o2.x * n.z, o0.y * n.x + o1.y * n.y + o2.y * n.z,
                        o0.z * n.x + o1.z * n.y + o2.z * n.z});
    {   // shading.n, shading.dpdu, then shading.n = face_forward(shading.n, n) (pbrt-v3 Transform(SurfaceInteraction))
        V3 sn = s->ns, sd = s->sdpdu;
        sn = normalize(V3{o0.x * sn.x + o1.x * sn.y + o2.x * sn.z, o0.y * sn.x + o1.y * sn.y + o2.y * sn.z,
                          o0.z * sn.x + o1.z * sn.y + o2.z * sn.z});
        s->ns = dot(sn, s->n) < 0.0f ? -sn : sn;
        s->sdpdu = V3{w0.x * sd.x + w0.y * sd.y + w0.z * sd.z, w1.x * sd.x + w1.y * sd.y + w1.z * sd.z,
                      w2.x * sd.x + w2.y * sd.y + w2.z * sd.z};
    }
    V3 wo = s->wo, du = s->dpdu;
    s->wo = normalize(V3{w0.x * wo.x + w0.y * wo.y + w0.z * wo.z, w1.x * wo.x + w1.y * wo.y + w1.z * wo.z,
                         w2.x * wo.x + w2.y * wo.y + w2.z * wo.z});
    s->dpdu = V3{w0.x * du.x + w0.y * du.y + w0.z * du.z, w1.x * du.x + w1.y * du.y + w1.z * du.z,
                 w2.x * du.x + w2.y * du.y + w2.z * du.z};
    if (mat >= 0) s->material = mat;
    s->light = -1;  // instanced primitives carry no area lights
}
PB_DEV void instance_to_world(const DevBVH& bvh, int inst_slot, Surf* s) {
    const float4* m = bvh.instances + 7 * (size_t)inst_slot;
    instance_to_world_rows(m[0], m[1], m[2], m[3], m[4], m[5], __float_as_int(m[6].x), s);
}
// The rows of a moving scene's instance slot at the path's time, as the traversal kernel entered it (trace_persistent.h,
// MOV): the slot's own for a static instance and up to the start time, the stored end rows from the end time on,
// AnimatedTransform::interpolate's (motion.h) between them.
PB_DEV void instance_rows_at(const DevBVH& bvh, const DevMotion* __restrict__ motions, int inst_slot, float time, float4* o, float4* w) {
    const float4* m = bvh.instances + 7 * (size_t)inst_slot;
    for (int k = 0; k < 3; ++k) {
        o[k] = m[k];
        w[k] = m[3 + k];
    }
    const DevMotion& mo = motions[inst_slot];
    if (!mo.animated || time <= mo.start_time) return;
    if (time >= mo.end_time) {
        const float4* eo = reinterpret_cast<const float4*>(mo.end_w2o);
        const float4* ew = reinterpret_cast<const float4*>(mo.end_o2w);
        for (int k = 0; k < 3; ++k) {
            o[k] = eo[k];
            w[k] = ew[k];
        }
        return;
    }
    MotionRows rows;
    motion_interpolate(mo, time, &rows);
    for (int k = 0; k < 3; ++k) {
        o[k] = make_float4(rows.w2o[4 * k], rows.w2o[4 * k + 1], rows.w2o[4 * k + 2], rows.w2o[4 * k + 3]);
        w[k] = make_float4(rows.o2w[4 * k], rows.o2w[4 * k + 1], rows.o2w[4 * k + 2], rows.o2w[4 * k + 3]);
    }
}
// TransformedPrimitive::intersect's second half over an AnimatedTransform (primitive.rs:140-147): the same interpolation at
// the path's time, then the formulas of instance_to_world
PB_DEV void instance_to_world_moving(const DevBVH& bvh, const float4* o, const float4* w, int inst_slot, Surf* s) {
    instance_to_world_rows(o[0], o[1], o[2], w[0], w[1], w[2], __float_as_int(bvh.instances[7 * (size_t)inst_slot + 6].x), s);
}
// Sphere::intersect past the hit test (sphere.rs:38-92) for a full sphere placed by translate(centre): partial
// derivatives, SurfaceInteraction::new, then pbrt-v3's Transform(SurfaceInteraction) through that translation (every
// product of the general matrix formulas is kept, as in sphere_object_ray). ph = the refined object-space hit point.
PB_DEV Surf make_surface_sphere(const DevBVH& bvh, int slot, V3 ph, V3 rd) {
    float4 a = bvh.tris[3 * (size_t)slot], c4 = bvh.tris[3 * (size_t)slot + 2];
    float cx = a.x, cy = a.y, cz = a.z, radius = a.w;
    Surf s;
    s.material = __float_as_int(c4.z);
    s.light = (__float_as_int(c4.w) & kPrimLightMask) - 1;
    const float phi_max = 360.0f * (kPi / 180.0f);
    const float theta_min = det_acos(clampf(fminr(-radius, radius) / radius, -1.0f, 1.0f));
    const float theta_max = det_acos(clampf(fmaxr(-radius, radius) / radius, -1.0f, 1.0f));
    float theta = det_acos(clampf(ph.z / radius, -1.0f, 1.0f));
    float z_radius = __builtin_sqrtf(ph.x * ph.x + ph.y * ph.y);
    float inv_z_radius = 1.0f / z_radius;
    float cos_phi = ph.x * inv_z_radius, sin_phi = ph.y * inv_z_radius;
    V3 dpdu = V3{-phi_max * ph.y, phi_max * ph.x, 0.0f};
    V3 dpdv = V3{ph.z * cos_phi, ph.z * sin_phi, -radius * det_sin(theta)} * (theta_max - theta_min);
    V3 n = normalize(cross(dpdu, dpdv));  // SurfaceInteraction::new (interaction.rs:248-300)
    V3 pe = vabs(ph) * kGamma5;
    // Transform(SurfaceInteraction) with m = translate(c), m_inv = translate(-c)
    const float g3 = kGamma3;
    float x = ph.x, y = ph.y, z = ph.z;
    s.p = V3{1.0f * x + 0.0f * y + 0.0f * z + cx, 0.0f * x + 1.0f * y + 0.0f * z + cy, 0.0f * x + 0.0f * y + 1.0f * z + cz};
    s.p_error.x = (g3 + 1.0f) * (__builtin_fabsf(1.0f * pe.x) + __builtin_fabsf(0.0f * pe.y) + __builtin_fabsf(0.0f * pe.z)) +
                  g3 * (__builtin_fabsf(1.0f * x) + __builtin_fabsf(0.0f * y) + __builtin_fabsf(0.0f * z) + __builtin_fabsf(cx));
    s.p_error.y = (g3 + 1.0f) * (__builtin_fabsf(0.0f * pe.x) + __builtin_fabsf(1.0f * pe.y) + __builtin_fabsf(0.0f * pe.z)) +
                  g3 * (__builtin_fabsf(0.0f * x) + __builtin_fabsf(1.0f * y) + __builtin_fabsf(0.0f * z) + __builtin_fabsf(cy));
    s.p_error.z = (g3 + 1.0f) * (__builtin_fabsf(0.0f * pe.x) + __builtin_fabsf(0.0f * pe.y) + __builtin_fabsf(1.0f * pe.z)) +
                  g3 * (__builtin_fabsf(0.0f * x) + __builtin_fabsf(0.0f * y) + __builtin_fabsf(1.0f * z) + __builtin_fabsf(cz));
    auto through = [](V3 v) {  // upper 3x3 of either matrix (the identity), as xform_vector / xform_normal evaluate it
        return V3{1.0f * v.x + 0.0f * v.y + 0.0f * v.z, 0.0f * v.x + 1.0f * v.y + 0.0f * v.z, 0.0f * v.x + 0.0f * v.y + 1.0f * v.z};
    };
    s.n = normalize(through(n));
    V3 d_obj = through(rd);  // the object-space ray direction of sphere_object_ray
    s.wo = normalize(through(-d_obj));
    s.dpdu = through(dpdu);
    V3 sn = normalize(through(n));  // shading.n = n before the transform (D47)
    s.ns = dot(sn, s.n) < 0.0f ? -sn : sn;
    s.sdpdu = through(dpdu);
    return s;
}
// Sphere / Disk / Cylinder::intersect past the hit test (sphere.rs:38-92, disk.rs:97-105, cylinder.rs:105-115) for a row of the
// shape table: partial derivatives and the object-space error bound, SurfaceInteraction::new (n = normalize(dpdu x dpdv),
// flipped when reverse_orientation ^ transform_swaps_handedness, as in pbrt-v3), then pbrt-v3's Transform(SurfaceInteraction)
// through the shape's matrices, in the operation order of make_surface_sphere / instance_to_world. ph = the hit record's
// object-space point (sphere and cylinder: refined onto the surface; disk: z is set to the height here).
PB_DEV Surf make_surface_shape(const DevBVH& bvh, int slot, V3 ph, V3 rd) {
    float4 c4 = bvh.tris[3 * (size_t)slot + 2];
    const DevShape& sh = bvh.shapes[__float_as_int(c4.x)];
    Surf s;
    s.material = __float_as_int(c4.z);
    s.light = (__float_as_int(c4.w) & kPrimLightMask) - 1;
    const int type = sh.flags & kShapeTypeMask;
    const float radius = sh.radius, phi_max = sh.phi_max;
    V3 dpdu = V3{-phi_max * ph.y, phi_max * ph.x, 0.0f};
    float vx, vy, vz, ex, ey, ez, z = ph.z;  // dpdv, the object-space error bound (scalars: the branches assign no aggregate)
    if (type == kShapeSphere) {
        float theta = det_acos(clampf(ph.z / radius, -1.0f, 1.0f));
        float z_radius = __builtin_sqrtf(ph.x * ph.x + ph.y * ph.y);
        float inv_z_radius = 1.0f / z_radius;
        float cos_phi = ph.x * inv_z_radius, sin_phi = ph.y * inv_z_radius;
        float dtheta = sh.theta_max - sh.theta_min;
        vx = (ph.z * cos_phi) * dtheta;
        vy = (ph.z * sin_phi) * dtheta;
        vz = (-radius * det_sin(theta)) * dtheta;
        ex = __builtin_fabsf(ph.x) * kGamma5;
        ey = __builtin_fabsf(ph.y) * kGamma5;
        ez = __builtin_fabsf(ph.z) * kGamma5;
    } else if (type == kShapeCylinder) {
        vx = 0.0f;
        vy = 0.0f;
        vz = sh.z_max - sh.z_min;
        ex = __builtin_fabsf(ph.x) * kGamma3;
        ey = __builtin_fabsf(ph.y) * kGamma3;
        ez = __builtin_fabsf(0.0f) * kGamma3;
    } else {
        float r_hit = __builtin_sqrtf(ph.x * ph.x + ph.y * ph.y);
        float k = sh.inner_radius - radius;
        vx = (ph.x * k) / r_hit;
        vy = (ph.y * k) / r_hit;
        vz = (0.0f * k) / r_hit;
        z = sh.z_min;
        ex = ey = ez = 0.0f;
    }
    const V3 dpdv = V3{vx, vy, vz}, pe = V3{ex, ey, ez};
    V3 n = normalize(cross(dpdu, dpdv));  // SurfaceInteraction::new (interaction.rs:248-300)
    if (sh.flags & kShapeFlipNormal) n = -n;
    const float* w = sh.o2w;
    const float* o = sh.w2o;
    const float g3 = kGamma3;
    float x = ph.x, y = ph.y;
    s.p = V3{w[0] * x + w[1] * y + w[2] * z + w[3], w[4] * x + w[5] * y + w[6] * z + w[7], w[8] * x + w[9] * y + w[10] * z + w[11]};
    s.p_error.x = (g3 + 1.0f) * (__builtin_fabsf(w[0] * pe.x) + __builtin_fabsf(w[1] * pe.y) + __builtin_fabsf(w[2] * pe.z)) +
                  g3 * (__builtin_fabsf(w[0] * x) + __builtin_fabsf(w[1] * y) + __builtin_fabsf(w[2] * z) + __builtin_fabsf(w[3]));
    s.p_error.y = (g3 + 1.0f) * (__builtin_fabsf(w[4] * pe.x) + __builtin_fabsf(w[5] * pe.y) + __builtin_fabsf(w[6] * pe.z)) +
                  g3 * (__builtin_fabsf(w[4] * x) + __builtin_fabsf(w[5] * y) + __builtin_fabsf(w[6] * z) + __builtin_fabsf(w[7]));
    s.p_error.z = (g3 + 1.0f) * (__builtin_fabsf(w[8] * pe.x) + __builtin_fabsf(w[9] * pe.y) + __builtin_fabsf(w[10] * pe.z)) +
                  g3 * (__builtin_fabsf(w[8] * x) + __builtin_fabsf(w[9] * y) + __builtin_fabsf(w[10] * z) + __builtin_fabsf(w[11]));
    auto vec = [](const float* m, V3 v) {  // Transform * Vector3: the upper 3x3
        return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
    };
    auto nrm = [o](V3 v) {  // Transform * Normal3: the transpose of the inverse's upper 3x3
        return V3{o[0] * v.x + o[4] * v.y + o[8] * v.z, o[1] * v.x + o[5] * v.y + o[9] * v.z, o[2] * v.x + o[6] * v.y + o[10] * v.z};
    };
    s.n = normalize(nrm(n));
    V3 d_obj = vec(o, rd);  // the object-space ray direction of shape_object_ray
    s.wo = normalize(vec(w, -d_obj));
    s.dpdu = vec(w, dpdu);
    V3 sn = normalize(nrm(n));  // shading.n = n before the transform (D47)
    s.ns = dot(sn, s.n) < 0.0f ? -sn : sn;
    s.sdpdu = vec(w, dpdu);
    return s;
}
// Hit record -> world-space surface. `rd` is the world-space ray direction. SHP: the scene may hold general shapes
// (DevBVH::has_spheres == 2); a template value so that the kernels of the other scenes compile without the dispatch.
template <bool SHP = false>
PB_DEV Surf surface_from_hit(const DevBVH& bvh, int slot, int inst_slot, float b0, float b1, float b2, V3 rd) {
    if (SHP) {
        Surf s;
        if (__float_as_int(bvh.tris[3 * (size_t)slot + 2].w) & kPrimSphere)
            s = make_surface_shape(bvh, slot, V3{b0, b1, b2}, rd);
        else
            s = make_surface(bvh, slot, b0, b1, b2, rd);
        return s;
    }
    if (bvh.has_spheres && (__float_as_int(bvh.tris[3 * (size_t)slot + 2].w) & kPrimSphere))
        return make_surface_sphere(bvh, slot, V3{b0, b1, b2}, rd);
    if (bvh.instanced && inst_slot >= 0) {
        const float4* m = bvh.instances + 7 * (size_t)inst_slot;
        float4 r0 = m[0], r1 = m[1], r2 = m[2];
        // the object-space ray direction TransformedPrimitive::intersect traced (geometry.rs:872)
        V3 d_obj = V3{r0.x * rd.x + r0.y * rd.y + r0.z * rd.z, r1.x * rd.x + r1.y * rd.y + r1.z * rd.z,
                      r2.x * rd.x + r2.y * rd.y + r2.z * rd.z};
        Surf s = make_surface(bvh, slot, b0, b1, b2, d_obj);
        instance_to_world(bvh, inst_slot, &s);
        return s;
    }
    return make_surface(bvh, slot, b0, b1, b2, rd);
}
// ... in a scene with moving instances (two levels, triangles only): `time` is the path's
PB_DEV Surf surface_from_hit_moving(const DevBVH& bvh, const DevMotion* __restrict__ motions, float time, int slot, int inst_slot,
                                    float b0, float b1, float b2, V3 rd) {
    if (inst_slot < 0) return make_surface(bvh, slot, b0, b1, b2, rd);
    float4 o[3], w[3];
    instance_rows_at(bvh, motions, inst_slot, time, o, w);
    V3 d_obj = V3{o[0].x * rd.x + o[0].y * rd.y + o[0].z * rd.z, o[1].x * rd.x + o[1].y * rd.y + o[1].z * rd.z,
                  o[2].x * rd.x + o[2].y * rd.y + o[2].z * rd.z};
    Surf s = make_surface(bvh, slot, b0, b1, b2, d_obj);
    instance_to_world_moving(bvh, o, w, inst_slot, &s);
    return s;
}
// Curve::intersect past the hit test (curve.rs:243-276) for row `row` of the curve table. A curve's hit record carries (u, v, 0)
// and no t, so the surface is rebuilt from the ray: the hit test runs again on this one curve with an unbounded ray and gives
// the hit the traversal kernel recorded (the nearest inside the curve: a t_max only ever prunes it), and with it t, hit_width
// and the ray's frame. p = ray(t) with p_error = 2 hit_width on each axis, dpdu from the whole curve at u, dpdv across the
// ray (flat), rotated about dpdu by lerp(v, -90, 90) degrees (cylinder) or n_hit x dpdu (ribbon); n = normalize(dpdu x dpdv),
// flipped by reverse_orientation ^ swaps_handedness; shading geometry = geometric. Then Transform(SurfaceInteraction) through
// the curve's matrices as make_surface_shape does it.
PB_DEV Surf make_surface_curve(const DevBVH& bvh, const DevCurve* __restrict__ curves, int slot, int row, V3 ro, V3 rd) {
    float4 c4 = bvh.tris[3 * (size_t)slot + 2];
    const DevCurve& c = curves[row];
    Surf s;
    s.material = __float_as_int(c4.z);
    s.light = -1;
    CurveHit h;
    CurveFrame f;
    h.t = h.u = h.width = 0.0f;
    h.v = 0.5f;
    f.n_hit = V3{0.0f, 0.0f, 1.0f};
    // Invariant: this call finds the hit. It evaluates the expressions the traversal kernel evaluated, on the same inputs, in
    // the same order and without contraction; the only difference is t_max = inf, which can only let more through. Should it
    // miss all the same (another compiler, another build of one of the two), the end of this function replaces what was
    // computed from the empty hit by a finite surface, so that no NaN reaches the film.
    f.o = ro;
    f.d = rd;
    f.right = V3{1.0f, 0.0f, 0.0f};
    f.up = V3{0.0f, 1.0f, 0.0f};
    f.dir = V3{0.0f, 0.0f, 1.0f};
    f.ray_length = 1.0f;
    const bool found = curve_test(c, TravRay{ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, kInf}, kInf, false, &h, &f);
    const int type = c.flags & kCurveTypeMask;
    V3 dpdu, dpdv;
    (void)curve_eval(V3{c.cp[0], c.cp[1], c.cp[2]}, V3{c.cp[3], c.cp[4], c.cp[5]}, V3{c.cp[6], c.cp[7], c.cp[8]}, V3{c.cp[9], c.cp[10], c.cp[11]},
                     h.u, &dpdu);
    if (type == kCurveRibbon) {
        dpdv = normalize(cross(f.n_hit, dpdu)) * h.width;
    } else {
        // object_to_ray and back are rotations by (right, up, dir)
        const V3 du = V3{dot(f.right, dpdu), dot(f.up, dpdu), dot(f.dir, dpdu)};
        V3 dv = normalize(V3{-du.y, du.x, 0.0f}) * h.width;
        if (type == kCurveCylinder) {
            // Rotate(-theta, dpdu_plane) (transform.rs): v cos + (a x v) sin + a (a . v) (1 - cos) about the unit axis a
            const float theta = curve_lerp(h.v, -90.0f, 90.0f);
            float sn, cs;
            det_sincos(-theta * (kPi / 180.0f), &sn, &cs);
            const V3 a = normalize(du);
            dv = dv * cs + cross(a, dv) * sn + a * (dot(a, dv) * (1.0f - cs));
        }
        dpdv = f.right * dv.x + f.up * dv.y + f.dir * dv.z;
    }
    V3 n = normalize(cross(dpdu, dpdv));  // SurfaceInteraction::new (interaction.rs:248-300)
    if (c.flags & kCurveFlipNormal) n = -n;
    const V3 ph = f.o + f.d * h.t;
    const float pe = 2.0f * h.width;
    const float* w = c.o2w;
    const float* o = c.w2o;
    const float g3 = kGamma3;
    const float x = ph.x, y = ph.y, z = ph.z;
    s.p = V3{w[0] * x + w[1] * y + w[2] * z + w[3], w[4] * x + w[5] * y + w[6] * z + w[7], w[8] * x + w[9] * y + w[10] * z + w[11]};
    s.p_error.x = (g3 + 1.0f) * (__builtin_fabsf(w[0] * pe) + __builtin_fabsf(w[1] * pe) + __builtin_fabsf(w[2] * pe)) +
                  g3 * (__builtin_fabsf(w[0] * x) + __builtin_fabsf(w[1] * y) + __builtin_fabsf(w[2] * z) + __builtin_fabsf(w[3]));
    s.p_error.y = (g3 + 1.0f) * (__builtin_fabsf(w[4] * pe) + __builtin_fabsf(w[5] * pe) + __builtin_fabsf(w[6] * pe)) +
                  g3 * (__builtin_fabsf(w[4] * x) + __builtin_fabsf(w[5] * y) + __builtin_fabsf(w[6] * z) + __builtin_fabsf(w[7]));
    s.p_error.z = (g3 + 1.0f) * (__builtin_fabsf(w[8] * pe) + __builtin_fabsf(w[9] * pe) + __builtin_fabsf(w[10] * pe)) +
                  g3 * (__builtin_fabsf(w[8] * x) + __builtin_fabsf(w[9] * y) + __builtin_fabsf(w[10] * z) + __builtin_fabsf(w[11]));
    auto vec = [](const float* m, V3 v) {  // Transform * Vector3: the upper 3x3
        return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
    };
    auto nrm = [o](V3 v) {  // Transform * Normal3: the transpose of the inverse's upper 3x3
        return V3{o[0] * v.x + o[4] * v.y + o[8] * v.z, o[1] * v.x + o[5] * v.y + o[9] * v.z, o[2] * v.x + o[6] * v.y + o[10] * v.z};
    };
    s.n = normalize(nrm(n));
    s.wo = normalize(vec(w, -f.d));
    s.dpdu = vec(w, dpdu);
    if (!found) {  // (see the invariant above) the curve's material at the ray's origin, facing the ray
        s.p = ro;
        s.p_error = V3{0.0f, 0.0f, 0.0f};
        s.n = s.wo = normalize(-rd);
        V3 other;
        coordinate_system(s.n, &s.dpdu, &other);
    }
    s.ns = s.n;
    s.sdpdu = s.dpdu;
    return s;
}
// Hit record -> world-space surface in a scene with curves: `ro` / `rd` the world-space ray; everything but a curve as in the
// build for shapes
PB_DEV Surf surface_from_hit_curves(const DevBVH& bvh, const DevCurve* __restrict__ curves, int slot, float b0, float b1, float b2, V3 ro, V3 rd) {
    const float4 c4 = bvh.tris[3 * (size_t)slot + 2];
    Surf s;
    if ((__float_as_int(c4.w) & kPrimSphere) && __float_as_int(c4.x) < 0)
        s = make_surface_curve(bvh, curves, slot, ~__float_as_int(c4.x), ro, rd);
    else
        s = surface_from_hit<true>(bvh, slot, -1, b0, b1, b2, rd);
    return s;
}
// SurfaceInteraction::n of a hit at barycentrics (b0, b1, b2): the geometric normal, on the shading normal's side
template <bool SHP = false>
PB_DEV V3 tri_interaction_normal(const DevBVH& bvh, int slot, float b0, float b1, float b2) {
    if (SHP && (__float_as_int(bvh.tris[3 * (size_t)slot + 2].w) & kPrimSphere))
        return make_surface_shape(bvh, slot, V3{b0, b1, b2}, V3{0.0f, 0.0f, 1.0f}).n;  // (b0, b1, b2) = the hit point
    if (bvh.has_spheres && (__float_as_int(bvh.tris[3 * (size_t)slot + 2].w) & kPrimSphere))
        return make_surface_sphere(bvh, slot, V3{b0, b1, b2}, V3{0.0f, 0.0f, 1.0f}).n;  // (b0, b1, b2) = the hit point
    V3 p0, p1, p2;
    int a, b, c;
    tri_vertices(bvh, slot, &p0, &p1, &p2, &a, &b, &c);
    if (!(bvh.tri_shading && (bvh.has_normals || bvh.has_tangents))) return normalize(cross(p0 - p2, p1 - p2));
    V3 n, ns, dpdu, sdpdu;
    tri_shading_geometry(bvh, slot, p0, p1, p2, b0, b1, b2, &n, &ns, &dpdu, &sdpdu);
    return n;
}

struct Frame {  // BSDF::new (reflection.rs:220-234)
    V3 ss, ts, ns, ng;
};
PB_DEV V3 to_local(const Frame& f, V3 v) { return V3{dot(v, f.ss), dot(v, f.ts), dot(v, f.ns)}; }
PB_DEV V3 to_world(const Frame& f, V3 v) {
    return V3{f.ss.x * v.x + f.ts.x * v.y + f.ns.x * v.z, f.ss.y * v.x + f.ts.y * v.y + f.ns.y * v.z,
              f.ss.z * v.x + f.ts.z * v.y + f.ns.z * v.z};
}

// BSDF::f and BSDF::pdf for the non-specular query of estimate_direct: only the Lambertian lobe of
// a matte material matches (reflection.rs:264-283, 414-446, 475-481, 840-842).
PB_DEV void matte_f_pdf(const Frame& fr, V3 kd, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f) return;
    bool reflect = dot(wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    if (reflect) *f = V3{0.0f + kd.x * kInvPi, 0.0f + kd.y * kInvPi, 0.0f + kd.z * kInvPi};
    float p = (wo.z * wi.z > 0.0f) ? __builtin_fabsf(wi.z) * kInvPi : 0.0f;
    *pdf = (0.0f + p) / 1.0f;
}
// BSDF::sample_f with one Lambertian lobe (reflection.rs:285-377, 459-472)
PB_DEV V3 matte_sample_f(const Frame& fr, V3 kd, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    *ok = false;
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    float ur = fminr(u0 * 1.0f - 0.0f, kOneMinusEpsilon);
    V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;  // pdf keeps the caller's value (reflection.rs:323-326)
    V3 wi = cosine_sample_hemisphere(ur, u1);
    if (wo.z < 0.0f) wi.z *= -1.0f;
    *pdf = (wo.z * wi.z > 0.0f) ? __builtin_fabsf(wi.z) * kInvPi : 0.0f;
    if (*pdf == 0.0f) return zero;
    *wi_w = to_world(fr, wi);
    *ok = true;
    bool reflect = dot(*wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    if (!reflect) return zero;
    return V3{0.0f + kd.x * kInvPi, 0.0f + kd.y * kInvPi, 0.0f + kd.z * kInvPi};
}

PB_DEV bool is_black(V3 c) { return c.x == 0.0f && c.y == 0.0f && c.z == 0.0f; }
PB_DEV V3 mulv(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
PB_DEV float max_comp(V3 c) {
    float m = -kFloatMax;
    m = (m > c.x) ? m : c.x;
    m = (m > c.y) ? m : c.y;
    m = (m > c.z) ? m : c.z;
    return m;
}

// find_interval over a cdf with predicate cdf[i] < u (pbrt.rs:229-243, sampling.rs:107)
PB_DEV int find_interval_cdf(const float* cdf, int size, float u) {
    int first = 0, len = size;
    while (len > 0) {
        int half = len >> 1, middle = first + half;
        if (cdf[middle] < u) {
            first = middle + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    int v = first - 1;
    return v < 0 ? 0 : (v > size - 2 ? size - 2 : v);
}
// Distribution1D::sample_continuous (sampling.rs:99-123) on a 2-bin table
PB_DEV float sample_continuous2(const float* func, const float* cdf, float func_int, float u, float* pdf, int* off) {
    int offset = find_interval_cdf(cdf, 3, u);
    *off = offset;
    float du = u - cdf[offset];
    if (cdf[offset + 1] - cdf[offset] > 0.0f) du /= cdf[offset + 1] - cdf[offset];
    *pdf = func_int > 0.0f ? func[offset] / func_int : 0.0f;
    return ((float)offset + du) / 2.0f;
}

// Full Triangle::intersect of ONE triangle for Shape::pdf2 (shape.rs:54-69): returns hit point and normal
PB_DEV bool light_triangle_intersect(const DevBVH& bvh, int slot, V3 o, V3 d, V3* p_hit, V3* n_hit) {
    V3 p0, p1, p2;
    int flags;
    load_tri(bvh.tris, slot, &p0, &p1, &p2, &flags);
    TravRay r{o.x, o.y, o.z, d.x, d.y, d.z, kInf};
    TriRayConst c = tri_ray_setup(r);
    float b0, b1, b2, t;
    if (!triangle_test(p0, p1, p2, r, c, kInf, &b0, &b1, &b2, &t)) return false;
    if (flags & kTriDegenerate) return false;
    *p_hit = p0 * b0 + p1 * b1 + p2 * b2;
    *n_hit = tri_interaction_normal(bvh, slot, b0, b1, b2);
    return true;
}

struct ShadeConsts {
    DevBVH bvh;
    const DevMaterial* materials;
    const DevLight* lights;
    int n_lights, n_infinite;
    const int* infinite_ids;
    const DevEnvMap* env_maps;  // image maps of infinite lights (DevLight::slot >= 0), null when there are none
    DevDistribution1D distrib;  // light_distribution.lookup (lightdistrib.rs:43/66)
    float env_cond_func[2][2], env_cond_cdf[2][3], env_cond_int[2];
    float env_marg_func[2], env_marg_cdf[3], env_marg_int;
    float world_radius;
    // DirectLightingIntegrator (directlighting.rs:58-78): per-light sample counts, prefix sums
    const int* light_sample_prefix;  // [n_lights + 1]
    int total_light_samples;
    // SpatialLightDistribution (lightdistrib.rs:76-220): one Distribution1D per voxel of the scene bounds,
    // spatial[v * (2 n + 2)] = func[n], cdf[n + 1], func_int; null = the fixed `distrib`
    const float* spatial;
    int n_voxel[3];
    // MIS rays towards lights that are not area lights are queued as RS_MIS_BOOL (wf_state.h); off while the reference's
    // loops are being counted (pbrt_hip_set_counting(1): the reference walks those rays to their closest hit)
    int mis_bool;
    const DevDisney* disney;  // [n_materials]: the blocks of the kMatDisney rows (wf_disney.h)
    const DevLightMap* light_maps;  // side table of the projection / goniometric lights (DevLight::slot), null when there are none
    const DevLobeRow* lobe_rows;  // [n_materials]: the lobe lists of the kMatLobes rows (wf_lobes.h)
    // One side table, by the kind of scene: a scene has two levels and may move, or has one level and may hold curves, never both
    // (creation refuses it). One slot for both keeps the argument block of every shading kernel the size and layout it had before
    // curves, and with it the text of the 38 kernels that read nothing else new (profiles/curve_resource_usage.txt).
    union {
        const DevMotion* motions;  // [top-level leaf slots]: the side table of a scene with moving instances (motion.h), else null
        const DevCurve* curves;    // the rows of a one-level scene's curve segments (shapes_curve.h), else null
    };
};

// ---- InfiniteAreaLight with an image map (DevEnvMap): one lookup and one Distribution2D for le, sample_li and pdf_li ----
// MIPMap::lookup at width 0 (mipmap.rs:211-215): MIPMap::triangle on level 0, ImageWrap::Repeat, signed floor (D60).
// Map: DevEnvMap, or the DevLightMap of a projection / goniometric light (texels, w, h)
template <class Map>
PB_DEV V3 env_lookup(const Map& e, float st_s, float st_t) {
    float s = st_s * (float)e.w - 0.5f, t = st_t * (float)e.h - 0.5f;
    if (!(s >= -1.0f && s <= (float)e.w)) s = -0.5f;  // a NaN direction: keep the fetches inside the level
    if (!(t >= -1.0f && t <= (float)e.h)) t = -0.5f;
    float fs = __builtin_floorf(s), ft = __builtin_floorf(t);
    float ds = s - fs, dt = t - ft;
    int s0 = (int)fs, t0 = (int)ft;
    s0 = s0 < 0 ? s0 + e.w : (s0 >= e.w ? s0 - e.w : s0);  // -1 <= s0 <= w, -1 <= t0 <= h
    t0 = t0 < 0 ? t0 + e.h : (t0 >= e.h ? t0 - e.h : t0);
    int s1 = s0 + 1 >= e.w ? s0 + 1 - e.w : s0 + 1;
    int t1 = t0 + 1 >= e.h ? t0 + 1 - e.h : t0 + 1;
    float4 a = e.texels[(size_t)t0 * e.w + s0], b = e.texels[(size_t)t1 * e.w + s0];
    float4 c = e.texels[(size_t)t0 * e.w + s1], d = e.texels[(size_t)t1 * e.w + s1];
    float wa = (1.0f - ds) * (1.0f - dt), wb = (1.0f - ds) * dt, wc = ds * (1.0f - dt), wd = ds * dt;
    return V3{a.x * wa + b.x * wb + c.x * wc + d.x * wd, a.y * wa + b.y * wb + c.y * wc + d.y * wd,
              a.z * wa + b.z * wb + c.z * wc + d.z * wd};
}
PB_DEV V3 mat3_mul(const float* m, V3 v) {  // Transform * Vector3 (transform.rs), upper 3x3 row-major
    return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z};
}
// spherical (phi / 2pi, theta / pi) of a light-space direction (geometry.rs spherical_phi / spherical_theta); sin(theta)
PB_DEV void env_uv(V3 wl, float* u, float* v, float* sin_theta) {
    float theta = det_acos(clampf(wl.z, -1.0f, 1.0f));
    float phi = det_atan2(wl.y, wl.x);
    if (phi < 0.0f) phi = phi + 2.0f * kPi;
    *u = phi * kInv2Pi;
    *v = theta * kInvPi;
    if (sin_theta) *sin_theta = det_sin(theta);
}
// InfiniteAreaLight::le (infinite.rs:84-88; D33 intended: the light's le) for a world direction
PB_DEV V3 env_le(const DevEnvMap& e, V3 d) {
    float u, v;
    env_uv(normalize(mat3_mul(e.w2l, d)), &u, &v, nullptr);
    return env_lookup(e, u, v);
}
// Distribution1D::sample_continuous (sampling.rs:99-123) over an n-entry table
PB_DEV float sample_continuous_n(const float* func, const float* cdf, float func_int, int n, float u, float* pdf, int* off) {
    int offset = find_interval_cdf(cdf, n + 1, u);
    *off = offset;
    float c0 = cdf[offset], c1 = cdf[offset + 1];
    float du = u - c0;
    if (c1 - c0 > 0.0f) du /= c1 - c0;
    *pdf = func_int > 0.0f ? func[offset] / func_int : 0.0f;
    return ((float)offset + du) / (float)n;
}
// Distribution2D::sample_continuous (sampling.rs:186-197): (u, v) and the map pdf
PB_DEV void env_sample(const DevEnvMap& e, float u0, float u1, float* d0, float* d1, float* map_pdf) {
    float pdf0, pdf1;
    int v, dummy;
    *d1 = sample_continuous_n(e.row_int, e.marg_cdf, e.marg_int, e.nv, u1, &pdf1, &v);
    *d0 = sample_continuous_n(e.func + (size_t)v * e.nu, e.cdf + (size_t)v * (e.nu + 1), e.row_int[v], e.nu, u0, &pdf0, &dummy);
    *map_pdf = pdf0 * pdf1;
}
// InfiniteAreaLight::pdf_li (infinite.rs:140-151; Distribution2D::pdf, sampling.rs:199-212, D48 intended) for a world direction
PB_DEV float env_pdf(const DevEnvMap& e, V3 wi) {
    float u, v, st;
    env_uv(mat3_mul(e.w2l, wi), &u, &v, &st);
    if (st == 0.0f || e.marg_int == 0.0f) return 0.0f;  // (a black map: no light sample either, D61)
    int iu = (int)(u * (float)e.nu);
    iu = iu < 0 ? 0 : (iu > e.nu - 1 ? e.nu - 1 : iu);
    int iv = (int)(v * (float)e.nv);
    iv = iv < 0 ? 0 : (iv > e.nv - 1 ? e.nv - 1 : iv);
    return e.func[(size_t)iv * e.nu + iu] / e.marg_int / (2.0f * kPi * kPi * st);
}

// SpatialLightDistribution::lookup (lightdistrib.rs:171-182): the voxel of p, then its distribution
PB_DEV DevDistribution1D light_distribution_lookup(const ShadeConsts& sc, V3 p) {
    if (!sc.spatial) return sc.distrib;
    const float* mn = sc.bvh.root_min;
    const float* mx = sc.bvh.root_max;
    float o[3] = {p.x - mn[0], p.y - mn[1], p.z - mn[2]};  // Bounds3::offset
    int pi[3];
    for (int i = 0; i < 3; ++i) {
        if (mx[i] > mn[i]) o[i] /= mx[i] - mn[i];
        int v = (int)(o[i] * (float)sc.n_voxel[i]);
        pi[i] = v < 0 ? 0 : (v > sc.n_voxel[i] - 1 ? sc.n_voxel[i] - 1 : v);
    }
    size_t voxel = ((size_t)pi[2] * sc.n_voxel[1] + pi[1]) * sc.n_voxel[0] + pi[0];
    const float* t = sc.spatial + voxel * (size_t)(2 * sc.n_lights + 2);
    DevDistribution1D d;
    d.func = t;
    d.cdf = t + sc.n_lights;
    d.func_int = t[2 * sc.n_lights + 1];
    d.n = sc.n_lights;
    return d;
}

PB_DEV Samp path_sampler(const PathState& ps, const PassParams& pp, const TileList& tiles, uint32_t p) {
    // this path's stream: inc from the (pixel, sample) index, state and the dimension counters from memory
    Samp sm;
    if (pp.stream_keys) {  // a batch of Integrator::li calls: the caller's own stream per ray, RandomSampler only
        sm.rng.inc = (pp.stream_keys[p] << 1) | 1;
        sm.rng.state = ps.rng[p];
        sm.pix = 0;
        sm.s = 0;
        sm.dim1 = sm.dim2 = sm.arr = 0;
        sm.h_offset = 0;
        return sm;
    }
    int s_local, pix;
    path_to_sample_pixel(pp, p, &s_local, &pix);
    int2 org = tiles.origin[pix >> 8];
    int x = org.x + (pix & 15), y = org.y + ((pix & 255) >> 4);
    sm.rng.inc = (sample_sequence(pp, x, y, pp.sample0 + s_local) << 1) | 1;
    sm.rng.state = ps.rng[p];
    sm.pix = pix;
    sm.s = pp.sample0 + s_local;
    int c = ps.samp[p];
    sm.dim1 = c & 0x3ff;
    sm.dim2 = (c >> 10) & 0x3f;
    sm.arr = (c >> 16) & 0xffff;
    sm.h_offset = pp.smp.kind == PBRT_SAMPLER_HALTON ? halton_pixel_offset(pp.smp, x, y) : 0;
    return sm;
}

PB_DEV Frame make_frame(const Surf& sf) {  // BSDF::new (reflection.rs:220-234)
    Frame fr;
    fr.ns = sf.ns;
    fr.ng = sf.n;
    fr.ss = normalize(sf.sdpdu);
    fr.ts = cross(fr.ns, fr.ss);
    return fr;
}

// SurfaceInteraction::le (interaction.rs:387-395) -> DiffuseAreaLight::l (diffuse.rs:150-156)
PB_DEV V3 surface_le(const ShadeConsts& sc, const Surf& sf, V3 w) {
    if (sf.light >= 0) {
        DevLight lt = sc.lights[sf.light];
        if (lt.two_sided || dot(sf.n, w) > 0.0f) return V3{lt.L[0], lt.L[1], lt.L[2]};
    }
    return V3{0.0f, 0.0f, 0.0f};
}

}  // namespace pb
