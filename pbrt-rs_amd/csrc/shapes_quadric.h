// shapes_quadric.h — Sphere, Disk and Cylinder under a general affine transform (included at the end of trace.h).
//
// Hit tests of src/shapes/sphere.rs:228-284 (partial sweeps included), src/shapes/disk.rs:42-73 and
// src/shapes/cylinder.rs:41-88 on the object-space ray of Ray::from((world_to_object, r, o_err, d_err))
// (src/core/geometry.rs:1077-1096), in the operation order of sphere_object_ray / sphere_test (trace.h), so that a full
// sphere under translate(c) gives the hit record of the translated-sphere path bit for bit: with -ffp-contract=off every
// product of the general formula with a 0 or 1 entry is exact. The surface past the hit test is in wf_surface.h
// (make_surface_shape), the shapes as area lights in wf_lights.h.
#pragma once

namespace pb {

constexpr int kShapeSphere = 0, kShapeDisk = 1, kShapeCylinder = 2;  // PbrtShapeType
constexpr int kShapeTypeMask = 3;
constexpr int kShapeFlipNormal = 4;  // reverse_orientation ^ transform_swaps_handedness: SurfaceInteraction::new flips n, and so
                                     // does the shape's sampling as an area light (D85)

// One row per shape (DevBVH::shapes). theta_min / theta_max are filled on the device (k_shape_angles: the kernels' own acos).
struct DevShape {
    float w2o[12];  // world_to_object rows 0-2
    float o2w[12];  // object_to_world rows 0-2
    float radius, z_min, z_max;  // disk: z_min = height
    float theta_min, theta_max;  // sphere (Sphere::new, sphere.rs:222-223)
    float phi_max;               // radians
    float inner_radius;          // disk
    int flags;                   // type | kShapeFlipNormal
    // the z range the hit test rejects against: the cylinder's [z_min, z_max]; a sphere tests a side only where it is short of
    // the pole (sphere.rs:273-274), so a side that reaches the pole is -inf / +inf here
    float z_clip_min, z_clip_max;
};

// Ray::from((world_to_object, r, &mut o_err, &mut d_err)) for an affine 3x4 `m` (rows), with the origin pushed along d
// past its error bound (geometry.rs:1089-1093); sphere_object_ray is this with the entries of translate(-c) as literals
PB_DEV SphereRay shape_object_ray(const float* m, const TravRay& r) {
    SphereRay q;
    float x = r.ox, y = r.oy, z = r.oz;
    q.ox = m[0] * x + m[1] * y + m[2] * z + m[3];
    q.oy = m[4] * x + m[5] * y + m[6] * z + m[7];
    q.oz = m[8] * x + m[9] * y + m[10] * z + m[11];
    q.oex = (__builtin_fabsf(m[0] * x) + __builtin_fabsf(m[1] * y) + __builtin_fabsf(m[2] * z) + __builtin_fabsf(m[3])) * kGamma3;
    q.oey = (__builtin_fabsf(m[4] * x) + __builtin_fabsf(m[5] * y) + __builtin_fabsf(m[6] * z) + __builtin_fabsf(m[7])) * kGamma3;
    q.oez = (__builtin_fabsf(m[8] * x) + __builtin_fabsf(m[9] * y) + __builtin_fabsf(m[10] * z) + __builtin_fabsf(m[11])) * kGamma3;
    float dx = r.dx, dy = r.dy, dz = r.dz;
    q.dex = (__builtin_fabsf(m[0] * dx) + __builtin_fabsf(m[1] * dy) + __builtin_fabsf(m[2] * dz)) * kGamma3;
    q.dey = (__builtin_fabsf(m[4] * dx) + __builtin_fabsf(m[5] * dy) + __builtin_fabsf(m[6] * dz)) * kGamma3;
    q.dez = (__builtin_fabsf(m[8] * dx) + __builtin_fabsf(m[9] * dy) + __builtin_fabsf(m[10] * dz)) * kGamma3;
    q.dx = m[0] * dx + m[1] * dy + m[2] * dz;
    q.dy = m[4] * dx + m[5] * dy + m[6] * dz;
    q.dz = m[8] * dx + m[9] * dy + m[10] * dz;
    float l2 = q.dx * q.dx + q.dy * q.dy + q.dz * q.dz;
    if (l2 > 0.0f) {
        float dt = (__builtin_fabsf(q.dx) * q.oex + __builtin_fabsf(q.dy) * q.oey + __builtin_fabsf(q.dz) * q.oez) / l2;
        q.ox += q.dx * dt;
        q.oy += q.dy * dt;
        q.oz += q.dz * dt;
    }
    return q;
}

// Sphere::intersect_test (sphere.rs:228-284, partial spheres included) and Cylinder::compute_intersect (cylinder.rs:41-88) in
// one body: the cylinder's quadratic is the sphere's without the z terms, and EFloat sums associate to the left, so the x / y
// partial sums are the cylinder's coefficients and the sphere adds its z term to each. One body, not two behind a branch: the
// traversal kernel holds one set of interval registers at its four-waves launch bound.
PB_DEV bool quadric_round_test(const DevShape& sh, const SphereRay& q, bool sphere, float tmax, float* t_out, V3* p_hit) {
    const float radius = sh.radius;
    EFloat ox = ef_make(q.ox, q.oex), oy = ef_make(q.oy, q.oey);
    EFloat dx = ef_make(q.dx, q.dex), dy = ef_make(q.dy, q.dey);
    EFloat a = ef_add(ef_mul(dx, dx), ef_mul(dy, dy));
    EFloat b = ef_add(ef_mul(dx, ox), ef_mul(dy, oy));
    EFloat c = ef_add(ef_mul(ox, ox), ef_mul(oy, oy));
    if (sphere) {
        EFloat oz = ef_make(q.oz, q.oez), dz = ef_make(q.dz, q.dez);
        a = ef_add(a, ef_mul(dz, dz));
        b = ef_add(b, ef_mul(dz, oz));
        c = ef_add(c, ef_mul(oz, oz));
    }
    b = ef_mulf(b, 2.0f);
    EFloat rr = ef_make(radius, 0.0f);
    c = ef_sub(c, ef_mul(rr, rr));
    EFloat t0, t1;
    if (!ef_quadratic(a, b, c, &t0, &t1)) return false;
    for (int k = 0; k < 2; ++k) {  // sphere.rs:259-281, cylinder.rs:67-85: the nearer root, then the farther one
        EFloat t = k == 0 ? t0 : t1;
        // sphere.rs:261 rejects lower_bound() < 0, cylinder.rs:68 lower_bound() <= 0
        if (t.low < 0.0f || (!sphere && t.low == 0.0f) || t.high > tmax) continue;
        V3 ph = V3{q.ox + q.dx * t.v, q.oy + q.dy * t.v, q.oz + q.dz * t.v};
        // sphere.rs:265: p_hit *= radius / |p_hit|; cylinder.rs:72-74: the same in x / y alone (x^2 + y^2 + 0 is exact)
        float scale = radius / __builtin_sqrtf(ph.x * ph.x + ph.y * ph.y + (sphere ? ph.z * ph.z : 0.0f));
        ph = V3{ph.x * scale, ph.y * scale, sphere ? ph.z * scale : ph.z};
        if (sphere && ph.x == 0.0f && ph.y == 0.0f) ph.x = 1e-5f * radius;
        float phi = det_atan2(ph.y, ph.x);
        if (phi < 0.0f) phi += 2.0f * kPi;
        if (ph.z < sh.z_clip_min || ph.z > sh.z_clip_max || phi > sh.phi_max) continue;
        *t_out = t.v;
        *p_hit = ph;
        return true;
    }
    return false;
}

// Disk::intersect_test (disk.rs:42-73): the plane z = height, no EFloat
PB_DEV bool quadric_disk_test(const DevShape& sh, const SphereRay& q, float tmax, float* t_out, V3* p_hit) {
    if (q.dz == 0.0f) return false;
    float t = (sh.z_min - q.oz) / q.dz;
    if (t <= 0.0f || t >= tmax) return false;
    V3 ph = V3{q.ox + q.dx * t, q.oy + q.dy * t, q.oz + q.dz * t};
    float dist2 = ph.x * ph.x + ph.y * ph.y;
    if (dist2 > sh.radius * sh.radius || dist2 < sh.inner_radius * sh.inner_radius) return false;
    // the centre (a ray down the axis): dpdv = p (r_i - r) / |p| is 0 / 0 there (disk.rs:98-101 divides all the same); the
    // sphere's nudge at its pole, so that the hit keeps the tangent of phi = 0 (D94). No other hit's bits change.
    if (ph.x == 0.0f && ph.y == 0.0f) ph.x = 1e-5f * sh.radius;
    float phi = det_atan2(ph.y, ph.x);
    if (phi < 0.0f) phi += 2.0f * kPi;
    if (phi > sh.phi_max) return false;
    *t_out = t;
    *p_hit = ph;
    return true;
}

// Shape::intersect / intersect_p up to the hit record: t and the (refined) object-space hit point; tmax is the world ray's
PB_DEV bool shape_test(const DevShape& sh, const TravRay& r, float tmax, float* t_out, V3* p_hit) {
    const int type = sh.flags & kShapeTypeMask;
    SphereRay q = shape_object_ray(sh.w2o, r);
    if (type != kShapeDisk) return quadric_round_test(sh, q, type == kShapeSphere, tmax, t_out, p_hit);
    return quadric_disk_test(sh, q, tmax, t_out, p_hit);
}

}  // namespace pb
