// motion.h — AnimatedTransform::interpolate (src/core/transform.rs:2008-2046) on the device: the side table of a scene with
// moving instances and the per-visit interpolation the traversal kernels' MOV builds run (trace_persistent.h).
//
// The host (host_motion.cpp) decomposes an instance's start and end matrices once, in double, into translation, rotation
// quaternion and the rest (Matrix4x4::decompose, transform.rs:264-330) and rounds the parts to float; the device recomposes
// T(u) R(u) S(u) in float32 per instance visit and inverts the affine 3x4 by cofactors. At or beyond either end of the time
// range interpolate() returns the stored matrix itself, so those rows are kept as they were given (the start ones in the
// slot's seven float4, the end ones here).
#pragma once
#include "dev_math.h"

namespace pb {

struct DevMotion {
    float t[2][3];       // translation at the start / end time
    float r[2][4];       // rotation quaternion (x, y, z, w); r[1] negated when r0 . r1 < 0 (AnimatedTransform::new)
    float s[2][9];       // the rest of the upper 3x3 (scale / shear), row-major
    float end_w2o[12];   // rows 0-2 of the end transform's inverse (computed in double, rounded once) ...
    float end_o2w[12];   // ... and of the end transform itself
    float start_time, end_time;
    int animated;        // 0: the slot's own rows are the instance at every time
    int pad;
};
static_assert(sizeof(DevMotion) == 60 * 4, "DevMotion layout");

// rows 0-2 of an affine transform and of its inverse
struct MotionRows {
    float o2w[12], w2o[12];
};

// Quaternion::slerp (src/core/quaternion.rs, pbrt-v3 Slerp) with the kernels' deterministic acos / sin / cos
PB_DEV void motion_slerp(float u, const float* q0, const float* q1, float* q) {
    const float cos_theta = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
    if (cos_theta > 0.9995f) {
        float l2 = 0.0f;
        for (int k = 0; k < 4; ++k) {
            q[k] = (1.0f - u) * q0[k] + u * q1[k];
            l2 += q[k] * q[k];
        }
        const float len = __builtin_sqrtf(l2);
        for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
        return;
    }
    const float theta = det_acos(clampf(cos_theta, -1.0f, 1.0f));
    const float thetap = theta * u;
    float perp[4], l2 = 0.0f;
    for (int k = 0; k < 4; ++k) {
        perp[k] = q1[k] - q0[k] * cos_theta;
        l2 += perp[k] * perp[k];
    }
    const float len = __builtin_sqrtf(l2);
    float sn, cs;
    det_sincos(thetap, &sn, &cs);
    for (int k = 0; k < 4; ++k) q[k] = q0[k] * cs + (perp[k] / len) * sn;
}

// The instance's rows at `time`, strictly inside (start_time, end_time): lerp T, slerp R, lerp S, compose T R S, invert by
// cofactors. -0 is normalised to +0 in both matrices (x + 0.0f), so that a product with a zero entry has the sign it has in a
// matrix the caller would have written down.
PB_DEV void motion_interpolate(const DevMotion& mo, float time, MotionRows* out) {
    const float u = (time - mo.start_time) / (mo.end_time - mo.start_time);
    float q[4];
    motion_slerp(u, mo.r[0], mo.r[1], q);
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    // Quaternion::to_transform, as the rotation acts on column vectors
    const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - z * w),        2.0f * (x * z + y * w),
                        2.0f * (x * y + z * w),        1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - x * w),
                        2.0f * (x * z - y * w),        2.0f * (y * z + x * w),        1.0f - 2.0f * (x * x + y * y)};
    float S[9];
    for (int k = 0; k < 9; ++k) S[k] = (1.0f - u) * mo.s[0][k] + u * mo.s[1][k];
    float A[9], T[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) A[3 * i + j] = (R[3 * i] * S[j] + R[3 * i + 1] * S[3 + j] + R[3 * i + 2] * S[6 + j]) + 0.0f;
        T[i] = ((1.0f - u) * mo.t[0][i] + u * mo.t[1][i]) + 0.0f;
    }
    // inverse of the upper 3x3: adjugate / determinant; the inverse's translation is -(A^-1 T)
    const float c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const float det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    const float inv_det = 1.0f / det;
    float I[9];
    I[0] = c00 * inv_det;
    I[1] = (A[2] * A[7] - A[1] * A[8]) * inv_det;
    I[2] = (A[1] * A[5] - A[2] * A[4]) * inv_det;
    I[3] = c01 * inv_det;
    I[4] = (A[0] * A[8] - A[2] * A[6]) * inv_det;
    I[5] = (A[2] * A[3] - A[0] * A[5]) * inv_det;
    I[6] = c02 * inv_det;
    I[7] = (A[1] * A[6] - A[0] * A[7]) * inv_det;
    I[8] = (A[0] * A[4] - A[1] * A[3]) * inv_det;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            out->o2w[4 * i + j] = A[3 * i + j];
            out->w2o[4 * i + j] = I[3 * i + j] + 0.0f;
        }
        out->o2w[4 * i + 3] = T[i];
        out->w2o[4 * i + 3] = -(I[3 * i] * T[0] + I[3 * i + 1] * T[1] + I[3 * i + 2] * T[2]) + 0.0f;
    }
}

// The forward rows alone, for a transform that is only ever applied forwards (the animated camera's camera_to_world,
// wf_generate_trace.h): motion_interpolate's arithmetic for o2w, expression by expression, without the inverse.
PB_DEV void motion_interpolate_forward(const DevMotion& mo, float time, float* o2w) {
    const float u = (time - mo.start_time) / (mo.end_time - mo.start_time);
    float q[4];
    motion_slerp(u, mo.r[0], mo.r[1], q);
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - z * w),        2.0f * (x * z + y * w),
                        2.0f * (x * y + z * w),        1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - x * w),
                        2.0f * (x * z - y * w),        2.0f * (y * z + x * w),        1.0f - 2.0f * (x * x + y * y)};
    float S[9];
    for (int k = 0; k < 9; ++k) S[k] = (1.0f - u) * mo.s[0][k] + u * mo.s[1][k];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o2w[4 * i + j] = (R[3 * i] * S[j] + R[3 * i + 1] * S[3 + j] + R[3 * i + 2] * S[6 + j]) + 0.0f;
        o2w[4 * i + 3] = ((1.0f - u) * mo.t[0][i] + u * mo.t[1][i]) + 0.0f;
    }
}

}  // namespace pb
