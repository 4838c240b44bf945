// host_motion.cpp — moving instances on the host (no device code): Matrix4x4::decompose (src/core/transform.rs:264-330,
// after pbrt-v3's AnimatedTransform::Decompose), AnimatedTransform::new's choice of the shorter rotation (transform.rs:870-912),
// the device side table's rows (motion.h) and pbrt_hip_instance_motion_bounds; the animated camera's row, built by the same code,
// and pbrt_hip_camera_motion_interpolate.
//
// The motion bound is NOT AnimatedTransform::motion_bounds / bound_point_motion (transform.rs:913-2084): that one finds the
// roots of the motion's derivative with a thousand lines of precomputed coefficients and, where r0 . r1 >= 0.9995, falls back
// to the union of the end boxes, which a rotating corner leaves. Here a corner p moves on
//   c(u) = T(u) + R(u) S(u) p,  u in [0, 1],
// whose speed is at most  L = |T1 - T0| + w max(|S0 p|, |S1 p|) + |(S1 - S0) p|  with w the bound on the rotation's angular
// speed: 2 theta on the slerp branch (theta = acos(r0 . r1) is the quaternions' angle, the rotation turns twice as far) and
// 4 tan(theta / 2) on the normalised-lerp branch (the chord q0 -> q1 has length 2 sin(theta / 2) and stays at least
// cos(theta / 2) from the origin). [0, 1] is cut into 32 segments; on a segment the corner is never further than L / 64 from the
// nearer of its two end positions, so the box of the two, grown by L / 64, holds it. Everything in double; the result is
// padded for the device's float32 interpolation and rounded outward.
#include "host_motion.h"

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "abi_guard.h"
#include "motion.h"

static_assert(sizeof(PbrtInstanceMotion) == 80 && offsetof(PbrtInstanceMotion, end_to_world) == 0 &&
                  offsetof(PbrtInstanceMotion, start_time) == 64 && offsetof(PbrtInstanceMotion, end_time) == 68 &&
                  offsetof(PbrtInstanceMotion, animated) == 72 && offsetof(PbrtInstanceMotion, pad) == 76,
              "PbrtInstanceMotion layout (include/pbrt_hip.h; pbrt_hip/scenes.py INSTANCE_MOTION_DTYPE)");

static_assert(sizeof(PbrtCameraMotion) == 80 && offsetof(PbrtCameraMotion, end_camera_to_world) == 0 &&
                  offsetof(PbrtCameraMotion, start_time) == 64 && offsetof(PbrtCameraMotion, end_time) == 68 &&
                  offsetof(PbrtCameraMotion, animated) == 72 && offsetof(PbrtCameraMotion, pad) == 76,
              "PbrtCameraMotion layout (include/pbrt_hip.h; pbrt_hip/scenes.py CAMERA_MOTION_DTYPE)");

namespace pb {

namespace {

constexpr int kMotionSegments = 32;

double det3(const double* a) {
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}
// inverse of a 3x3 by cofactors; false when the determinant is zero or not finite
bool inv3(const double* a, double* o) {
    const double d = det3(a);
    if (d == 0.0 || !std::isfinite(d)) return false;
    const double r = 1.0 / d;
    o[0] = (a[4] * a[8] - a[5] * a[7]) * r;
    o[1] = (a[2] * a[7] - a[1] * a[8]) * r;
    o[2] = (a[1] * a[5] - a[2] * a[4]) * r;
    o[3] = (a[5] * a[6] - a[3] * a[8]) * r;
    o[4] = (a[0] * a[8] - a[2] * a[6]) * r;
    o[5] = (a[2] * a[3] - a[0] * a[5]) * r;
    o[6] = (a[3] * a[7] - a[4] * a[6]) * r;
    o[7] = (a[1] * a[6] - a[0] * a[7]) * r;
    o[8] = (a[0] * a[4] - a[1] * a[3]) * r;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(o[k])) return false;
    return true;
}
void mul3(const double* a, const double* b, double* o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
void quat_to_matrix(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - z * w);
    R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);
    R[7] = 2.0 * (y * z + x * w);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}
// Quaternion::from(Transform) (quaternion.rs, pbrt-v3 Quaternion::Quaternion(const Transform&))
void matrix_to_quat(const double* m, double* q) {
    const double trace = m[0] + m[4] + m[8];
    if (trace > 0.0) {
        double s = std::sqrt(trace + 1.0);
        q[3] = s / 2.0;
        s = 0.5 / s;
        q[0] = (m[7] - m[5]) * s;
        q[1] = (m[2] - m[6]) * s;
        q[2] = (m[3] - m[1]) * s;
    } else {
        const int nxt[3] = {1, 2, 0};
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = nxt[i], k = nxt[j];
        double s = std::sqrt((m[4 * i] - (m[4 * j] + m[4 * k])) + 1.0);
        q[i] = s * 0.5;
        if (s != 0.0) s = 0.5 / s;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * s;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * s;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * s;
    }
}
// the quaternion AnimatedTransform::interpolate uses at u, by the device's branch rule (motion.h), in double
void slerp(double u, const double* q0, const double* q1, double* q) {
    const double c = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
    double l2 = 0.0;
    if (c > 0.9995) {
        for (int k = 0; k < 4; ++k) {
            q[k] = (1.0 - u) * q0[k] + u * q1[k];
            l2 += q[k] * q[k];
        }
        for (int k = 0; k < 4; ++k) q[k] /= std::sqrt(l2);
        return;
    }
    const double theta = std::acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
    double perp[4];
    for (int k = 0; k < 4; ++k) {
        perp[k] = q1[k] - q0[k] * c;
        l2 += perp[k] * perp[k];
    }
    for (int k = 0; k < 4; ++k) q[k] = q0[k] * std::cos(theta * u) + perp[k] / std::sqrt(l2) * std::sin(theta * u);
}
const char* matrix_invalid(const float* m) {
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return "a non-finite matrix entry";
    if (m[12] != 0.0f || m[13] != 0.0f || m[14] != 0.0f || m[15] != 1.0f) return "a matrix that is not affine (last row 0 0 0 1)";
    return nullptr;
}

float round_down(double v) {
    float f = (float)v;
    return (double)f > v ? std::nextafterf(f, -INFINITY) : f;
}
float round_up(double v) {
    float f = (float)v;
    return (double)f < v ? std::nextafterf(f, INFINITY) : f;
}

}  // namespace

const char* motion_decompose(const float m[16], MotionParts* out) {
    if (const char* why = matrix_invalid(m)) return why;
    double M[9], R[9];
    for (int i = 0; i < 3; ++i) {
        out->t[i] = m[4 * i + 3];
        for (int j = 0; j < 3; ++j) M[3 * i + j] = R[3 * i + j] = m[4 * i + j];
    }
    double tmp[9];
    if (!inv3(M, tmp)) return "a singular matrix";
    // polar decomposition: R <- (R + (R^T)^-1) / 2 until the step's largest row sum is at most 1e-4, 100 steps at the most
    double norm;
    int count = 0;
    do {
        double inv[9], next[9];
        if (!inv3(R, inv)) return "a singular matrix";
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) next[3 * i + j] = 0.5 * (R[3 * i + j] + inv[3 * j + i]);
        norm = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double n = std::fabs(R[3 * i] - next[3 * i]) + std::fabs(R[3 * i + 1] - next[3 * i + 1]) + std::fabs(R[3 * i + 2] - next[3 * i + 2]);
            norm = n > norm ? n : norm;
        }
        std::memcpy(R, next, sizeof(R));
    } while (++count < 100 && norm > 1e-4);
    matrix_to_quat(R, out->q);
    double Rinv[9];
    if (!inv3(R, Rinv)) return "a singular matrix";
    mul3(Rinv, M, out->s);  // S = R^-1 M
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(out->q[k])) return "a matrix without a rotation part";
    return nullptr;
}

const char* motion_parts(const float start[16], const float end[16], float start_time, float end_time, MotionParts* p0, MotionParts* p1) {
    if (!std::isfinite(start_time) || !std::isfinite(end_time)) return "a non-finite start or end time";
    if (!(end_time > start_time)) return "end_time <= start_time";
    if (const char* why = motion_decompose(start, p0)) return why;
    if (const char* why = motion_decompose(end, p1)) return why;
    const double d = p0->q[0] * p1->q[0] + p0->q[1] * p1->q[1] + p0->q[2] * p1->q[2] + p0->q[3] * p1->q[3];
    if (d < 0.0)
        for (int k = 0; k < 4; ++k) p1->q[k] = -p1->q[k];
    return nullptr;
}

const char* motion_parts(const PbrtInstance& inst, const PbrtInstanceMotion& mo, MotionParts* p0, MotionParts* p1) {
    return motion_parts(inst.to_world, mo.end_to_world, mo.start_time, mo.end_time, p0, p1);
}

namespace {
// the row of a transform animated from `start` to `end_to_world`, for instances and the camera alike
const char* animated_row(const float start[16], const float end_to_world[16], float start_time, float end_time, DevMotion* row) {
    MotionParts p[2];
    if (const char* why = motion_parts(start, end_to_world, start_time, end_time, &p[0], &p[1])) return why;
    for (int e = 0; e < 2; ++e) {
        for (int k = 0; k < 3; ++k) row->t[e][k] = (float)p[e].t[k];
        for (int k = 0; k < 4; ++k) row->r[e][k] = (float)p[e].q[k];
        for (int k = 0; k < 9; ++k) row->s[e][k] = (float)p[e].s[k];
    }
    // the end transform's rows as given, and its inverse in double, rounded once
    double M[9], I[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = end_to_world[4 * i + j];
    if (!inv3(M, I)) return "a singular matrix";
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) row->end_o2w[4 * i + j] = end_to_world[4 * i + j];
        for (int j = 0; j < 3; ++j) row->end_w2o[4 * i + j] = (float)I[3 * i + j] + 0.0f;
        const double t = -(I[3 * i] * (double)end_to_world[3] + I[3 * i + 1] * (double)end_to_world[7] + I[3 * i + 2] * (double)end_to_world[11]);
        row->end_w2o[4 * i + 3] = (float)t + 0.0f;
    }
    row->start_time = start_time;
    row->end_time = end_time;
    row->animated = 1;
    return nullptr;
}
}  // namespace

const char* motion_row(const PbrtInstance& inst, const PbrtInstanceMotion& mo, DevMotion* row) {
    std::memset(row, 0, sizeof(*row));
    if (!mo.animated) return nullptr;
    return animated_row(inst.to_world, mo.end_to_world, mo.start_time, mo.end_time, row);
}

const char* camera_motion_row(const PbrtCamera& camera, const PbrtCameraMotion& mo, DevMotion* row) {
    std::memset(row, 0, sizeof(*row));
    if (!mo.animated) return nullptr;
    return animated_row(camera.camera_to_world, mo.end_camera_to_world, mo.start_time, mo.end_time, row);
}

}  // namespace pb

extern "C" int pbrt_hip_instance_bounds(const float object_min[3], const float object_max[3], const PbrtInstance* instances,
                                        int32_t n_instances, float* bounds_min, float* bounds_max);

extern "C" int pbrt_hip_instance_motion_bounds(const float object_min[3], const float object_max[3], const PbrtInstance* instances,
                                               const PbrtInstanceMotion* motions, int32_t n_instances, float* bounds_min,
                                               float* bounds_max) try {
    using namespace pb;
    if (!object_min || !object_max || n_instances < 0 || (n_instances > 0 && (!instances || !bounds_min || !bounds_max)))
        return PBRT_HIP_ERR_INVALID;
    for (int32_t i = 0; i < n_instances; ++i) {
        float* lo = bounds_min + 3 * (size_t)i;
        float* hi = bounds_max + 3 * (size_t)i;
        int rc = pbrt_hip_instance_bounds(object_min, object_max, instances + i, 1, lo, hi);
        if (rc != PBRT_HIP_OK) return rc;
        if (!motions || !motions[i].animated) continue;
        MotionParts p0, p1;
        if (motion_parts(instances[i], motions[i], &p0, &p1)) return PBRT_HIP_ERR_INVALID;
        // the end box, exactly as pbrt_hip_instance_bounds evaluates it; with equal rotations the union of the two is the bound
        PbrtInstance end = instances[i];
        std::memcpy(end.to_world, motions[i].end_to_world, 64);
        float elo[3], ehi[3];
        rc = pbrt_hip_instance_bounds(object_min, object_max, &end, 1, elo, ehi);
        if (rc != PBRT_HIP_OK) return rc;
        for (int k = 0; k < 3; ++k) {
            lo[k] = elo[k] < lo[k] ? elo[k] : lo[k];
            hi[k] = ehi[k] > hi[k] ? ehi[k] : hi[k];
        }
        if (p0.q[0] == p1.q[0] && p0.q[1] == p1.q[1] && p0.q[2] == p1.q[2] && p0.q[3] == p1.q[3]) continue;
        // rotation present: the segment bound
        const double c = p0.q[0] * p1.q[0] + p0.q[1] * p1.q[1] + p0.q[2] * p1.q[2] + p0.q[3] * p1.q[3];
        const double theta = std::acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
        const double omega = c > 0.9995 ? 4.0 * std::tan(0.5 * theta) : 2.0 * theta;
        const double dT = std::sqrt((p1.t[0] - p0.t[0]) * (p1.t[0] - p0.t[0]) + (p1.t[1] - p0.t[1]) * (p1.t[1] - p0.t[1]) +
                                    (p1.t[2] - p0.t[2]) * (p1.t[2] - p0.t[2]));
        // R(u) S(u) and T(u) at the 33 segment ends
        double A[kMotionSegments + 1][9], T[kMotionSegments + 1][3];
        for (int s = 0; s <= kMotionSegments; ++s) {
            const double u = (double)s / kMotionSegments;
            double q[4], R[9], S[9];
            slerp(u, p0.q, p1.q, q);
            quat_to_matrix(q, R);
            for (int k = 0; k < 9; ++k) S[k] = (1.0 - u) * p0.s[k] + u * p1.s[k];
            mul3(R, S, A[s]);
            for (int k = 0; k < 3; ++k) T[s][k] = (1.0 - u) * p0.t[k] + u * p1.t[k];
        }
        double mn[3] = {lo[0], lo[1], lo[2]}, mx[3] = {hi[0], hi[1], hi[2]};
        for (int corner = 0; corner < 8; ++corner) {
            const double p[3] = {(corner & 1) ? object_max[0] : object_min[0], (corner & 2) ? object_max[1] : object_min[1],
                                 (corner & 4) ? object_max[2] : object_min[2]};
            double l0 = 0.0, l1 = 0.0, ld = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double a = p0.s[3 * r] * p[0] + p0.s[3 * r + 1] * p[1] + p0.s[3 * r + 2] * p[2];
                const double b = p1.s[3 * r] * p[0] + p1.s[3 * r + 1] * p[1] + p1.s[3 * r + 2] * p[2];
                l0 += a * a;
                l1 += b * b;
                ld += (b - a) * (b - a);
            }
            const double L = dT + omega * std::sqrt(l0 > l1 ? l0 : l1) + std::sqrt(ld);
            const double grow = L / (2.0 * kMotionSegments);
            for (int s = 0; s <= kMotionSegments; ++s)  // every segment end belongs to a segment: its position, grown
                for (int r = 0; r < 3; ++r) {
                    const double v = A[s][3 * r] * p[0] + A[s][3 * r + 1] * p[1] + A[s][3 * r + 2] * p[2] + T[s][r];
                    mn[r] = v - grow < mn[r] ? v - grow : mn[r];
                    mx[r] = v + grow > mx[r] ? v + grow : mx[r];
                }
        }
        // the device interpolates in float32: 16 ulps of the largest coordinate on every side, then outward to float
        double big = 0.0;
        for (int k = 0; k < 3; ++k) {
            big = std::fabs(mn[k]) > big ? std::fabs(mn[k]) : big;
            big = std::fabs(mx[k]) > big ? std::fabs(mx[k]) : big;
        }
        const double pad = 16.0 * 5.9604644775390625e-08 * big;
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(mn[k]) || !std::isfinite(mx[k])) return PBRT_HIP_ERR_INVALID;
            lo[k] = round_down(mn[k] - pad);
            hi[k] = round_up(mx[k] + pad);
        }
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// AnimatedTransform::interpolate (transform.rs:2010-2030) of the camera's two matrices, in double, rounded once
extern "C" int pbrt_hip_camera_motion_interpolate(const PbrtCamera* camera, const PbrtCameraMotion* motion, float time,
                                                  float out_camera_to_world[16]) try {
    using namespace pb;
    if (!camera || !out_camera_to_world) return PBRT_HIP_ERR_INVALID;
    if (!motion || !motion->animated) {
        std::memcpy(out_camera_to_world, camera->camera_to_world, 64);
        return PBRT_HIP_OK;
    }
    MotionParts p0, p1;
    if (const char* why = motion_parts(camera->camera_to_world, motion->end_camera_to_world, motion->start_time, motion->end_time, &p0, &p1)) {
        set_thread_error(std::string("camera motion: ") + why);
        return PBRT_HIP_ERR_INVALID;
    }
    if (!std::isfinite(time)) {
        set_thread_error("camera motion: a non-finite time");
        return PBRT_HIP_ERR_INVALID;
    }
    if (time <= motion->start_time) {
        std::memcpy(out_camera_to_world, camera->camera_to_world, 64);
        return PBRT_HIP_OK;
    }
    if (time >= motion->end_time) {
        std::memcpy(out_camera_to_world, motion->end_camera_to_world, 64);
        return PBRT_HIP_OK;
    }
    const double u = ((double)time - (double)motion->start_time) / ((double)motion->end_time - (double)motion->start_time);
    double q[4], R[9], S[9], A[9];
    slerp(u, p0.q, p1.q, q);
    quat_to_matrix(q, R);
    for (int k = 0; k < 9; ++k) S[k] = (1.0 - u) * p0.s[k] + u * p1.s[k];
    mul3(R, S, A);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out_camera_to_world[4 * i + j] = (float)A[3 * i + j];
        out_camera_to_world[4 * i + 3] = (float)((1.0 - u) * p0.t[i] + u * p1.t[i]);
    }
    out_camera_to_world[12] = out_camera_to_world[13] = out_camera_to_world[14] = 0.0f;
    out_camera_to_world[15] = 1.0f;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH
