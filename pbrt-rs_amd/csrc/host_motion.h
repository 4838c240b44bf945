// host_motion.h — moving instances on the host: Matrix4x4::decompose, the checks scene creation makes on a PbrtInstanceMotion,
// and the device side table's row (motion.h). Implemented in host_motion.cpp, in double precision.
#pragma once
#include "../../include/pbrt_hip.h"

namespace pb {

struct DevMotion;

// translation, rotation quaternion (x, y, z, w) and the rest of the upper 3x3 (row-major) of an affine matrix
struct MotionParts {
    double t[3], q[4], s[9];
};
// Matrix4x4::decompose (src/core/transform.rs:264-330, after pbrt-v3's AnimatedTransform::Decompose). nullptr, or why not.
const char* motion_decompose(const float m[16], MotionParts* out);
// Both decompositions of an animated instance, the end quaternion negated when the two have a negative dot product
// (AnimatedTransform::new). nullptr, or what pbrt_hip_scene_create_two_level_moving refuses the instance for.
const char* motion_parts(const PbrtInstance& inst, const PbrtInstanceMotion& mo, MotionParts* p0, MotionParts* p1);
// The side table's row of one instance (animated or not). nullptr, or the refusal.
const char* motion_row(const PbrtInstance& inst, const PbrtInstanceMotion& mo, DevMotion* row);

}  // namespace pb
