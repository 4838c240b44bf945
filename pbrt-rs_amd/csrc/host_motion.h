// host_motion.h — moving instances on the host: Matrix4x4::decompose, the checks scene creation makes on a PbrtInstanceMotion,
// and the device side table's row (motion.h); the same for an animated camera_to_world (PbrtCameraMotion). Implemented in
// host_motion.cpp, in double precision.
#pragma once
#include <string>

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
// The same for any pair of matrices over [start_time, end_time]: what the instance form above and the animated camera share.
const char* motion_parts(const float start[16], const float end[16], float start_time, float end_time, MotionParts* p0, MotionParts* p1);
// The side table's row of one instance (animated or not). nullptr, or the refusal.
const char* motion_row(const PbrtInstance& inst, const PbrtInstanceMotion& mo, DevMotion* row);
// The row of an animated camera_to_world (PbrtCamera.camera_to_world at start_time; the generator reads the forward half only).
// nullptr, or what pbrt_hip_render_moving_camera refuses the motion for.
const char* camera_motion_row(const PbrtCamera& camera, const PbrtCameraMotion& mo, DevMotion* row);
// The message pbrt_hip_last_error(NULL) returns to the calling thread (pbrt_hip.hip): for entry points that take no context.
void set_thread_error(const std::string& message);

}  // namespace pb
