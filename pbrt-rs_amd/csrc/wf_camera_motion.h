// wf_camera_motion.h — k_generate_moving_camera: the camera-ray generator for an animated camera_to_world (part of wavefront.h)
#pragma once
#include "wf_film.h"

namespace pb {

// Defined after every other kernel of the wavefront headers and named in kernel_select.h behind every older table: the code
// generated for some of the older kernels depends on the order in which the instantiations are met.
// One build serves static and moving scenes alike: it always writes the ray's time, which the static scenes' kernels never read.
// The camera's DevMotion row (host_motion.cpp: camera_motion_row) rides in the arguments.
PB_PLAIN_KERNEL void k_generate_moving_camera(PathState ps, Queues q, PassParams pp, DevCamera cam, DevMotion cmo, TileList tiles) {
    generate_camera_rays<true, true>(ps, q, pp, cam, tiles, &cmo);
}

}  // namespace pb
