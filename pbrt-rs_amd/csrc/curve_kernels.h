// curve_kernels.h — what curve_kernels.hip gives the render driver: the shading kernels and the traversal launch of scenes with
// curve segments (needs wavefront.h)
#pragma once

namespace pb {

using DirectKernel = void (*)(ShadeConsts, PathState, DirectState, Queues, Queues, PassParams, TileList, uint32_t);
using PathKernel = void (*)(ShadeConsts, PathState, Queues, Queues, PassParams, TileList, uint32_t, const uint32_t*);

DirectKernel curve_direct_kernel(int integrator);  // PBRT_INTEGRATOR_DIRECT / _WHITTED / _AO
PathKernel curve_path_kernel(bool bin);
void launch_trace_curves(bool count, dim3 grid, hipStream_t stream, const DevBVH& bvh, const DevCurve* curves, const PathState& ps,
                         const uint32_t* queue, uint32_t n, unsigned int* work_counter, unsigned long long* counters, int segments);

}  // namespace pb
