// curve_kernels.hip — the shading and wavefront-traversal builds for scenes with curve segments (shapes_curve.h), in a
// translation unit of their own: render.hip, which holds every older instantiation of these templates, names none of them and so
// compiles as it did before curves existed (kernel_select.h explains why that matters). It reaches them through the three
// functions below.
#include <hip/hip_runtime.h>

#define PB_PLAIN_KERNEL static __global__  // dev_math.h: the headers' plain kernels are render.hip's; here they are local and dropped
#include "scene.h"
#include "trace.h"
#include "wavefront.h"

#include "curve_kernels.h"

namespace pb {

// k_shade_direct<MODE, 3 + kDirectCurves> and the AO build
DirectKernel curve_direct_kernel(int integrator) {
    static constexpr DirectKernel table[3] = {k_shade_direct<PBRT_INTEGRATOR_DIRECT, 3 + kDirectCurves>,
                                              k_shade_direct<PBRT_INTEGRATOR_WHITTED, 3 + kDirectCurves>,
                                              k_shade_direct<PBRT_INTEGRATOR_AO, kDirectCurves>};
    return table[integrator == PBRT_INTEGRATOR_DIRECT ? 0 : integrator == PBRT_INTEGRATOR_WHITTED ? 1 : 2];
}
// k_shade_curves<BIN>
PathKernel curve_path_kernel(bool bin) {
    static constexpr PathKernel table[2] = {k_shade_curves<true>, k_shade_curves<false>};
    return table[bin ? 0 : 1];
}
// k_trace_curves<COUNT> over one wavefront's ray queue
void launch_trace_curves(bool count, dim3 grid, hipStream_t stream, const DevBVH& bvh, const DevCurve* curves, const PathState& ps,
                         const uint32_t* queue, uint32_t n, unsigned int* work_counter, unsigned long long* counters, int segments) {
    if (count)
        hipLaunchKernelGGL(k_trace_curves<true>, grid, dim3(kTraceBlock), 0, stream, bvh, curves, ps, queue, n, work_counter, counters, segments);
    else
        hipLaunchKernelGGL(k_trace_curves<false>, grid, dim3(kTraceBlock), 0, stream, bvh, curves, ps, queue, n, work_counter, counters, segments);
}

}  // namespace pb
