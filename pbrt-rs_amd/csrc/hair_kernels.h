// hair_kernels.h — what hair_kernels.hip gives the render driver: the shading kernels of a scene with curves whose material table
// holds a hair row (needs wavefront.h and curve_kernels.h's kernel types)
#pragma once

namespace pb {

DirectKernel hair_direct_kernel(bool whitted);  // PBRT_INTEGRATOR_DIRECT / _WHITTED (AO reads no BSDF: curve_direct_kernel)
PathKernel hair_path_kernel(bool bin);

}  // namespace pb
