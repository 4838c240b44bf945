// hair_kernels.hip — the shading builds for scenes with curve segments whose material table holds a hair row (wf_hair.h), and the
// hair row's BSDF query, in a translation unit of their own: render.hip and curve_kernels.hip, which hold every older
// instantiation of these templates, name none of them and never include wf_hair.h, so they compile as they did before hair rows
// existed (kernel_select.h explains why that matters; profiles/hair_resource_usage.txt compares).
#include <hip/hip_runtime.h>
#include "abi_guard.h"

#define PB_PLAIN_KERNEL static __global__  // dev_math.h: the headers' plain kernels are render.hip's; here they are local and dropped
#include "scene.h"
#include "trace.h"
#include "wavefront.h"
#include "wf_hair.h"

#include "curve_kernels.h"
#include "hair_kernels.h"
#include "point_query.h"

namespace pb {

// k_shade_direct<MODE, 3 + kDirectCurves + kDirectHair>
DirectKernel hair_direct_kernel(bool whitted) {
    static constexpr DirectKernel table[2] = {k_shade_direct<PBRT_INTEGRATOR_DIRECT, 3 + kDirectCurves + kDirectHair>,
                                              k_shade_direct<PBRT_INTEGRATOR_WHITTED, 3 + kDirectCurves + kDirectHair>};
    return table[whitted ? 1 : 0];
}
// k_shade_hair<BIN>
PathKernel hair_path_kernel(bool bin) {
    static constexpr PathKernel table[2] = {k_shade_hair<true>, k_shade_hair<false>};
    return table[bin ? 0 : 1];
}

// BSDF::f / pdf / sample_f of a hair row in the shading frame (ns = ng = +z, dpdu = +x: the fibre runs along x), evaluated by the
// functions the hair builds inline, with the offset across the fibre given per point. out: 12 floats per query, as k_bsdf_query's.
__global__ void k_bsdf_query_hair(const DevHair* __restrict__ hr, int64_t n, const float* __restrict__ h_in, const float* __restrict__ wo_in,
                                  const float* __restrict__ wi_in, const float* __restrict__ u_in, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Frame fr = query_frame();
    const V3 wo = query_v3(wo_in, i), wi = query_v3(wi_in, i);
    const float h = h_in[i];
    V3 f, wi_s = V3{0.0f, 0.0f, 0.0f}, f_s = wi_s;
    float pdf, pdf_s = 0.0f;
    int sampled = 0;
    hair_f_pdf(hr, h, fr, wo, wi, &f, &pdf);
    bool ok;
    float ps = 0.0f;
    V3 w;
    V3 fs = hair_sample_f(hr, h, fr, wo, u_in[2 * i], u_in[2 * i + 1], &w, &ps, &ok);
    if (ok) {
        wi_s = w;
        f_s = fs;
        pdf_s = ps;
        sampled = kBxdfGlossy | kBxdfReflection | kBxdfTransmission;
    }
    query_write(out, i, f, pdf, wi_s, f_s, pdf_s, sampled);
}

}  // namespace pb

using namespace pb;

extern "C" int pbrt_hip_bsdf_query_hair(PbrtHipScene* s, int32_t material, int64_t n, const float* h, const float* wo, const float* wi,
                                        const float* u, float* f, float* pdf, float* wi_s, float* f_s, float* pdf_s,
                                        int32_t* sampled_flags) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(s->ctx);
    const size_t un = (size_t)n;
    return bsdf_query(
        s, "pbrt_hip_bsdf_query_hair", true, material, n, {{wo, 3}, {wi, 3}, {u, 2}, {h, 1}}, "null h / wo / wi / u", "k_bsdf_query_hair",
        [&](const float* d_in, float* d_out) {
            hipLaunchKernelGGL(k_bsdf_query_hair, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->ctx->stream,
                               (const DevHair*)(s->d.disney + material), n, d_in + 8 * un, d_in, d_in + 3 * un, d_in + 6 * un, d_out);
        },
        BsdfQueryOut{f, pdf, wi_s, f_s, pdf_s, sampled_flags});
}
PB_ABI_CATCH
