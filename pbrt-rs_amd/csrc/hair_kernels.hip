// hair_kernels.hip — the shading builds for scenes with curve segments whose material table holds a hair row (wf_hair.h), and the
// hair row's BSDF query, in a translation unit of their own: render.hip and curve_kernels.hip, which hold every older
// instantiation of these templates, name none of them and never include wf_hair.h, so they compile as they did before hair rows
// existed (kernel_select.h explains why that matters; profiles/hair_resource_usage.txt compares).
#include <hip/hip_runtime.h>
#include "abi_guard.h"

#include <cstring>
#include <string>
#include <vector>

#define PB_PLAIN_KERNEL static __global__  // dev_math.h: the headers' plain kernels are render.hip's; here they are local and dropped
#include "scene.h"
#include "trace.h"
#include "wavefront.h"
#include "wf_hair.h"

#include "curve_kernels.h"
#include "hair_kernels.h"

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
    Frame fr;
    fr.ss = V3{1.0f, 0.0f, 0.0f};
    fr.ts = V3{0.0f, 1.0f, 0.0f};
    fr.ns = V3{0.0f, 0.0f, 1.0f};
    fr.ng = fr.ns;
    const V3 wo = V3{wo_in[3 * i], wo_in[3 * i + 1], wo_in[3 * i + 2]};
    const V3 wi = V3{wi_in[3 * i], wi_in[3 * i + 1], wi_in[3 * i + 2]};
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
    float* o = out + 12 * i;
    o[0] = f.x;
    o[1] = f.y;
    o[2] = f.z;
    o[3] = pdf;
    o[4] = wi_s.x;
    o[5] = wi_s.y;
    o[6] = wi_s.z;
    o[7] = f_s.x;
    o[8] = f_s.y;
    o[9] = f_s.z;
    o[10] = pdf_s;
    o[11] = __int_as_float(sampled);
}

}  // namespace pb

using namespace pb;

extern "C" int pbrt_hip_bsdf_query_hair(PbrtHipScene* s, int32_t material, int64_t n, const float* h, const float* wo, const float* wi,
                                        const float* u, float* f, float* pdf, float* wi_s, float* f_s, float* pdf_s,
                                        int32_t* sampled_flags) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const char* why) {
        ctx->last_error = std::string("pbrt_hip_bsdf_query_hair: ") + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (material < 0 || material >= s->d.n_materials) return invalid("material index out of range");
    if (s->h_materials[material].type != kMatHair) return invalid("the row is not a hair row (pbrt_hip_bsdf_query serves every other row)");
    if (n < 0 || n > ((int64_t)1 << 31)) return invalid("n must be in [0, 2^31]");
    if (n == 0) return PBRT_HIP_OK;
    if (!h || !wo || !wi || !u) return invalid("null h / wo / wi / u");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t un = (size_t)n;
    float *d_in = nullptr, *d_out = nullptr;
    int rc = PBRT_HIP_OK;
    if (!hip_ok(ctx, hipMalloc((void**)&d_in, un * 9 * sizeof(float)), "hipMalloc") ||
        !hip_ok(ctx, hipMalloc((void**)&d_out, un * 12 * sizeof(float)), "hipMalloc"))
        rc = PBRT_HIP_ERR_OOM;
    if (rc == PBRT_HIP_OK && (!hip_ok(ctx, hipMemcpy(d_in, wo, un * 3 * sizeof(float), hipMemcpyHostToDevice), "H2D") ||
                              !hip_ok(ctx, hipMemcpy(d_in + 3 * un, wi, un * 3 * sizeof(float), hipMemcpyHostToDevice), "H2D") ||
                              !hip_ok(ctx, hipMemcpy(d_in + 6 * un, u, un * 2 * sizeof(float), hipMemcpyHostToDevice), "H2D") ||
                              !hip_ok(ctx, hipMemcpy(d_in + 8 * un, h, un * sizeof(float), hipMemcpyHostToDevice), "H2D")))
        rc = PBRT_HIP_ERR_DEVICE;
    std::vector<float> res;
    if (rc == PBRT_HIP_OK) {
        hipLaunchKernelGGL(k_bsdf_query_hair, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const DevHair*)(s->d.disney + material), n, d_in + 8 * un, d_in, d_in + 3 * un, d_in + 6 * un, d_out);
        res.resize(un * 12);
        if (!hip_ok(ctx, hipGetLastError(), "k_bsdf_query_hair") || !hip_ok(ctx, hipStreamSynchronize(ctx->stream), "k_bsdf_query_hair") ||
            !hip_ok(ctx, hipMemcpy(res.data(), d_out, un * 12 * sizeof(float), hipMemcpyDeviceToHost), "D2H"))
            rc = PBRT_HIP_ERR_DEVICE;
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (rc != PBRT_HIP_OK) return rc;
    for (size_t i = 0; i < un; ++i) {
        const float* o = &res[12 * i];
        for (int k = 0; k < 3; ++k) {
            if (f) f[3 * i + k] = o[k];
            if (wi_s) wi_s[3 * i + k] = o[4 + k];
            if (f_s) f_s[3 * i + k] = o[7 + k];
        }
        if (pdf) pdf[i] = o[3];
        if (pdf_s) pdf_s[i] = o[10];
        if (sampled_flags) std::memcpy(&sampled_flags[i], &o[11], 4);
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH
