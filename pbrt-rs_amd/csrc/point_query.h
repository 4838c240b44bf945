// point_query.h — the point queries (pbrt_hip_bsdf_query, pbrt_hip_bsdf_query_hair, pbrt_hip_light_sample_li): what their kernels
// share on the device (the shading frame, a point's inputs, the 12-float record) and their one host driver (stage the inputs,
// launch through a callable, bring the records home). The kernels stay in the translation units that hold the functions they
// inline. A unit that keeps the headers' plain kernels local (PB_PLAIN_KERNEL, dev_math.h) says so before it includes this.
#pragma once
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "staging.h"
#include "wavefront.h"  // Frame, V3, PB_DEV; scene.h through it

namespace pb {

// ---- device ----
// the shading frame of a query: ns = ng = +z, dpdu = +x
PB_DEV Frame query_frame() {
    Frame fr;
    fr.ss = V3{1.0f, 0.0f, 0.0f};
    fr.ts = V3{0.0f, 1.0f, 0.0f};
    fr.ns = V3{0.0f, 0.0f, 1.0f};
    fr.ng = fr.ns;
    return fr;
}
PB_DEV V3 query_v3(const float* __restrict__ in, int64_t i) { return V3{in[3 * i], in[3 * i + 1], in[3 * i + 2]}; }
// a BSDF query's record: {f.xyz, pdf, wi_s.xyz, f_s.xyz, pdf_s, sampled BxDFType bits}
PB_DEV void query_write(float* __restrict__ out, int64_t i, V3 f, float pdf, V3 wi_s, V3 f_s, float pdf_s, int sampled) {
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

// ---- host ----
struct QueryInput {
    const float* host;  // n * width floats, or null: the kernel does not read them and nothing goes up
    int width;
};
// The inputs side by side in one device block, in the order given (input k starts at n * the widths before it); launch(d_in, d_out)
// queues the kernel on the context's stream; *records receives n * record floats. Allocation failure: PBRT_HIP_ERR_OOM.
template <class Launch>
int run_point_query(PbrtHipContext* ctx, int64_t n, std::initializer_list<QueryInput> inputs, int record, const char* kernel, Launch&& launch,
                    std::vector<float>* records) {
    const size_t un = (size_t)n;
    size_t in_width = 0;
    for (const QueryInput& q : inputs) in_width += (size_t)q.width;
    Staging dev(ctx);
    float* d_in = dev.alloc<float>(un * in_width);
    float* d_out = dev.alloc<float>(un * record);
    if (dev.failed) return PBRT_HIP_ERR_OOM;
    size_t at = 0;
    for (const QueryInput& q : inputs) {
        if (q.host && !dev.upload(d_in + at * un, q.host, un * q.width * sizeof(float))) return PBRT_HIP_ERR_DEVICE;
        at += (size_t)q.width;
    }
    launch(d_in, d_out);
    records->resize(un * record);
    if (!hip_ok(ctx, hipGetLastError(), kernel) || !hip_ok(ctx, hipStreamSynchronize(ctx->stream), kernel) ||
        !dev.download(records->data(), d_out, un * record * sizeof(float)))
        return PBRT_HIP_ERR_DEVICE;
    return PBRT_HIP_OK;
}

struct BsdfQueryOut {  // each optional
    float *f, *pdf, *wi_s, *f_s, *pdf_s;
    int32_t* sampled_flags;
};
// pbrt_hip_bsdf_query (hair_row false: every row but a hair row) and pbrt_hip_bsdf_query_hair (hair_row true) behind PB_ENTER:
// validate, run, scatter the records to the outputs. `inputs` start with wo, wi, u; null_text names them all.
template <class Launch>
int bsdf_query(PbrtHipScene* s, const char* entry, bool hair_row, int32_t material, int64_t n, std::initializer_list<QueryInput> inputs,
               const char* null_text, const char* kernel, Launch&& launch, const BsdfQueryOut& out) {
    PbrtHipContext* ctx = s->ctx;
    auto invalid = [&](const char* why) {
        ctx->last_error = std::string(entry) + ": " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (material < 0 || material >= s->d.n_materials) return invalid("material index out of range");
    if ((s->h_materials[material].type == kMatHair) != hair_row)
        return invalid(hair_row ? "the row is not a hair row (pbrt_hip_bsdf_query serves every other row)"
                                : "a hair row needs h per point: pbrt_hip_bsdf_query_hair");
    if (n < 0 || n > ((int64_t)1 << 31)) return invalid("n must be in [0, 2^31]");
    if (n == 0) return PBRT_HIP_OK;
    for (const QueryInput& q : inputs)
        if (!q.host) return invalid(null_text);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<float> h;
    if (int rc = run_point_query(ctx, n, inputs, 12, kernel, launch, &h)) return rc;
    for (size_t i = 0; i < (size_t)n; ++i) {
        const float* o = &h[12 * i];
        for (int k = 0; k < 3; ++k) {
            if (out.f) out.f[3 * i + k] = o[k];
            if (out.wi_s) out.wi_s[3 * i + k] = o[4 + k];
            if (out.f_s) out.f_s[3 * i + k] = o[7 + k];
        }
        if (out.pdf) out.pdf[i] = o[3];
        if (out.pdf_s) out.pdf_s[i] = o[10];
        if (out.sampled_flags) std::memcpy(&out.sampled_flags[i], &o[11], 4);
    }
    return PBRT_HIP_OK;
}

}  // namespace pb
