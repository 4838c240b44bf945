// render.hip — Integrator::render behind the C ABI: pbrt_hip_render / pbrt_hip_render_device, pbrt_hip_li and pbrt_hip_camera_rays
// (SamplerIntegrator::render, src/core/integrator.rs:399-480) = wavefront_render, the device half of a render. What a call
// decides on the host (parameters, refusals, tiles, pass size, sort switches, sampler layout, PassParams) is host_render.cpp's
// plan_render; RenderJob here is that plan plus the device objects that carry it out, in stages (buffers, sampler tables, light
// distribution, the wavefront loop, the film); which traversal and shading kernel a launch runs comes from kernel_select.h. Also
// here: the film helpers, the block cache (DevBuf), the point-query kernels of the rows this unit's shading kernels inline
// (point_query.h holds what they share and their host driver; staging.h the scratch of every entry point that takes host
// pointers), and the per-vertex shading data of the TriangleMesh (pbrt_hip_scene_set_shading_data).
#include <hip/hip_runtime.h>
#include "abi_guard.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host_motion.h"
#include "host_render.h"
#include "scene.h"
#include "trace.h"
#include "wavefront.h"
#define PB_SELECT_SHADING_KERNELS  // kernel_select.h: the tables over the kernels of wavefront.h as well
#include "kernel_select.h"
#include "point_query.h"

using namespace pb;

// ------------------------------------------------------------------------------------
// render: see wavefront.h
// ------------------------------------------------------------------------------------
// The animated camera's DevMotion row, checked before anything is launched (host_motion.cpp). *row stays null for the static
// camera: a null motion or animated == 0.
static int camera_row(PbrtHipContext* ctx, const PbrtCamera& camera, const PbrtCameraMotion* motion, DevMotion* storage,
                      const DevMotion** row) {
    *row = nullptr;
    if (!motion || !motion->animated) return PBRT_HIP_OK;
    if (const char* why = camera_motion_row(camera, *motion, storage)) {
        ctx->last_error = std::string("camera motion: ") + why;
        return PBRT_HIP_ERR_INVALID;
    }
    *row = storage;
    return PBRT_HIP_OK;
}

extern "C" int pbrt_hip_render_device_moving_camera(PbrtHipScene* s, const PbrtCamera* camera, const PbrtCameraMotion* motion,
                                                    const PbrtRenderParams* params, float* d_film, PbrtRenderStats* stats) try {
    if (!s || !camera || !params || !d_film) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(s->ctx);
    DevMotion storage;
    const DevMotion* row;
    if (int rc = camera_row(s->ctx, *camera, motion, &storage, &row)) return rc;
    HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    return wavefront_render(s, *camera, *params, d_film, stats, nullptr, row);
}
PB_ABI_CATCH
extern "C" int pbrt_hip_render_device(PbrtHipScene* s, const PbrtCamera* camera, const PbrtRenderParams* params,
                                      float* d_film, PbrtRenderStats* stats) try {
    return pbrt_hip_render_device_moving_camera(s, camera, nullptr, params, d_film, stats);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_render(PbrtHipScene* s, const PbrtCamera* camera, const PbrtRenderParams* params,
                               float* film_xyzw, PbrtRenderStats* stats) try {
    return pbrt_hip_render_moving_camera(s, camera, nullptr, params, film_xyzw, stats);
}
PB_ABI_CATCH
extern "C" int pbrt_hip_render_moving_camera(PbrtHipScene* s, const PbrtCamera* camera, const PbrtCameraMotion* motion,
                                             const PbrtRenderParams* params, float* film_xyzw, PbrtRenderStats* stats) try {
    if (!s || !camera || !params || !film_xyzw) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    DevMotion storage;
    const DevMotion* row;
    if (int rc = camera_row(ctx, *camera, motion, &storage, &row)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (params->width <= 0 || params->height <= 0) return PBRT_HIP_ERR_INVALID;
    const size_t n_floats = (size_t)params->width * params->height * 4;
    Staging dev(ctx);  // after a deadline (ctx->lost) an abandoned kernel may still write the film: it stays
    float* d_film = dev.alloc<float>(n_floats);
    if (!d_film) return PBRT_HIP_ERR_DEVICE;
    int rc = wavefront_render(s, *camera, *params, d_film, stats, nullptr, row);
    if (rc == PBRT_HIP_OK && !dev.download(film_xyzw, d_film, n_floats * sizeof(float), false, "film D2H")) rc = PBRT_HIP_ERR_DEVICE;
    return rc;
}
PB_ABI_CATCH

// A film on the context's device for hosts that have no HIP binding of their own (a Rust or C caller): what
// pbrt_hip_render_device renders into, pbrt_hip_film_reduce merges and pbrt_hip_film_download brings home.
extern "C" int pbrt_hip_film_create(PbrtHipContext* ctx, int64_t n_pixels, float** d_film_out) try {
    if (!ctx || !d_film_out || n_pixels <= 0) return PBRT_HIP_ERR_INVALID;
    *d_film_out = nullptr;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_pixels * 4 * sizeof(float);
    float* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        ctx->last_error = "pbrt_hip_film_create: out of device memory";
        return PBRT_HIP_ERR_OOM;
    }
    HIP_TRY(ctx, e);
    if (!hip_ok(ctx, hipMemsetAsync(d, 0, bytes, ctx->stream), "hipMemsetAsync (film)") ||
        !hip_ok(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize (film)")) {
        (void)hipFree(d);
        return PBRT_HIP_ERR_DEVICE;
    }
    *d_film_out = d;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_film_download(PbrtHipContext* ctx, const float* d_film_xyzw, int64_t n_pixels, float* film_xyzw) try {
    if (!ctx || !d_film_xyzw || !film_xyzw || n_pixels < 0) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // renders and reduces of this context run on its stream
    HIP_TRY(ctx, hipMemcpy(film_xyzw, d_film_xyzw, (size_t)n_pixels * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" void pbrt_hip_film_destroy(PbrtHipContext* ctx, float* d_film_xyzw) {
    if (!ctx || !d_film_xyzw) return;
    PB_LOCK(ctx);
    if (ctx->lost) return;  // an abandoned kernel may still write it and hipFree would wait for the device: it goes with the process
    if (hipSetDevice(ctx->device) == hipSuccess) (void)hipFree(d_film_xyzw);
}

// ------------------------------------------------------------------------------------
// Integrator::li in batch form (integrator.rs:29-42) and the camera-ray stage on its own
// ------------------------------------------------------------------------------------
static int li_params_to_render(const PbrtLiParams* lp, PbrtRenderParams* rp) {
    std::memset(rp, 0, sizeof(*rp));
    rp->integrator = lp->integrator;
    rp->max_depth = lp->max_depth;
    rp->rr_threshold = lp->rr_threshold;
    rp->light_strategy = lp->light_strategy;
    rp->ao_samples = lp->ao_samples;
    rp->tile_world = 1;
    return (lp->draws_before_li < 0 || lp->draws_before_li > 4096) ? PBRT_HIP_ERR_INVALID : PBRT_HIP_OK;
}

extern "C" int pbrt_hip_li_device(PbrtHipScene* s, const PbrtLiParams* lp, const PbrtRay* d_rays, const uint64_t* d_stream_keys,
                                  int64_t n, float* d_rgb, PbrtRenderStats* stats) try {
    if (!s || !lp || n < 0 || (n > 0 && (!d_rays || !d_stream_keys || !d_rgb))) return PBRT_HIP_ERR_INVALID;
    PbrtRenderStats zero{};
    if (stats) *stats = zero;
    if (n == 0) return PBRT_HIP_OK;
    PB_ENTER(s->ctx);
    HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    PbrtRenderParams rp;
    if (li_params_to_render(lp, &rp) != PBRT_HIP_OK) {
        s->ctx->last_error = "li: draws_before_li must be in [0, 4096]";
        return PBRT_HIP_ERR_INVALID;
    }
    LiBatch b;
    b.d_rays = d_rays;
    b.d_keys = d_stream_keys;
    b.n = n;
    b.skip = lp->draws_before_li;
    b.d_rgb = d_rgb;
    PbrtCamera cam{};
    return wavefront_render(s, cam, rp, nullptr, stats, &b);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_li(PbrtHipScene* s, const PbrtLiParams* lp, const PbrtRay* rays, const uint64_t* stream_keys, int64_t n,
                           float* rgb, PbrtRenderStats* stats) try {
    if (!s || !lp || n < 0 || (n > 0 && (!rays || !stream_keys || !rgb))) return PBRT_HIP_ERR_INVALID;
    PbrtRenderStats zero{};
    if (stats) *stats = zero;
    if (n == 0) return PBRT_HIP_OK;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Staging dev(ctx);  // as pbrt_hip_render: what an abandoned kernel may still touch is never freed
    PbrtRay* d_rays = dev.alloc<PbrtRay>((size_t)n);
    uint64_t* d_keys = dev.alloc<uint64_t>((size_t)n);
    float* d_rgb = dev.alloc<float>((size_t)n * 3);
    if (dev.failed) return PBRT_HIP_ERR_OOM;
    if (!dev.upload(d_rays, rays, (size_t)n * sizeof(PbrtRay)) || !dev.upload(d_keys, stream_keys, (size_t)n * sizeof(uint64_t)))
        return PBRT_HIP_ERR_DEVICE;
    int rc = pbrt_hip_li_device(s, lp, d_rays, d_keys, n, d_rgb, stats);
    if (rc == PBRT_HIP_OK && !dev.download(rgb, d_rgb, (size_t)n * 3 * sizeof(float))) rc = PBRT_HIP_ERR_DEVICE;
    return rc;
}
PB_ABI_CATCH

// BSDF::f / pdf / sample_f of one material in the shading frame (ns = ng = +z, dpdu = +x), evaluated by the functions k_shade
// and k_shade_direct inline (wf_microfacet.h; mirror / glass: the specular sampler of k_shade). out: 12 floats per query,
// {f.xyz, pdf, wi_s.xyz, f_s.xyz, pdf_s, sampled BxDFType bits}.
__global__ void k_bsdf_query(const DevMaterial* __restrict__ materials, int material, int64_t n, const float* __restrict__ wo_in,
                             const float* __restrict__ wi_in, const float* __restrict__ u_in, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevMaterial mat = materials[material];
    const Frame fr = query_frame();
    const V3 wo = query_v3(wo_in, i), wi = query_v3(wi_in, i);
    const float u0 = u_in[2 * i], u1 = u_in[2 * i + 1];
    V3 f = V3{0.0f, 0.0f, 0.0f}, wi_s = f, f_s = f;
    float pdf = 0.0f, pdf_s = 0.0f;
    int sampled = 0;
    const GenBsdf nsb = gen_bsdf(mat);
    if (nsb.n > 0) {
        gen_f_pdf(nsb, fr, wo, wi, &f, &pdf);
        bool ok;
        float ps = 0.0f;
        V3 w;
        V3 fs = gen_sample_f(nsb, fr, wo, u0, u1, &w, &ps, &ok, &sampled);
        if (ok) {
            wi_s = w;
            f_s = fs;
            pdf_s = ps;
        } else {
            sampled = 0;
        }
    } else if (mat.type == PBRT_MAT_MIRROR || mat.type == PBRT_MAT_GLASS) {
        const V3 kd = V3{mat.kd[0], mat.kd[1], mat.kd[2]}, kt = V3{mat.kt[0], mat.kt[1], mat.kt[2]};
        const bool has_lobe = mat.type == PBRT_MAT_GLASS ? !(is_black(kd) && is_black(kt)) : !is_black(kd);
        const float ur = fminr(u0 * 1.0f - 0.0f, kOneMinusEpsilon);
        if (has_lobe && wo.z != 0.0f) {
            V3 wil = V3{0.0f, 0.0f, 0.0f};
            float ps = 0.0f;
            bool tr = false;
            V3 fs = sample_specular_local(mat, kd, kt, wo, ur, 0, &wil, &ps, &tr);
            if (ps != 0.0f) {
                wi_s = to_world(fr, wil);
                f_s = fs;
                pdf_s = ps;
                sampled = kBxdfSpecular | (tr ? kBxdfTransmission : kBxdfReflection);
            }
        }
    }
    query_write(out, i, f, pdf, wi_s, f_s, pdf_s, sampled);
}

// the same for a Disney row (wf_disney.h): `d` is the row's block
__global__ void k_bsdf_query_disney(const DevDisney* __restrict__ d, int64_t n, const float* __restrict__ wo_in, const float* __restrict__ wi_in,
                                    const float* __restrict__ u_in, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Frame fr = query_frame();
    const V3 wo = query_v3(wo_in, i), wi = query_v3(wi_in, i);
    V3 f, wi_s = V3{0.0f, 0.0f, 0.0f}, f_s = wi_s;
    float pdf, pdf_s = 0.0f;
    int sampled = 0;
    dz_f_pdf(d, fr, wo, wi, &f, &pdf);
    bool ok;
    float ps = 0.0f;
    V3 w;
    V3 fs = dz_sample_f(d, fr, wo, u_in[2 * i], u_in[2 * i + 1], &w, &ps, &ok, &sampled);
    if (ok) {
        wi_s = w;
        f_s = fs;
        pdf_s = ps;
    } else {
        sampled = 0;
    }
    query_write(out, i, f, pdf, wi_s, f_s, pdf_s, sampled);
}

// the same for a lobe row (wf_lobes.h): BSDF::f and pdf under BSDF_ALL, sample_f under BSDF_ALL, so a specular lobe can be the
// pick: sampled then carries bit 16 beside a non-zero pdf_s
__global__ void k_bsdf_query_lobes(const DevLobeRow* __restrict__ row, int64_t n, const float* __restrict__ wo_in, const float* __restrict__ wi_in,
                                   const float* __restrict__ u_in, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Frame fr = query_frame();
    const V3 wo = query_v3(wo_in, i), wi = query_v3(wi_in, i);
    V3 f, wi_s = V3{0.0f, 0.0f, 0.0f}, f_s = wi_s;
    float pdf, pdf_s = 0.0f;
    int sampled = 0;
    lobes_f_pdf(row, fr, wo, wi, kBxdfAll, &f, &pdf);
    bool ok;
    float ps = 0.0f;
    V3 w;
    V3 fs = lobes_sample_f(row, fr, wo, u_in[2 * i], u_in[2 * i + 1], kBxdfAll, &w, &ps, &ok, &sampled);
    if (ok) {
        wi_s = w;
        f_s = fs;
        pdf_s = ps;
    } else {
        sampled = 0;
    }
    query_write(out, i, f, pdf, wi_s, f_s, pdf_s, sampled);
}

extern "C" int pbrt_hip_bsdf_query(PbrtHipScene* s, int32_t material, int64_t n, const float* wo, const float* wi, const float* u, float* f,
                                   float* pdf, float* wi_s, float* f_s, float* pdf_s, int32_t* sampled_flags) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(s->ctx);
    const size_t un = (size_t)n;
    return bsdf_query(
        s, "pbrt_hip_bsdf_query", false, material, n, {{wo, 3}, {wi, 3}, {u, 2}}, "null wo / wi / u", "k_bsdf_query",
        [&](const float* d_in, float* d_out) {
            const dim3 grid((unsigned)((n + 255) / 256)), block(256);
            hipStream_t st = s->ctx->stream;
            if (s->h_materials[material].type == kMatLobes)
                hipLaunchKernelGGL(k_bsdf_query_lobes, grid, block, 0, st, s->d.lobe_rows + material, n, d_in, d_in + 3 * un, d_in + 6 * un, d_out);
            else if (s->h_materials[material].type == kMatDisney)
                hipLaunchKernelGGL(k_bsdf_query_disney, grid, block, 0, st, s->d.disney + material, n, d_in, d_in + 3 * un, d_in + 6 * un, d_out);
            else
                hipLaunchKernelGGL(k_bsdf_query, grid, block, 0, st, s->d.materials, material, n, d_in, d_in + 3 * un, d_in + 6 * un, d_out);
        },
        BsdfQueryOut{f, pdf, wi_s, f_s, pdf_s, sampled_flags});
}
PB_ABI_CATCH

// the scene's part of ShadeConsts: its tables as the shading kernels read them (the light distribution of a render, the
// light-sample prefix and a spatial table are the caller's to add)
static void scene_shade_consts(const PbrtHipScene* s, ShadeConsts* out) {
    ShadeConsts& sc = *out;
    sc.bvh = s->d.bvh;
    sc.materials = s->d.materials;
    sc.lights = s->d.lights;
    sc.n_lights = s->d.n_lights;
    sc.n_infinite = s->d.n_infinite;
    sc.infinite_ids = s->d.infinite_ids;
    sc.env_maps = s->d.env_maps;
    sc.distrib = s->d.light_distrib_uniform;
    std::memcpy(sc.env_cond_func, s->d.env_cond_func, sizeof(sc.env_cond_func));
    std::memcpy(sc.env_cond_cdf, s->d.env_cond_cdf, sizeof(sc.env_cond_cdf));
    std::memcpy(sc.env_cond_int, s->d.env_cond_int, sizeof(sc.env_cond_int));
    std::memcpy(sc.env_marg_func, s->d.env_marg_func, sizeof(sc.env_marg_func));
    std::memcpy(sc.env_marg_cdf, s->d.env_marg_cdf, sizeof(sc.env_marg_cdf));
    sc.env_marg_int = s->d.env_marg_int;
    sc.world_radius = s->d.world_radius;
    sc.light_sample_prefix = nullptr;
    sc.total_light_samples = 0;
    sc.spatial = nullptr;
    sc.n_voxel[0] = sc.n_voxel[1] = sc.n_voxel[2] = 1;
    sc.mis_bool = s->ctx->count_traversal != 1 ? 1 : 0;  // wf_state.h: RS_MIS_BOOL
    sc.disney = s->d.disney;
    sc.light_maps = s->d.light_maps;
    sc.lobe_rows = s->d.lobe_rows;
    sc.motions = s->d_motions;
    if (s->d.curves) sc.curves = s->d.curves;  // the same slot: a scene with curves has one level and no motions (wf_surface.h)
}

// Light::sample_li (light.rs:35-42) of one light of the scene from bare interactions at the world points p (normal and error
// zero, as spatial_light_tables calls it), through the light_sample_li the shading kernels inline. out: 7 floats per query,
// {wi.xyz, pdf, li.rgb}. u == null (delta lights): the sample is not read.
template <bool SHP>
__global__ void k_light_query(ShadeConsts sc, int light, int64_t n, const float* __restrict__ p_in, const float* __restrict__ u_in,
                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Surf sf;
    sf.n = V3{0.0f, 0.0f, 0.0f};
    sf.p_error = V3{0.0f, 0.0f, 0.0f};
    sf.p = V3{p_in[3 * i], p_in[3 * i + 1], p_in[3 * i + 2]};
    const float u0 = u_in ? u_in[2 * i] : 0.0f, u1 = u_in ? u_in[2 * i + 1] : 0.0f;
    const DevLight lt = sc.lights[light];
    V3 wi, li, p1, p1_err, p1_n;
    float pdf;
    light_sample_li<SHP, true>(sc, sf, lt, u0, u1, &wi, &pdf, &li, &p1, &p1_err, &p1_n);
    float* o = out + 7 * i;
    o[0] = wi.x;
    o[1] = wi.y;
    o[2] = wi.z;
    o[3] = pdf;
    o[4] = li.x;
    o[5] = li.y;
    o[6] = li.z;
}

extern "C" int pbrt_hip_light_sample_li(PbrtHipScene* s, int32_t light, int64_t n, const float* p, const float* u, float* wi, float* pdf,
                                        float* li) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const char* why) {
        ctx->last_error = std::string("pbrt_hip_light_sample_li: ") + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (light < 0 || light >= s->d.n_lights) return invalid("light index out of range");
    if (n < 0 || n > ((int64_t)1 << 31)) return invalid("n must be in [0, 2^31]");
    if (n == 0) return PBRT_HIP_OK;
    if (!p) return invalid("null p");
    if (!u && !s->h_lights[light].delta) return invalid("null u for a light that is not a delta light");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t un = (size_t)n;
    std::vector<float> h;
    const int rc = run_point_query(
        ctx, n, {{p, 3}, {u, 2}}, 7, "k_light_query",
        [&](const float* d_in, float* d_out) {
            ShadeConsts sc;
            scene_shade_consts(s, &sc);
            const dim3 grid((unsigned)((n + 255) / 256)), block(256);
            const float* d_u = u ? d_in + 3 * un : nullptr;
            if (s->d.bvh.has_spheres == 2)
                hipLaunchKernelGGL(k_light_query<true>, grid, block, 0, ctx->stream, sc, light, n, d_in, d_u, d_out);
            else
                hipLaunchKernelGGL(k_light_query<false>, grid, block, 0, ctx->stream, sc, light, n, d_in, d_u, d_out);
        },
        &h);
    if (rc != PBRT_HIP_OK) return rc;
    for (size_t i = 0; i < un; ++i) {
        const float* o = &h[7 * i];
        for (int k = 0; k < 3; ++k) {
            if (wi) wi[3 * i + k] = o[k];
            if (li) li[3 * i + k] = o[4 + k];
        }
        if (pdf) pdf[i] = o[3];
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_camera_rays(PbrtHipScene* s, const PbrtCamera* camera, const PbrtRenderParams* params, int64_t capacity,
                                    PbrtRay* rays, uint64_t* stream_keys, float* p_film, int32_t* pixel_sample, int64_t* n_out) try {
    return pbrt_hip_camera_rays_moving_camera(s, camera, nullptr, params, capacity, rays, stream_keys, p_film, pixel_sample, n_out);
}
PB_ABI_CATCH
extern "C" int pbrt_hip_camera_rays_moving_camera(PbrtHipScene* s, const PbrtCamera* camera, const PbrtCameraMotion* motion,
                                                  const PbrtRenderParams* params, int64_t capacity, PbrtRay* rays,
                                                  uint64_t* stream_keys, float* p_film, int32_t* pixel_sample, int64_t* n_out) try {
    if (!s || !camera || !params || !n_out) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    DevMotion storage;
    const DevMotion* row;
    if (int rc = camera_row(ctx, *camera, motion, &storage, &row)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (params->width <= 0 || params->height <= 0 || params->spp <= 0 || params->x0 > params->x1 || params->y0 > params->y1)
        return PBRT_HIP_ERR_INVALID;
    int64_t n = 0;  // as wavefront_render will fix it
    if (const char* why = export_ray_count(*params, &n)) {
        ctx->last_error = why;
        return PBRT_HIP_ERR_INVALID;
    }
    *n_out = n;
    if (n == 0) return PBRT_HIP_OK;
    if (capacity < n || !rays || !stream_keys || !p_film || !pixel_sample) {
        ctx->last_error = "camera rays: output capacity too small (n_out holds the need)";
        return PBRT_HIP_ERR_INVALID;
    }
    Staging dev(ctx);
    LiBatch b;
    b.out_rays = dev.alloc<PbrtRay>((size_t)n);
    b.out_keys = dev.alloc<uint64_t>((size_t)n);
    b.out_pfilm = dev.alloc<float>((size_t)n * 2);
    b.out_pixel_sample = dev.alloc<int32_t>((size_t)n * 3);
    if (dev.failed) return PBRT_HIP_ERR_OOM;
    int rc = wavefront_render(s, *camera, *params, nullptr, nullptr, &b, row);
    if (rc == PBRT_HIP_OK && (!dev.download(rays, b.out_rays, (size_t)n * sizeof(PbrtRay)) ||
                              !dev.download(stream_keys, b.out_keys, (size_t)n * sizeof(uint64_t)) ||
                              !dev.download(p_film, b.out_pfilm, (size_t)n * 2 * sizeof(float)) ||
                              !dev.download(pixel_sample, b.out_pixel_sample, (size_t)n * 3 * sizeof(int32_t))))
        rc = PBRT_HIP_ERR_DEVICE;
    return rc;
}
PB_ABI_CATCH

// ------------------------------------------------------------------------------------
// wavefront_render — host driver of the kernels in wavefront.h
// ------------------------------------------------------------------------------------
namespace {
// Device buffers of one call. Blocks come from (and return to) the context's cache, so that repeated renders of the
// same size do not pay hipMalloc / hipFree again.
struct DevBuf {
    std::vector<size_t> taken;  // indices into ctx->block_cache
    PbrtHipContext* ctx;
    explicit DevBuf(PbrtHipContext* c) : ctx(c) {}
    ~DevBuf() {
        if (ctx->lost) return;  // a kernel of the abandoned call may still be writing these blocks: they stay taken for good
        for (size_t i : taken) ctx->block_cache[i].in_use = false;
        size_t idle = 0;
        for (const auto& b : ctx->block_cache)
            if (!b.in_use) idle += b.bytes;
        if (idle > ((size_t)160 << 30)) trim(ctx);  // renders of many different sizes: do not sit on most of the HBM
    }
    static void trim(PbrtHipContext* ctx) {  // release every block no call is using (slots stay, indices are stable)
        for (auto& b : ctx->block_cache)
            if (!b.in_use && b.ptr) {
                (void)hipFree(b.ptr);
                b.ptr = nullptr;
                b.bytes = 0;
            }
    }
    template <class T>
    T* alloc(size_t n, bool* ok) {
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        // best fit among the free cached blocks that are not wastefully large
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < ctx->block_cache.size(); ++i) {
            const auto& b = ctx->block_cache[i];
            if (!b.in_use && b.ptr && b.bytes >= bytes && b.bytes <= bytes + bytes / 4 + 4096 &&
                (best == SIZE_MAX || b.bytes < ctx->block_cache[best].bytes))
                best = i;
        }
        if (best != SIZE_MAX) {
            ctx->block_cache[best].in_use = true;
            taken.push_back(best);
            return (T*)ctx->block_cache[best].ptr;
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {  // out of memory with idle cached blocks around: drop them and retry once
            (void)hipGetLastError();
            trim(ctx);
            e = hipMalloc(&p, bytes);
        }
        if (!hip_ok(ctx, e, "hipMalloc (path state)")) {
            *ok = false;
            return nullptr;
        }
        size_t slot = ctx->block_cache.size();
        for (size_t i = 0; i < ctx->block_cache.size(); ++i)
            if (!ctx->block_cache[i].ptr && !ctx->block_cache[i].in_use) {
                slot = i;
                break;
            }
        if (slot == ctx->block_cache.size()) ctx->block_cache.push_back({nullptr, 0, false});
        ctx->block_cache[slot] = {p, bytes, true};
        taken.push_back(slot);
        return (T*)p;
    }
};
}  // namespace

// ---- optional per-vertex normals / uvs of the TriangleMesh (triangle.rs:17-26, used at :60-72, 252-312, 337-341) ----
__global__ void k_set_shading(const int* __restrict__ slot_prim, const int* __restrict__ idx, const float* __restrict__ pos,
                              const float* __restrict__ normals, const float* __restrict__ tangents,
                              const float* __restrict__ uvs, int n, float4* __restrict__ out, float4* __restrict__ tris) {
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    int prim = slot_prim[slot];
    int v[3] = {idx[3 * (size_t)prim], idx[3 * (size_t)prim + 1], idx[3 * (size_t)prim + 2]};
    float nn[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, uv[6] = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f};
    for (int k = 0; k < 3; ++k) {
        if (normals)
            for (int c = 0; c < 3; ++c) nn[3 * k + c] = normals[3 * (size_t)v[k] + c];
        if (tangents)
            for (int c = 0; c < 3; ++c) tt[3 * k + c] = tangents[3 * (size_t)v[k] + c];
        if (uvs)
            for (int c = 0; c < 2; ++c) uv[2 * k + c] = uvs[2 * (size_t)v[k] + c];
    }
    float4* o = out + 6 * (size_t)slot;
    o[0] = make_float4(nn[0], nn[1], nn[2], nn[3]);
    o[1] = make_float4(nn[4], nn[5], nn[6], nn[7]);
    o[2] = make_float4(nn[8], tt[0], tt[1], tt[2]);
    o[3] = make_float4(tt[3], tt[4], tt[5], tt[6]);
    o[4] = make_float4(tt[7], tt[8], uv[0], uv[1]);
    o[5] = make_float4(uv[2], uv[3], uv[4], uv[5]);
    // "Triangle::intersect returns false" depends on the uvs (triangle.rs:197-216): refresh the flag
    float a[3], b[3], c[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = pos[3 * (size_t)v[0] + k];
        b[k] = pos[3 * (size_t)v[1] + k];
        c[k] = pos[3 * (size_t)v[2] + k];
    }
    float4 t2 = tris[3 * (size_t)slot + 2];
    int w = __float_as_int(t2.w) & ~kTriDegenerate;
    if (triangle_rejected_by_intersect(a, b, c, uv)) w |= kTriDegenerate;
    t2.w = __int_as_float(w);
    tris[3 * (size_t)slot + 2] = t2;
}

// the wide-order triangle copies (wide_bvh.h) carry the kTriDegenerate flag too
__global__ void k_wide_refresh_flags(float4* __restrict__ wtris, int wide_stride, const float4* __restrict__ tris, int n) {
    int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    float4 c = wtris[(size_t)wide_stride * (size_t)pos + 2];
    c.z = tris[3 * (size_t)__float_as_int(c.y) + 2].w;
    wtris[(size_t)wide_stride * (size_t)pos + 2] = c;
}

extern "C" int pbrt_hip_scene_set_shading_data(PbrtHipScene* s, const float* positions, int32_t n_verts,
                                               const int32_t* indices, int32_t n_tris, const float* normals,
                                               const float* tangents, const float* uvs) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto fail = [&](const char* msg) {
        ctx->last_error = msg;
        return PBRT_HIP_ERR_INVALID;
    };
    if (!positions || !indices || n_tris != s->n_tris || n_verts <= 0) return fail("mesh does not match the scene");
    if (!normals && !tangents && !uvs) return fail("no normals, tangents or uvs given");
    if (s->d.bvh.tri_shading) return fail("shading data already set");
    if (s->d.bvh.has_spheres) return fail("per-vertex shading data is not supported for scenes with spheres");
    if (!mesh_indices_in_range(indices, n_tris, n_verts)) return fail("vertex index out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf tmp(ctx);
    bool ok = true;
    int* d_idx = tmp.alloc<int>(3 * (size_t)n_tris, &ok);
    float* d_pos = tmp.alloc<float>(3 * (size_t)n_verts, &ok);
    float* d_n = normals ? tmp.alloc<float>(3 * (size_t)n_verts, &ok) : nullptr;
    float* d_t = tangents ? tmp.alloc<float>(3 * (size_t)n_verts, &ok) : nullptr;
    float* d_uv = uvs ? tmp.alloc<float>(2 * (size_t)n_verts, &ok) : nullptr;
    void* out = nullptr;
    if (!ok || !hip_ok(ctx, hipMalloc(&out, (size_t)n_tris * 96), "hipMalloc shading data")) return PBRT_HIP_ERR_OOM;
    s->allocs.push_back(out);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, indices, 3 * (size_t)n_tris * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_pos, positions, 3 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, st));
    if (d_n) HIP_TRY(ctx, hipMemcpyAsync(d_n, normals, 3 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, st));
    if (d_t) HIP_TRY(ctx, hipMemcpyAsync(d_t, tangents, 3 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, st));
    if (d_uv) HIP_TRY(ctx, hipMemcpyAsync(d_uv, uvs, 2 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_set_shading, dim3((n_tris + 255) / 256), dim3(256), 0, st, s->d.slot_prim, d_idx, d_pos, d_n, d_t, d_uv,
                       n_tris, (float4*)out, const_cast<float4*>(s->d.bvh.tris));
    if (s->has_wide)
        hipLaunchKernelGGL(k_wide_refresh_flags, dim3((n_tris + 255) / 256), dim3(256), 0, st, const_cast<float4*>(s->wide.tris),
                           s->wide.vec_stride, s->d.bvh.tris, n_tris);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    s->d.bvh.tri_shading = (const float4*)out;
    s->d.bvh.has_normals = normals ? 1 : 0;
    s->d.bvh.has_tangents = tangents ? 1 : 0;
    s->d.bvh.has_uvs = uvs ? 1 : 0;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

namespace pb {
int sort_pairs_u32(hipStream_t st, void* temp, size_t* temp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                   const uint32_t* vals_in, uint32_t* vals_out, size_t n, int bits);
int exclusive_scan_u64(hipStream_t st, void* temp, size_t* temp_bytes, const unsigned long long* in, unsigned long long* out, size_t n);
}

// ---- wavefront_render in stages: one plain struct holds the render, its member functions are the stages in order ----
namespace {
// the four events of a render; they go with this object on every way out
struct RenderEvents {
    hipEvent_t begin = nullptr, end = nullptr, t0 = nullptr, t1 = nullptr;
    bool create(PbrtHipContext* ctx) {
        return hip_ok(ctx, hipEventCreate(&begin), "hipEventCreate") && hip_ok(ctx, hipEventCreate(&end), "hipEventCreate") &&
               hip_ok(ctx, hipEventCreate(&t0), "hipEventCreate") && hip_ok(ctx, hipEventCreate(&t1), "hipEventCreate");
    }
    ~RenderEvents() {
        for (hipEvent_t e : {begin, end, t0, t1})
            if (e) (void)hipEventDestroy(e);
    }
};

// a rocPRIM pair sort's buffers (keys in / out, the sorted values, scratch)
struct SortBufs {
    uint32_t *keys[2] = {nullptr, nullptr}, *vals = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
};

// the ray-queue expansion's scratch (wf_ray_expand.h): per-block token counts, their exclusive scan, rocPRIM scratch
struct ExpandBufs {
    unsigned long long *counts = nullptr, *offsets = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
};

#ifndef PB_SORT_FROM
#define PB_SORT_FROM 2  // 1 (the first bounce sorted as well) measured in profiles/r13_path_sort.txt
#endif
constexpr int kSortFrom = PB_SORT_FROM;  // first sorted wavefront: the first bounce still follows the pixel order of its camera rays
static_assert(kSortFrom >= 1, "wavefront 0 is the identity queue k_generate leaves: it has no sort entries");

static_assert(kPlanTile == kTile && kPlanPathRecBits == kPathRecBits, "host_render.h plans the tiles and the sort entries of these kernels");

// One render: the plan (host_render.h: everything decided about the call, on the host), what the device half holds between its
// stages, and the stages in the order run() goes through them. The device blocks belong to the DevBuf of run()'s own frame.
struct RenderJob : RenderPlan {
    PbrtHipScene* s;
    PbrtHipContext* ctx;
    hipStream_t st;
    const LiBatch* li;
    float* d_film;
    const DevMotion* camera_motion;  // the animated camera's row, or null (kernel_select.h: generate_key)
    TraceChoice trace;               // kernel_select.h
    hipError_t mem_query;            // what hipMemGetInfo answered where the plan needed the free bytes
    PathState ps;
    Queues q[2];
    SortBufs ray_sort;    // Morton order of the bounce rays: one (cell, packed rays) pair per path
    ExpandBufs ray_expand;
    SortBufs shade_sort;  // shade_order 2: keys, the sorted queue positions (vals)
    uint32_t* shade_positions = nullptr;
    uint32_t* special_list = nullptr;  // rays the wide kernel leaves to the binary one (wide_bvh.h)
    DirectState ds{};
    float* d_filter = nullptr;
    float4* accum = nullptr;
    TileList tiles{};
    DevCamera cam;
    ShadeConsts sc;
    DirectKernel shade_direct = nullptr;            // the shading kernels of this scene and integrator, looked up once
    PathKernel shade_path[2] = {nullptr, nullptr};  // [BIN]
    PbrtRenderStats local{};

    int invalid(const char* m) const {
        ctx->last_error = m;
        return PBRT_HIP_ERR_INVALID;
    }
    int query_sort_sizes(RenderStep upto);
    void alloc_path_buffers(DevBuf& buf, bool* ok);
    int setup_sampler(DevBuf& buf, bool* ok);
    int setup_light_distribution(const SceneNeeds& needs);
    PassParams pass_params(int s0) const;
    void wait_for_counts(int& rc);
    void trace_wavefront(const RenderEvents& ev, const Queues& qcur, uint32_t n_trace, uint32_t n_shade, int wavefront, int group_shift, int& rc);
    void shade_wavefront(const PassParams& pp, int cur, int nxt, uint32_t n_shade, int wavefront, int& rc);
    void run_wavefronts(const RenderEvents& ev, const PassParams& pp, uint32_t n_paths, int& rc);
    void film_stage(const PassParams& pp, uint32_t n_paths, bool last_pass, int& rc);
    int run(const PbrtCamera& camera, PbrtRenderStats* stats);
};

// The rocPRIM scratch sizes of the sorts the plan switched on. They are asked where they always were among the plan's refusals:
// the ray sort's behind ray_order, the shade sort's behind shade_order.
int RenderJob::query_sort_sizes(RenderStep upto) {
    if (upto == RenderStep::RayOrder && sort_rays) {
        if (pb::sort_pairs_u32(st, nullptr, &ray_sort.tmp_bytes, nullptr, nullptr, nullptr, nullptr, N, kSortKeyBits) != 0)
            return invalid("rocPRIM radix sort: size query failed");
        const size_t n_scan = (size_t)pb::ray_expand_blocks((uint32_t)N) + 1;  // the last element: the sections' totals
        if (pb::exclusive_scan_u64(st, nullptr, &ray_expand.tmp_bytes, nullptr, nullptr, n_scan) != 0)
            return invalid("rocPRIM scan: size query failed");
    }
    if (upto == RenderStep::ShadeOrder && sort_shade &&
        pb::sort_pairs_u32(st, nullptr, &shade_sort.tmp_bytes, nullptr, nullptr, nullptr, nullptr, N, 3) != 0)
        return invalid("rocPRIM radix sort: size query failed");
    return PBRT_HIP_OK;
}

// stage 3: path state, queues, sort buffers in the sizes the plan states (allocation failures land in *ok)
void RenderJob::alloc_path_buffers(DevBuf& buf, bool* ok) {
    ps.n_paths = N;
    ps.two_level = s->d.bvh.instanced ? 1 : 0;
    ps.ray = buf.alloc<float4>(N * 6, ok);
    ps.hit = buf.alloc<float4>(N * 6, ok);
    ps.rng = buf.alloc<uint64_t>(N, ok);
    ps.L = buf.alloc<float4>(N, ok);
    ps.beta = buf.alloc<float4>(N, ok);
    ps.nee_a = buf.alloc<float4>(N, ok);
    ps.nee_f = buf.alloc<float4>(N, ok);
    ps.nee_b = buf.alloc<float4>(N, ok);
    ps.nee_light = buf.alloc<int>(N, ok);
    ps.pfilm = buf.alloc<float2>(N, ok);
    // the path integrator keeps two generations of the rays and the pending estimates (wf_state.h); the others one
    ps.ray_next = direct ? ps.ray : buf.alloc<float4>(N * 6, ok);
    ps.nee_a_next = direct ? ps.nee_a : buf.alloc<float4>(N, ok);
    ps.nee_f_next = direct ? ps.nee_f : buf.alloc<float4>(N, ok);
    ps.nee_b_next = direct ? ps.nee_b : buf.alloc<float4>(N, ok);
    ps.nee_light_next = direct ? ps.nee_light : buf.alloc<int>(N, ok);
    for (int k = 0; k < 2; ++k) {
        Queues& qk = q[k];
        qk.trace = buf.alloc<uint32_t>(N * 3, ok);
        qk.shade = buf.alloc<uint32_t>(N, ok);
        qk.counts64 = buf.alloc<unsigned long long>(2, ok);
        qk.keys = nullptr;
        for (int a = 0; a < 3; ++a) {
            const float lo = s->d.bvh.root_min[a], hi = s->d.bvh.root_max[a];
            qk.key_lo[a] = lo;
            qk.key_inv[a] = hi > lo ? 1.0f / (hi - lo) : 0.0f;
        }
    }
    if (sort_rays) {  // ray-queue sort: keys in / out, sorted entries, rocPRIM scratch; the expansion's counts and offsets
        SortBufs& rs = ray_sort;
        rs.keys[0] = buf.alloc<uint32_t>(N, ok);
        rs.keys[1] = buf.alloc<uint32_t>(N, ok);
        rs.vals = buf.alloc<uint32_t>(N, ok);
        rs.tmp = buf.alloc<char>(rs.tmp_bytes, ok);
        ExpandBufs& ex = ray_expand;
        const size_t n_scan = (size_t)pb::ray_expand_blocks((uint32_t)N) + 1;
        ex.counts = buf.alloc<unsigned long long>(n_scan, ok);
        ex.offsets = buf.alloc<unsigned long long>(n_scan, ok);
        ex.tmp = buf.alloc<char>(ex.tmp_bytes, ok);
    }
    // rays the wide kernel leaves to the binary one (wide_bvh.h): room for every entry of a trace queue
    special_list = trace.kind == TraceKind::Wide ? buf.alloc<uint32_t>(N * 3, ok) : nullptr;
    if (sort_shade) {
        SortBufs& ss = shade_sort;
        ss.keys[0] = buf.alloc<uint32_t>(N, ok);
        ss.keys[1] = buf.alloc<uint32_t>(N, ok);
        shade_positions = buf.alloc<uint32_t>(N, ok);
        ss.vals = buf.alloc<uint32_t>(N, ok);
        ss.tmp = buf.alloc<char>(ss.tmp_bytes, ok);
    }
}

// stage 4: the device side of the plan's SamplerParams: the per-path counters, the Halton tables (uploaded on first use), the
// PixelSampler tables and the list of requested arrays
int RenderJob::setup_sampler(DevBuf& buf, bool* ok) {
    ps.samp = buf.alloc<int>(N, ok);
    if (rp.sampler == PBRT_SAMPLER_HALTON) {
        if (!ctx->d_halton_primes) {
            std::vector<uint32_t> primes;
            std::vector<uint16_t> perms;
            halton_host_tables(&primes, &perms);
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_halton_primes, primes.size() * sizeof(uint32_t)));
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_halton_perms, perms.size() * sizeof(uint16_t)));
            HIP_TRY(ctx, hipMemcpy(ctx->d_halton_primes, primes.data(), primes.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIP_TRY(ctx, hipMemcpy(ctx->d_halton_perms, perms.data(), perms.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        }
        smp.primes = ctx->d_halton_primes;
        smp.perms = ctx->d_halton_perms;
    }
    if (tabulated) {
        smp.tables = buf.alloc<float>((size_t)smp.n_elems * n_pix, ok);
        int2* d_arrays = buf.alloc<int2>(arrays.size(), ok);
        smp.arrays = d_arrays;
        if (*ok && !arrays.empty())
            HIP_TRY(ctx, hipMemcpyAsync(d_arrays, arrays.data(), arrays.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        if (*ok) HIP_TRY(ctx, hipStreamSynchronize(st));  // as ever: the list is up before anything else of the render is queued
    }
    return PBRT_HIP_OK;
}

// stage 5: the light distribution of the render in sc (create_light_sample_distribution, lightdistrib.rs:222-232), with the
// scene's spatial table built on first use
int RenderJob::setup_light_distribution(const SceneNeeds& needs) {
    // "uniform", or one light -> uniform
    sc.distrib = (rp.light_strategy == 0 || s->d.n_lights == 1) ? s->d.light_distrib_uniform : s->d.light_distrib_power;
    if (spatial) {
        if (!s->d_spatial) {
            for (int i = 0; i < 3; ++i) s->spatial_voxels[i] = spatial_voxels[i];
            size_t n_voxels = (size_t)s->spatial_voxels[0] * s->spatial_voxels[1] * s->spatial_voxels[2];
            size_t floats = n_voxels * (size_t)(2 * s->d.n_lights + 2);
            void* p = nullptr;
            HIP_TRY(ctx, hipMalloc(&p, floats * sizeof(float)));
            s->allocs.push_back(p);
            for (int i = 0; i < 3; ++i) sc.n_voxel[i] = s->spatial_voxels[i];
            hipLaunchKernelGGL(spatial_tables_kernel(needs), dim3((unsigned)((n_voxels + 63) / 64)), dim3(64), 0, st, sc, (float*)p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(st));
            s->d_spatial = (float*)p;
        }
        sc.spatial = s->d_spatial;
        for (int i = 0; i < 3; ++i) sc.n_voxel[i] = s->spatial_voxels[i];
    }
    return PBRT_HIP_OK;
}

// stage 6: the plan's PassParams of the pass that starts at sample s0, with this call's device pointers
PassParams RenderJob::pass_params(int s0) const {
    PassParams pp = RenderPlan::pass_params(s0);
    pp.filter_table = d_filter;
    pp.stream_keys = li_mode ? li->d_keys : nullptr;
    return pp;
}
#define RENDER_TRY(call) \
    if (rc == PBRT_HIP_OK && !hip_ok(ctx, (call), #call)) rc = PBRT_HIP_ERR_DEVICE;

// stage 7: waits for the counts copy of a wavefront (ctx->ev_sync, recorded behind it)
void RenderJob::wait_for_counts(int& rc) {
    // spin on the event (a blocking sync costs a scheduler wake-up per wavefront), but not for ever: a kernel
    // that never finishes must surface as an error of this call, with the context's lock released
    hipError_t qe;
    const auto spin_start = std::chrono::steady_clock::now();
    uint32_t polls = 0;
    while ((qe = hipEventQuery(ctx->ev_sync)) == hipErrorNotReady) {
        if ((++polls & 0xfffu) == 0) {
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - spin_start).count();
            if (waited > ctx->wavefront_deadline_s) {
                ctx->last_error = "a wavefront did not finish within the deadline (hung kernel?)";
                ctx->lost = true;  // the stream is not drained afterwards: nothing may follow on this context
                rc = PBRT_HIP_ERR_DEVICE;
                break;
            }
            if (waited > 0.05) std::this_thread::yield();  // long wavefronts: stop burning a core
        }
    }
    if (rc == PBRT_HIP_OK) RENDER_TRY(qe);
}

// one wavefront's rays: the queue (sorted from the second bounce on when there are enough), then the traversal kernel
void RenderJob::trace_wavefront(const RenderEvents& ev, const Queues& qcur, uint32_t n_trace, uint32_t n_shade, int wavefront, int group_shift, int& rc) {
    RENDER_TRY(hipMemsetAsync(ctx->d_work_counter, 0, kWorkCounters * sizeof(unsigned int), st));
    const uint32_t* trace_queue = qcur.trace;
    if (sort_rays && wavefront >= kSortFrom) {
        // from the second bounce on the rays of a wavefront start all over the scene (the first bounce still
        // follows the pixel order of its camera rays): trace them in Morton order of their origins. k_shade left one
        // (cell, packed rays) pair per path of the shade queue (Queues::keys) and no trace-queue entries: sort the n_shade
        // pairs when there are enough rays, then expand the list into qcur.trace (wf_ray_expand.h); the pairs' values are
        // moved out of qcur.trace first, by the sort or by a copy.
        const SortBufs& rs = ray_sort;
        const ExpandBufs& ex = ray_expand;
        if (n_trace >= (1u << 20)) {
            size_t tb = rs.tmp_bytes;
            if (pb::sort_pairs_u32(st, rs.tmp, &tb, rs.keys[0], rs.keys[1], qcur.trace, rs.vals, n_shade, kSortKeyBits) != 0 && rc == PBRT_HIP_OK) {
                ctx->last_error = "rocPRIM radix sort failed";
                rc = PBRT_HIP_ERR_DEVICE;
            }
        } else {
            RENDER_TRY(hipMemcpyAsync(rs.vals, qcur.trace, (size_t)n_shade * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        }
        const uint32_t blocks = pb::ray_expand_blocks(n_shade);
        hipLaunchKernelGGL(k_ray_expand_count, dim3(blocks), dim3(kExpandBlock), 0, st, rs.vals, n_shade, ex.counts);
        size_t tb = ex.tmp_bytes;
        if (pb::exclusive_scan_u64(st, ex.tmp, &tb, ex.counts, ex.offsets, (size_t)blocks + 1) != 0 && rc == PBRT_HIP_OK) {
            ctx->last_error = "rocPRIM scan failed";
            rc = PBRT_HIP_ERR_DEVICE;
        }
        hipLaunchKernelGGL(k_ray_expand_scatter, dim3(blocks), dim3(kExpandBlock), 0, st, rs.vals, n_shade, ex.offsets, qcur.trace, n_trace);
    }
    RENDER_TRY(hipEventRecord(ev.t0, st));
    const int segments = (wavefront == 0 && !trace.inst) ? kQueueSegments : 1;  // see trace.h
    if (wavefront == 0) ctx->camera_kernel = PBRT_CAMERA_KERNEL_PER_LANE;
    dispatch(trace, [&](auto kind, auto count, auto inst) {
        constexpr TraceKind K = decltype(kind)::value;
        constexpr bool COUNT = decltype(count)::value;
        constexpr int INST = decltype(inst)::value;
        const dim3 grid(persistent_grid(s)), block(kTraceBlock);
        if constexpr (K == TraceKind::Stackless) {
            hipLaunchKernelGGL(k_trace_stackless, dim3(stackless_grid(s)), block, 0, st, s->d.bvh, ps, trace_queue, n_trace, ctx->d_work_counter,
                               segments);
        } else if constexpr (K == TraceKind::Wide) {  // the wide kernel, then the follow-up over the rays it left out
            WideTrees wt = s->wide;
            wt.special_list = special_list;
            wt.special_count = ctx->d_work_counter + kSpecialCount;
            // the camera rays of a one-level scene, a wave = one pixel's samples: walked once per wave (trace_wide_packet.h)
            const bool packets = use_camera_packets(s, trace, wavefront, group_shift);
            if (wavefront == 0) ctx->camera_kernel = packets ? PBRT_CAMERA_KERNEL_PACKET : PBRT_CAMERA_KERNEL_PER_LANE;
            if (packets)
                hipLaunchKernelGGL(k_trace_wide_packet<WavefrontRayIO<false>>, dim3(packet_grid(s)), block, 0, st, wt,
                                   WavefrontRayIO<false>{ps, trace_queue, n_trace, segments}, ctx->d_work_counter);
            else
                hipLaunchKernelGGL((k_trace_wide<COUNT, INST>), dim3(wide_grid<COUNT, INST>(s)), block, 0, st, wt, ps, trace_queue, n_trace,
                                   ctx->d_work_counter, segments, ctx->d_counters);
            hipLaunchKernelGGL(k_trace_special<INST>, grid, block, 0, st, s->d.bvh, ps, trace_queue, n_trace, special_list,
                               ctx->d_work_counter + kSpecialCount, ctx->d_work_counter + kFollowUpCounter);
        } else if constexpr (K == TraceKind::Shapes) {
            hipLaunchKernelGGL(k_trace_shapes<COUNT>, grid, block, 0, st, s->d.bvh, ps, trace_queue, n_trace, ctx->d_work_counter, ctx->d_counters,
                               segments);
        } else if constexpr (K == TraceKind::Moving) {
            hipLaunchKernelGGL((k_trace_moving<COUNT, INST>), dim3(persistent_grid(s, PB_MOVING_TRACE_WAVES)), block, 0, st, s->d.bvh, s->d_motions, ps,
                               trace_queue, n_trace, ctx->d_work_counter, ctx->d_counters, segments);
        } else if constexpr (K == TraceKind::Curves) {
            launch_trace_curves(COUNT, dim3(persistent_grid(s, PB_CURVE_TRACE_WAVES)), st, s->d.bvh, s->d.curves, ps, trace_queue, n_trace,
                                ctx->d_work_counter, ctx->d_counters, segments);
        } else {
            hipLaunchKernelGGL((k_trace<COUNT, INST, K == TraceKind::Spheres>), grid, block, 0, st, s->d.bvh, ps, trace_queue, n_trace,
                               ctx->d_work_counter, ctx->d_counters, segments);
        }
    });
    RENDER_TRY(hipGetLastError());
    RENDER_TRY(hipEventRecord(ev.t1, st));
}

// one wavefront's shading: k_shade_direct, or (sorted by material first, shade_order 2) the path kernel and the generation swap
void RenderJob::shade_wavefront(const PassParams& pp, int cur, int nxt, uint32_t n_shade, int wavefront, int& rc) {
    const dim3 grid((n_shade + 255) / 256), block(256);
    if (direct) {
        hipLaunchKernelGGL(shade_direct, grid, block, 0, st, sc, ps, ds, q[cur], q[nxt], pp, tiles, n_shade);
        return;
    }
    const Queues qin = q[cur];
    const uint32_t* order = nullptr;  // shade_order 2: the queue positions in material order
    if (sort_shade && wavefront >= 1 && n_shade >= (1u << 10)) {  // the first wavefront is all camera hits in pixel order
        const SortBufs& ss = shade_sort;
        hipLaunchKernelGGL(k_shade_sort_keys, dim3((n_shade + 255) / 256), dim3(256), 0, st, sc, ps, q[cur].shade, n_shade, pp.max_depth,
                           ss.keys[0], shade_positions);
        size_t tb = ss.tmp_bytes;
        if (pb::sort_pairs_u32(st, ss.tmp, &tb, ss.keys[0], ss.keys[1], shade_positions, ss.vals, n_shade, (s->bxdfs || s->disney || s->lobes || s->hair) ? 4 : 3) != 0 &&
            rc == PBRT_HIP_OK) {
            ctx->last_error = "rocPRIM radix sort failed";
            rc = PBRT_HIP_ERR_DEVICE;
        }
        order = ss.vals;
    }
    hipLaunchKernelGGL(shade_path[bin_shade && wavefront >= 1], grid, block, 0, st, sc, ps, qin, q[nxt], pp, tiles, n_shade, order);
    // what this launch wrote is the generation the next trace and shade launches read
    std::swap(ps.ray, ps.ray_next);
    std::swap(ps.nee_a, ps.nee_a_next);
    std::swap(ps.nee_f, ps.nee_f_next);
    std::swap(ps.nee_b, ps.nee_b_next);
    std::swap(ps.nee_light, ps.nee_light_next);
}

// stage 8a: the wavefront loop of one pass, from the generated camera rays until no path is left
void RenderJob::run_wavefronts(const RenderEvents& ev, const PassParams& pp, uint32_t n_paths, int& rc) {
    // the first wavefront is the identity: every path traces its camera ray and is shaded
    unsigned long long counts[2] = {n_paths, n_paths};
    local.camera_samples += (uint64_t)valid_pixels * pp.n_samples;
    local.rays_closest += (uint64_t)valid_pixels * pp.n_samples;
    int cur = 0, wavefront = 0;  // wavefront 0 = camera rays, 1 = first bounce + its shadow rays, ...
    while (rc == PBRT_HIP_OK && counts[1] > 0) {
        uint32_t n_trace = (uint32_t)counts[0], n_shade = (uint32_t)counts[1];
        if (n_trace > 0) trace_wavefront(ev, q[cur], n_trace, n_shade, wavefront, pp.group_shift, rc);
        int nxt = cur ^ 1;
        RENDER_TRY(hipMemsetAsync(q[nxt].counts64, 0, 2 * sizeof(unsigned long long), st));
        // the wavefront this launch of k_shade fills is traced in Morton order: have it write one sort pair per path instead
        // of the trace-queue entries (trace_wavefront expands them)
        q[nxt].keys = (sort_rays && wavefront + 1 >= kSortFrom) ? ray_sort.keys[0] : nullptr;
        shade_wavefront(pp, cur, nxt, n_shade, wavefront, rc);
        RENDER_TRY(hipGetLastError());
        RENDER_TRY(hipMemcpyAsync(ctx->h_counts, q[nxt].counts64, sizeof(counts), hipMemcpyDeviceToHost, st));
        RENDER_TRY(hipEventRecord(ctx->ev_sync, st));
        if (rc == PBRT_HIP_OK) wait_for_counts(rc);
        counts[0] = ctx->h_counts[0];
        counts[1] = ctx->h_counts[1];
        if (n_trace > 0 && rc == PBRT_HIP_OK) {
            float ms = 0.0f;
            RENDER_TRY(hipEventElapsedTime(&ms, ev.t0, ev.t1));
            local.trace_ms += ms;
            local.trace_launches += 1;
            if (ctx->trace_log)
                std::fprintf(stderr, "[pbrt_hip] k_trace: %u rays %.3f ms (%.0f Mrays/s), k_shade: %u paths\n", n_trace, ms, n_trace / ms * 1e-3,
                             n_shade);
            ctx->trace_ms += ms;
            ctx->trace_launches += 1;
        }
        const uint64_t n_rays = counts[0] & 0xffffffffull, n_shadow = counts[0] >> 32;
        local.rays_closest += n_rays - n_shadow;
        local.rays_shadow += n_shadow;
        counts[0] = n_rays;
        wavefront += 1;
        cur = nxt;
    }
}

// stage 8b: what a finished pass leaves: radiance per ray (li), splats, or the ordered accumulation and, after the last pass, the merge
void RenderJob::film_stage(const PassParams& pp, uint32_t n_paths, bool last_pass, int& rc) {
    if (li_mode) {
        hipLaunchKernelGGL(k_li_output, dim3((unsigned)((li->n + 255) / 256)), dim3(256), 0, st, ps, (uint32_t)li->n, li->d_rgb);
        RENDER_TRY(hipGetLastError());
        return;
    }
    if (!box) {
        hipLaunchKernelGGL(k_film_splat, dim3((n_paths + 255) / 256), dim3(256), 0, st, ps, pp, tiles, d_film);
        RENDER_TRY(hipGetLastError());
        return;
    }
    if (pp.group_shift == 6)  // a wave of paths = one pixel's samples: sixteen lanes per pixel, coalesced reads, ordered row sums
        hipLaunchKernelGGL(k_film_accumulate_rows, dim3((unsigned)(((size_t)n_pix * 16 + 255) / 256)), dim3(256), 0, st, ps, pp, tiles, accum,
                           d_film);
    else
        hipLaunchKernelGGL(k_film_accumulate, dim3((n_pix + 255) / 256), dim3(256), 0, st, ps, pp, tiles, accum, d_film);
    RENDER_TRY(hipGetLastError());
    if (last_pass) {
        hipLaunchKernelGGL(k_film_merge, dim3((n_pix + 255) / 256), dim3(256), 0, st, pp, tiles, accum, d_film);
        RENDER_TRY(hipGetLastError());
    }
}

// stage 8, the driver: the plan's refusals, the stages above, then per pass the camera rays, the wavefront loop and the film
int RenderJob::run(const PbrtCamera& camera, PbrtRenderStats* stats) {
    // A refusal surfaces where it always has among the calls that can fail on the device: `upto` names the last step before the next such call
    auto refused = [&](RenderStep upto) { return refusal && refused_at <= upto; };
    if (refused(RenderStep::Params)) return invalid(refusal);
    if (d_film) HIP_TRY(ctx, hipMemsetAsync(d_film, 0, (size_t)rp.width * rp.height * 4 * sizeof(float), st));
    if (refused(RenderStep::Tiles)) return invalid(refusal);
    if (origins.empty()) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (stats) *stats = local;
        return PBRT_HIP_OK;
    }
    if (!hip_ok(ctx, mem_query, "hipMemGetInfo(&free_b, &total_b)")) return PBRT_HIP_ERR_DEVICE;
    if (refused(RenderStep::RayOrder)) return invalid(refusal);
    if (int rc = query_sort_sizes(RenderStep::RayOrder)) return rc;
    if (refused(RenderStep::ShadeOrder)) return invalid(refusal);
    if (int rc = query_sort_sizes(RenderStep::ShadeOrder)) return rc;
    if (refusal) return invalid(refusal);

    // the device blocks of the call: released (or, on a lost context, kept for good) when this frame ends, after the drain below
    DevBuf buf(ctx);
    bool ok = true;
    alloc_path_buffers(buf, &ok);
    if (int rc = setup_sampler(buf, &ok)) return rc;
    int* d_prefix = buf.alloc<int>(prefix.size(), &ok);
    if (direct) {
        ds.stage = buf.alloc<int>(N, &ok);
        ds.ld_acc = buf.alloc<float4>(N, &ok);
        ds.frames = buf.alloc<float4>(N * (size_t)std::max(1, rp.max_depth) * 3, &ok);
        ds.light_strategy = ds_light_strategy;
        ds.mode = ds_mode;
        ds.ao_samples = ds_ao_samples;
        ds.ao_cos_sample = ds_ao_cos_sample;
    }
    if (!box) {
        d_filter = buf.alloc<float>(256, &ok);
        if (ok) HIP_TRY(ctx, hipMemcpyAsync(d_filter, rp.filter_table, 256 * sizeof(float), hipMemcpyHostToDevice, st));
    }
    accum = buf.alloc<float4>(n_pix, &ok);
    int2* d_origins = buf.alloc<int2>(origins.size(), &ok);
    if (!ok) return PBRT_HIP_ERR_OOM;
    HIP_TRY(ctx, hipMemcpyAsync(d_origins, origins.data(), origins.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(accum, 0, (size_t)n_pix * sizeof(float4), st));
    HIP_TRY(ctx, hipMemcpyAsync(d_prefix, prefix.data(), prefix.size() * sizeof(int), hipMemcpyHostToDevice, st));
    tiles = TileList{d_origins, (int)origins.size()};

    std::memcpy(cam.c2w, camera.camera_to_world, 64);
    std::memcpy(cam.r2c, camera.raster_to_camera, 64);
    cam.lens_radius = camera.lens_radius;
    cam.focal_distance = camera.focal_distance;
    cam.shutter_open = camera.shutter_open;
    cam.shutter_close = camera.shutter_close;
    cam.kind = camera.kind;

    // the scene's tables and, from them, this render's shading kernels (kernel_select.h)
    const SceneNeeds needs = scene_needs(s);
    scene_shade_consts(s, &sc);
    sc.light_sample_prefix = d_prefix;
    sc.total_light_samples = prefix.back();
    if (int rc = setup_light_distribution(needs)) return rc;
    if (direct) {
        shade_direct = direct_kernel(needs, rp.integrator);
    } else {
        shade_path[0] = path_kernel(needs, false);
        shade_path[1] = path_kernel(needs, true);
    }

    RenderEvents ev;
    if (!ev.create(ctx)) return PBRT_HIP_ERR_DEVICE;
    int rc = PBRT_HIP_OK;
    RENDER_TRY(hipEventRecord(ev.begin, st));
    bool tables_ready = !tabulated || rp.sampler == PBRT_SAMPLER_HALTON;
    for (int s0 = 0; s0 < rp.spp && rc == PBRT_HIP_OK; s0 += spp_pass) {
        const PassParams pp = pass_params(s0);
        const uint32_t n_paths = (uint32_t)n_pix * pp.n_samples;
        if (!tables_ready) {  // Sampler::start_pixel for every pixel of this GPU, once per render
            hipLaunchKernelGGL(k_sampler_tables, dim3((n_pix + 63) / 64), dim3(64), 0, st, pp, tiles);
            RENDER_TRY(hipGetLastError());
            tables_ready = true;
        }
        if (li_mode)
            hipLaunchKernelGGL(k_li_generate, dim3((n_paths + 255) / 256), dim3(256), 0, st, ps, q[0], li->d_rays, li->d_keys, (uint32_t)li->n,
                               n_paths, li->skip);
        else if (const int key = generate_key(s->moving, camera_motion != nullptr); key & kGenerateCameraAnimated)
            hipLaunchKernelGGL(generate_camera_kernel(key), dim3((n_paths + 255) / 256), dim3(256), 0, st, ps, q[0], pp, cam, *camera_motion, tiles);
        else
            hipLaunchKernelGGL(generate_kernel(key), dim3((n_paths + 255) / 256), dim3(256), 0, st, ps, q[0], pp, cam, tiles);
        RENDER_TRY(hipGetLastError());
        if (export_mode) {
            hipLaunchKernelGGL(k_camera_rays_out, dim3((n_paths + 255) / 256), dim3(256), 0, st, ps, pp, tiles, li->out_rays, li->out_keys,
                               li->out_pfilm, li->out_pixel_sample);
            RENDER_TRY(hipGetLastError());
            break;
        }
        if (direct) {
            RENDER_TRY(hipMemsetAsync(ds.stage, 0, (size_t)n_paths * sizeof(int), st));
            RENDER_TRY(hipMemsetAsync(ds.ld_acc, 0, (size_t)n_paths * sizeof(float4), st));
        }
        run_wavefronts(ev, pp, n_paths, rc);
        film_stage(pp, n_paths, s0 + spp_pass >= rp.spp, rc);
    }
    RENDER_TRY(hipEventRecord(ev.end, st));
    // Nothing of this call may still run when its buffers go back to the cache: drain the stream, also after an error
    // (an asynchronous fault of the last kernels surfaces here). After the deadline the stream is presumed hung: it is
    // not waited on, the context is lost and the buffers are never reused (DevBuf).
    if (!ctx->lost) {
        const hipError_t drained = hipStreamSynchronize(st);
        if (rc == PBRT_HIP_OK && !hip_ok(ctx, drained, "hipStreamSynchronize (end of render)")) rc = PBRT_HIP_ERR_DEVICE;
    }
    if (rc == PBRT_HIP_OK) {
        float ms = 0.0f;
        RENDER_TRY(hipEventElapsedTime(&ms, ev.begin, ev.end));
        local.total_ms = ms;
    }
    if (stats) *stats = local;
    return rc;
}
}  // namespace

int wavefront_render(PbrtHipScene* s, const PbrtCamera& camera, const PbrtRenderParams& rp_in, float* d_film,
                     PbrtRenderStats* stats, const LiBatch* li, const DevMotion* camera_motion) {
    PbrtHipContext* ctx = s->ctx;
    const RenderCall call = li && li->d_rays ? RenderCall::Li : li && li->out_rays ? RenderCall::Export : RenderCall::Frame;
    RenderSceneFacts facts;
    std::memcpy(facts.root_min, s->d.bvh.root_min, sizeof(facts.root_min));
    std::memcpy(facts.root_max, s->d.bvh.root_max, sizeof(facts.root_max));
    facts.n_lights = s->d.n_lights;
    facts.light_samples = s->light_samples.data();
    // The plan is one function, so what it reads of the device is fetched here, ahead of every refusal; what stays at its old
    // place among the refusals is where a FAILURE of these calls is reported (RenderJob::run). choose_trace writes a refusal
    // straight into last_error: it is moved aside into trace_refusal (last_error keeps what it held) and comes back through the
    // plan only when its turn among the refusals is reached. A render refused for its parameters, or one without tiles, now pays
    // a hipMemGetInfo it did not pay before.
    std::string trace_refusal = ctx->last_error;
    const TraceChoice trace = choose_trace(s);
    if (!trace.ok) {
        std::swap(trace_refusal, ctx->last_error);
        facts.trace_refusal = trace_refusal.c_str();
    }
    // the free device bytes, where the caller leaves the pass size to the library (li and export fix it themselves)
    size_t free_b = 0, total_b = 0;
    hipError_t mem_query = hipSuccess;
    if (call == RenderCall::Frame && rp_in.spp_per_pass <= 0) {
        mem_query = hipMemGetInfo(&free_b, &total_b);
        for (const auto& b : ctx->block_cache)
            if (!b.in_use) free_b += b.bytes;  // blocks kept from the previous render are available to this one
    }
    RenderJob job{plan_render(rp_in, call, li ? li->n : 0, camera.kind, facts, free_b), s, ctx, ctx->stream, li, d_film, camera_motion, trace, mem_query};
    return job.run(camera, stats);
}
#undef RENDER_TRY

#ifdef PB_LANE_STATS
extern "C" int pbrt_hip_debug_wide_stats(unsigned long long* out24, int reset) try {
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(pb::g_wide_stats), 32 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pb::g_wide_stats), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
PB_ABI_CATCH
extern "C" int pbrt_hip_debug_lane_stats(unsigned long long* out8, int reset) try {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(pb::g_lane_stats), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pb::g_lane_stats), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
PB_ABI_CATCH
#endif
