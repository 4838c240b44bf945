// pbrt_hip.hip — C ABI (include/pbrt_hip.h) over the gfx950 kernels.
//
// Stands in for the reference's Integrator / Primitive / Scene trait objects:
//   pbrt_hip_scene_create   Scene::new, src/core/scene.rs:18-34
//   pbrt_hip_intersect[_p]  Scene::intersect / intersect_p, src/core/scene.rs:40-46
//   pbrt_hip_render         SamplerIntegrator::render, src/core/integrator.rs:399-480
#include <hip/hip_runtime.h>
#include "abi_guard.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_edit.h"
#include "host_motion.h"
#include "host_scene.h"
#include "host_wide.h"
#include "kernel_select.h"
#include "motion.h"
#include "scene.h"
#include "staging.h"
#include "trace.h"
#include "trace_persistent.h"
#include "trace_wide.h"
#include "trace_stackless.h"

using namespace pb;

// why the calling THREAD's last pbrt_hip_context_create failed (pbrt_hip_last_error(NULL)): contexts may be created from several
// host threads at once, and a failed creation has no context to carry its message
static thread_local std::string g_create_error;
namespace pb {
void set_thread_error(const std::string& message) { g_create_error = message; }  // host_motion.h: entry points without a context
}



// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
extern "C" int pbrt_hip_context_create(int device_id, PbrtHipContext** out) try {
    if (!out) return PBRT_HIP_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_create_error = "no HIP device visible: the MI355X kernels cannot run (there is no CPU fallback)";
        return PBRT_HIP_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= n) {
        g_create_error = "device_id out of range";
        return PBRT_HIP_ERR_INVALID;
    }
    PbrtHipContext* ctx = new PbrtHipContext();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) {
        g_create_error = "hipSetDevice failed";
        delete ctx;
        return PBRT_HIP_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) {
        g_create_error = "hipGetDeviceProperties failed";
        delete ctx;
        return PBRT_HIP_ERR_DEVICE;
    }
    ctx->n_cus = prop.multiProcessorCount;
    ctx->trace_log = std::getenv("PBRT_HIP_TRACE_LOG") != nullptr;  // read once, here: the render loop asks per wavefront
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipMalloc((void**)&ctx->d_counters, 8 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&ctx->d_work_counter, kWorkCounters * sizeof(unsigned int)) != hipSuccess ||
        hipHostMalloc((void**)&ctx->h_counts, 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_sync, hipEventDisableTiming) != hipSuccess ||
        hipMemset(ctx->d_counters, 0, 8 * sizeof(unsigned long long)) != hipSuccess) {
        g_create_error = "stream / event creation failed";
        delete ctx;
        return PBRT_HIP_ERR_DEVICE;
    }
    *out = ctx;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" void pbrt_hip_context_destroy(PbrtHipContext* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->lost) {
        // a kernel of an abandoned call may never finish: waiting on the stream or freeing what it writes (hipFree waits
        // for the device) could block for ever. The device memory of a lost context goes back with the process.
        delete ctx;
        return;
    }
    if (ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->d_work_counter) (void)hipFree(ctx->d_work_counter);
    if (ctx->d_special_list) (void)hipFree(ctx->d_special_list);
    for (auto& b : ctx->block_cache)
        if (b.ptr) (void)hipFree(b.ptr);
    ctx->block_cache.clear();
    if (ctx->h_counts) (void)hipHostFree(ctx->h_counts);
    if (ctx->ev_sync) (void)hipEventDestroy(ctx->ev_sync);
    if (ctx->d_halton_primes) (void)hipFree(ctx->d_halton_primes);
    if (ctx->d_halton_perms) (void)hipFree(ctx->d_halton_perms);
    delete ctx;
}

extern "C" int pbrt_hip_context_is_lost(const PbrtHipContext* ctx) try {
    return ctx ? (ctx->lost.load(std::memory_order_acquire) ? 1 : 0) : -1;  // no lock: `lost` is atomic (polled from other threads)
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_set_deadline(PbrtHipContext* ctx, double seconds) try {
    if (!ctx || !(seconds > 0.0)) return PBRT_HIP_ERR_INVALID;
    PB_LOCK(ctx);
    ctx->wavefront_deadline_s = seconds;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" const char* pbrt_hip_last_error(const PbrtHipContext* ctx) {
    return ctx ? ctx->last_error.c_str() : g_create_error.c_str();
}

extern "C" int pbrt_hip_synchronize(PbrtHipContext* ctx) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_trace_timing(PbrtHipContext* ctx, int reset, double* total_ms, uint64_t* launches) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    if (total_ms) *total_ms = ctx->trace_ms;
    if (launches) *launches = ctx->trace_launches;
    if (reset) {
        ctx->trace_ms = 0.0;
        ctx->trace_launches = 0;
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_set_counting(PbrtHipContext* ctx, int enable) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    ctx->count_traversal = (enable == 1 || enable == 2) ? enable : 0;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_set_wide_build(PbrtHipContext* ctx, int where) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    if (where < PBRT_WIDE_BUILD_DEVICE || where > PBRT_WIDE_BUILD_NONE) {
        ctx->last_error = "wide build must be PBRT_WIDE_BUILD_DEVICE, _HOST or _NONE";
        return PBRT_HIP_ERR_INVALID;
    }
    ctx->wide_build = where;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_set_wide_layout(PbrtHipContext* ctx, int layout) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    if (layout < PBRT_WIDE_LAYOUT_AUTO || layout > PBRT_WIDE_LAYOUT_LINES) {
        ctx->last_error = "wide layout must be PBRT_WIDE_LAYOUT_AUTO, _PACKED or _LINES";
        return PBRT_HIP_ERR_INVALID;
    }
    ctx->wide_layout = layout;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_set_camera_packets(PbrtHipContext* ctx, int mode) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    if (mode < PBRT_CAMERA_PACKETS_AUTO || mode > PBRT_CAMERA_PACKETS_OFF) {
        ctx->last_error = "camera packets must be PBRT_CAMERA_PACKETS_AUTO or _OFF";
        return PBRT_HIP_ERR_INVALID;
    }
    ctx->camera_packets = mode;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_camera_kernel(PbrtHipContext* ctx) try {
    if (!ctx) return -1;
    PB_LOCK(ctx);
    return ctx->camera_kernel;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_wide_stride(const PbrtHipScene* s) try {
    return s ? (s->has_wide ? s->wide.vec_stride * 16 : 0) : -1;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_context_set_traversal(PbrtHipContext* ctx, int traversal) try {
    if (!ctx) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    if (traversal < PBRT_TRAVERSAL_AUTO || traversal > PBRT_TRAVERSAL_STACKLESS) {
        ctx->last_error = "traversal must be PBRT_TRAVERSAL_AUTO, _STACK or _STACKLESS";
        return PBRT_HIP_ERR_INVALID;
    }
    ctx->traversal = traversal;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_get_counters(PbrtHipContext* ctx, int reset, uint64_t counters[4]) try {
    if (!ctx || !counters) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpy(h, ctx->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    counters[0] = h[2];
    counters[1] = h[0];
    counters[2] = h[1];
    counters[3] = h[3];
    if (reset) {
        HIP_TRY(ctx, hipMemset(ctx->d_counters, 0, sizeof(h)));
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_get_wide_counters(PbrtHipContext* ctx, int reset, uint64_t counters[4]) try {
    if (!ctx || !counters) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpy(h, ctx->d_counters + 4, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) counters[k] = h[k];
    if (reset) {
        HIP_TRY(ctx, hipMemset(ctx->d_counters + 4, 0, sizeof(h)));
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// ------------------------------------------------------------------------------------
// scene
//
// Every pbrt_hip_scene_create* entry point fills a SceneDesc (host_scene.h) and goes through three phases: scene_invalid
// checks the description, plan_scene lays every table out in host arrays (both host_scene.cpp, no device call), and
// upload_scene below puts the plan on the device.
// ------------------------------------------------------------------------------------
namespace pb {
// Sphere::new (sphere.rs:222-223): theta_min = acos(clamp(z_min / radius, -1, 1)), theta_max likewise, with the device's acos
__global__ void k_shape_angles(DevShape* shapes, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = shapes[i].radius;
    shapes[i].theta_min = det_acos(clampf(shapes[i].z_min / r, -1.0f, 1.0f));
    shapes[i].theta_max = det_acos(clampf(shapes[i].z_max / r, -1.0f, 1.0f));
}
}  // namespace pb

// The plan's tables on the device, every one but the wide records and the spill slab.
static void upload_tables(PbrtHipScene* s, const SceneDesc& desc, ScenePlan& plan, bool* ok) {
    PbrtHipContext* ctx = s->ctx;
    DevSceneData& d = s->d;
    const int32_t n_lights = desc.n_lights, n_materials = desc.n_materials;
    if (DeviceTree* dt = desc.dt) {
        d.bvh.inodes = dt->inodes;
        d.bvh.tris = dt->tris;
        d.slot_prim = dt->slot_prim;
        s->allocs.push_back(dt->inodes);
        s->allocs.push_back(dt->tris);
        s->allocs.push_back(dt->slot_prim);
        dt->inodes = dt->tris = nullptr;  // owned by the scene from here on
        dt->slot_prim = nullptr;
    } else {
        d.bvh.inodes = (const float4*)dev_upload(s, plan.inodes.data(), plan.inodes.size(), ok);
        d.bvh.tris = (const float4*)dev_upload(s, plan.tris.data(), plan.tris.size(), ok);
        d.slot_prim = desc.instanced() ? dev_upload(s, plan.slot_prim.data(), plan.slot_prim.size(), ok)
                                       : dev_upload(s, desc.prim_order, (size_t)desc.n_prims(), ok);
    }
    if (!plan.shapes.empty()) {
        const int n_shapes = (int)plan.shapes.size();
        DevShape* d_rows = dev_upload(s, plan.shapes.data(), plan.shapes.size(), ok);
        if (*ok) {  // theta_min / theta_max with the kernels' own acos
            hipLaunchKernelGGL(k_shape_angles, dim3((n_shapes + 63) / 64), dim3(64), 0, ctx->stream, d_rows, n_shapes);
            *ok = hip_ok(ctx, hipGetLastError(), "k_shape_angles") && hip_ok(ctx, hipStreamSynchronize(ctx->stream), "k_shape_angles");
        }
        d.bvh.shapes = d_rows;
    }
    if (!plan.curves.empty()) d.curves = dev_upload(s, plan.curves.data(), plan.curves.size(), ok);
    if (desc.instanced()) {
        d.bvh.objects = (const float4*)dev_upload(s, plan.objects.data(), plan.objects.size(), ok);
        d.bvh.instances = (const float4*)dev_upload(s, plan.top_slot_records.data(), plan.top_slot_records.size(), ok);
        d.slot_instance = dev_upload(s, plan.slot_inst.data(), plan.slot_inst.size(), ok);
        s->n_instances = desc.ia.n_instances;
        if (!plan.motions.empty()) {
            s->d_motions = dev_upload(s, plan.motions.data(), plan.motions.size(), ok);
            s->moving = true;
        }
    }
    d.materials = dev_upload(s, plan.materials.data(), plan.materials.size(), ok);
    {
        std::vector<DevDisney> dz(n_materials, DevDisney{});  // pbrt_hip_scene_set_disney_material fills a row's block
        d.disney = dev_upload(s, dz.data(), dz.size(), ok);
        s->h_lobe_rows.assign(n_materials, DevLobeRow{});  // pbrt_hip_scene_set_lobe_material fills a row's list
        s->h_lobe_origin.assign(n_materials, 0);
        d.lobe_rows = dev_upload(s, s->h_lobe_rows.data(), s->h_lobe_rows.size(), ok);
    }
    d.lights = dev_upload(s, plan.lights.data(), plan.lights.size(), ok);
    if (plan.light_maps) d.light_maps = dev_upload(s, plan.light_map_rows.data(), plan.light_map_rows.size(), ok);
    s->light_allocs.assign(n_lights, {});
    d.infinite_ids = dev_upload(s, plan.infinite_ids.data(), plan.infinite_ids.size(), ok);
    if (n_lights > 0) {
        d.light_distrib_uniform.func = dev_upload(s, plan.uniform_func.data(), plan.uniform_func.size(), ok);
        d.light_distrib_uniform.cdf = dev_upload(s, plan.uniform_cdf.data(), plan.uniform_cdf.size(), ok);
        d.light_distrib_power.func = dev_upload(s, plan.power_func.data(), plan.power_func.size(), ok);
        d.light_distrib_power.cdf = dev_upload(s, plan.power_cdf.data(), plan.power_cdf.size(), ok);
    }
    // the host copies the scene keeps
    s->glossy = plan.glossy;
    s->light_maps = plan.light_maps;
    s->h_lights = std::move(plan.lights);
    s->h_materials = std::move(plan.materials);
    s->row_off_curve = std::move(plan.row_off_curve);
    s->h_light_maps = std::move(plan.light_map_rows);
    s->light_fov = std::move(plan.light_fov);
    s->light_samples = std::move(plan.light_samples);
}

// ---- 4-wide quantised records over the same tree (wide_bvh.h). Each of the three builders below leaves its device arrays
// in *w (n_records >= 0) or the reason the scene keeps the binary records only; false: a device call failed. ----

// A tree from the host: its flat nodes go up once, the records are laid out on the device from them and from the triangle
// records already there (wide_gpu.hip; the host builder produces the same bytes, tens of ms per million triangles slower:
// PBRT_WIDE_BUILD_HOST).
static bool wide_on_device(PbrtHipContext* ctx, const SceneDesc& desc, const float4* d_tris, pb::WideDeviceTree* w) {
    bool up = true;
    Staging flat(ctx);  // only the builder needs it
    const PbrtLinearBVHNode* d_flat = dev_copy(ctx, desc.nodes, (size_t)desc.n_nodes, &up);
    flat.adopt((void*)d_flat);
    return up && pb::build_wide_tree_device(ctx, d_flat, desc.n_nodes, (const float*)d_tris, desc.n_prims(),
                                            desc.nodes[0], w, &w->reason);
}

static bool wide_on_host(PbrtHipContext* ctx, const PbrtLinearBVHNode* nodes, int32_t n_nodes, const float* tris, int32_t n_prims,
                         pb::WideDeviceTree* w) {
    pb::WideTree wt;
    if ((w->reason = pb::build_wide_tree(nodes, n_nodes, tris, n_prims, &wt))) return true;
    bool ok = true;
    w->nodes = dev_copy(ctx, wt.nodes.data(), wt.nodes.size(), &ok);
    w->tris = dev_copy(ctx, wt.tris.data(), wt.tris.size(), &ok);
    w->leaf_boxes = dev_copy(ctx, wt.leaf_boxes.data(), wt.leaf_boxes.size(), &ok);
    w->root_ref = wt.root_ref;
    w->n_records = wt.n_records;
    w->stack_need = wt.stack_need;
    return ok;
}

// Two levels: besides the three arrays, the top-level entries, their boxes and the object table go up, and the scene's
// WideTrees gets the scalars of the two-level walk.
static bool wide_two_level_on_host(PbrtHipScene* s, const SceneDesc& desc, const ScenePlan& plan, pb::WideDeviceTree* w) {
    pb::TwoLevelWide tw;
    if ((w->reason = pb::plan_two_level_wide(desc, plan, &tw))) return true;
    bool ok = true;
    w->nodes = dev_copy(s->ctx, tw.nodes.data(), tw.nodes.size(), &ok);
    w->tris = dev_copy(s->ctx, tw.tris.data(), tw.tris.size(), &ok);
    w->leaf_boxes = dev_copy(s->ctx, tw.leaf_boxes.data(), tw.leaf_boxes.size(), &ok);
    w->root_ref = tw.root_ref;
    w->n_records = tw.n_records;
    w->stack_need = tw.stack_need;
    s->wide.top_slots = (const float4*)dev_upload(s, tw.top_slots.data(), tw.top_slots.size(), &ok);
    s->wide.top_boxes = (const float4*)dev_upload(s, tw.top_boxes.data(), tw.top_boxes.size(), &ok);
    s->wide.objects = (const float4*)dev_upload(s, tw.objects.data(), tw.objects.size(), &ok);
    s->wide.slot_tris = s->d.bvh.tris;
    s->wide.general_top = s->d.bvh.general_top;
    s->wide.obj0_root = tw.obj0_root;
    std::memcpy(s->wide.obj0_min, desc.ia.objects[0].nodes[0].bounds_min, 12);
    std::memcpy(s->wide.obj0_max, desc.ia.objects[0].nodes[0].bounds_max, 12);
    return ok;
}

// The scene takes the three arrays over.
static void adopt_wide(PbrtHipScene* s, pb::WideDeviceTree* w, bool instanced, int* spill_entries) {
    s->wide.nodes = (const uint4*)w->nodes;
    s->wide.tris = (const float4*)w->tris;
    s->wide.leaf_boxes = (const float4*)w->leaf_boxes;
    s->allocs.push_back(w->nodes);
    s->allocs.push_back(w->tris);
    s->allocs.push_back(w->leaf_boxes);
    w->nodes = nullptr;
    w->tris = w->leaf_boxes = nullptr;
    s->wide.root_ref = w->root_ref;
    s->n_wide_records = w->n_records;
    s->has_wide = true;
    if (!instanced) s->wide_stack_need = w->stack_need;
    *spill_entries = std::max(*spill_entries, w->stack_need + 1 - (instanced ? pb::wide_stack_lds(1) : kWideStackLds));
}

// Single-level triangle scenes and two-level scenes in which nothing moves get wide records, from the device tree that
// brought them, from the device builder, or from the host builder; PBRT_WIDE_BUILD_NONE keeps the scene on the binary records.
static bool obtain_wide(PbrtHipScene* s, const SceneDesc& desc, const ScenePlan& plan, int* spill_entries) {
    PbrtHipContext* ctx = s->ctx;
    DeviceTree* dt = desc.dt;
    pb::WideDeviceTree built;
    pb::WideDeviceTree* w = &built;
    bool ok = true;
    if (ctx->wide_build == PBRT_WIDE_BUILD_NONE) {
        built.reason = "disabled by PBRT_WIDE_BUILD_NONE";
    } else if (desc.n_curves > 0) {
        built.reason = "scene with curves";
    } else if (desc.sa.n_shapes > 0) {
        built.reason = "scene with shapes";
    } else if (desc.sa.n > 0) {
        built.reason = "scene with spheres";
    } else if (s->moving) {
        built.reason = "scene with moving instances";
    } else if (dt && dt->wide.n_records >= 0) {
        w = &dt->wide;  // laid out on the device beside the tree (wide_gpu.hip)
    } else if (dt && dt->h_nodes.empty()) {
        built.reason = dt->wide_reason ? dt->wide_reason : "tree built on the device: no wide records";
    } else if (desc.instanced()) {
        ok = wide_two_level_on_host(s, desc, plan, &built);
    } else if (!dt && ctx->wide_build != PBRT_WIDE_BUILD_HOST) {
        ok = wide_on_device(ctx, desc, s->d.bvh.tris, &built);
    } else {
        ok = dt ? wide_on_host(ctx, dt->h_nodes.data(), dt->n_nodes, dt->h_tris.data(), desc.n_prims(), &built)
                : wide_on_host(ctx, desc.nodes, desc.n_nodes, plan.tris.data(), desc.n_prims(), &built);
    }
    if (!ok) return false;
    if (w->n_records >= 0) adopt_wide(s, w, desc.instanced(), spill_entries);
    else if (w->reason) s->wide_reason = w->reason;
    return true;
}

// One 64-byte line per record / wide-order triangle (wide_bvh.h: kWideLineAlignBytes): a builder's packed array is spread on
// the device and released. Returns the spread array, which replaces the packed one among the scene's allocations, or nullptr.
static void* spread_array(PbrtHipScene* s, const void* packed, size_t count) {
    PbrtHipContext* ctx = s->ctx;
    void* out = nullptr;
    count = count ? count : 1;
    if (!hip_ok(ctx, hipMalloc(&out, count * 64), "hipMalloc wide lines")) return nullptr;
    if (!hip_ok(ctx, hipMemset(out, 0, count * 64), "hipMemset") ||
        !hip_ok(ctx, hipMemcpy2D(out, 64, packed, 48, 48, count, hipMemcpyDeviceToDevice), "hipMemcpy2D")) {
        (void)hipFree(out);
        return nullptr;
    }
    (void)hipFree(const_cast<void*>(packed));
    std::replace(s->allocs.begin(), s->allocs.end(), const_cast<void*>(packed), out);
    return out;
}
// Each pointer is replaced as soon as its array was spread: the scene never names a released array.
static bool spread_to_lines(PbrtHipScene* s, int32_t n_prims) {
    void* n4 = spread_array(s, s->wide.nodes, (size_t)std::max(s->n_wide_records, 1));
    if (!n4) return false;
    s->wide.nodes = (const uint4*)n4;
    void* t4 = spread_array(s, s->wide.tris, (size_t)n_prims);
    if (!t4) return false;
    s->wide.tris = (const float4*)t4;
    s->wide.vec_stride = 4;
    return true;
}

static int upload_scene(PbrtHipContext* ctx, const SceneDesc& desc, ScenePlan& plan, PbrtHipScene** out) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t n_prims = desc.n_prims();
    PbrtHipScene* s = new PbrtHipScene();
    s->ctx = ctx;
    s->n_tris = desc.n_tris;
    s->n_nodes = desc.dt ? desc.dt->n_nodes : desc.n_nodes;
    s->n_interior = plan.n_interior;
    s->d = plan.d;
    bool ok = true;
    upload_tables(s, desc, plan, &ok);
    int spill_entries = kStackSpill;
    ok = ok && obtain_wide(s, desc, plan, &spill_entries);
    // lines where the tree is too large for L2; pbrt_hip_context_set_wide_layout overrides
    s->wide.vec_stride = 3;
    if (s->has_wide && ok) {
        const size_t packed_bytes = ((size_t)std::max(s->n_wide_records, 1) + (size_t)n_prims) * 48;
        // (two-level scenes stay packed: the trees of a scene of instances are small, and trace_wide<.., INST> keeps its compile-time stride)
        const bool lines = !desc.instanced() && (ctx->wide_layout == PBRT_WIDE_LAYOUT_LINES || (ctx->wide_layout == PBRT_WIDE_LAYOUT_AUTO && packed_bytes > pb::kWideLineAlignBytes));
        if (lines) ok = spread_to_lines(s, n_prims);
    }
    // spill slab for the deepest stack entries of every resident lane of the traversal grid
    s->spill_lanes = ctx->n_cus * 2048;
    if (ok) {
        void* p = nullptr;
        if (!hip_ok(ctx, hipMalloc(&p, (size_t)s->spill_lanes * spill_entries * sizeof(uint2)), "hipMalloc spill")) ok = false;
        else s->allocs.push_back(p);
        s->d.bvh.spill = (uint2*)p;
        s->d.bvh.spill_stride = s->spill_lanes;
        s->wide.spill = (uint2*)p;
        s->wide.spill_stride = s->spill_lanes;
    }
    if (!ok) {
        pbrt_hip_scene_destroy(s);
        return PBRT_HIP_ERR_DEVICE;
    }
    *out = s;
    return PBRT_HIP_OK;
}

// The three phases, as every entry point but the device-tree one runs them.
static int create_scene(PbrtHipContext* ctx, const SceneDesc& desc, PbrtHipScene** out) {
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    *out = nullptr;
    std::string why = scene_invalid(desc);
    if (!why.empty()) {
        ctx->last_error = why;
        return PBRT_HIP_ERR_INVALID;
    }
    ScenePlan plan;
    plan_scene(desc, &plan);
    return upload_scene(ctx, desc, plan, out);
}

extern "C" int pbrt_hip_scene_create(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                     const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                     const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                     const PbrtLight* lights, int32_t n_lights, const PbrtLinearBVHNode* nodes,
                                     int32_t n_nodes, const int32_t* prim_order, PbrtHipScene** out) try {
    SceneDesc desc{positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights, n_lights, nodes, n_nodes, prim_order};
    return create_scene(ctx, desc, out);
}
PB_ABI_CATCH

namespace pb {
int hlbvh_build_scene_tree(PbrtHipContext* ctx, const float* positions, int32_t n_verts, const int32_t* indices,
                           int32_t n_tris, const int32_t* tri_material, const int32_t* tri_light, const PbrtLight* lights,
                           int32_t n_lights, int32_t max_prims_in_node, DeviceTree* out);
}

// Scene::new with BVHAccel::new(HLBVH) built and laid out on the device: only the mesh goes up.
extern "C" int pbrt_hip_scene_create_hlbvh(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                           const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                           const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                           const PbrtLight* lights, int32_t n_lights, int32_t max_prims_in_node,
                                           PbrtHipScene** out, double* build_ms, double* layout_ms) try {
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    *out = nullptr;
    SceneDesc desc{positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights, n_lights};
    desc.device_tree = true;
    // the description is checked before the build: the device builder takes the mesh and the light table as they are
    std::string why = scene_invalid(desc);
    if (!why.empty()) {
        ctx->last_error = why;
        return PBRT_HIP_ERR_INVALID;
    }
    pb::DeviceTree dt;  // frees whatever the scene does not take over
    int rc = pb::hlbvh_build_scene_tree(ctx, positions, n_verts, indices, n_tris, tri_material, tri_light, lights, n_lights,
                                        max_prims_in_node, &dt);
    if (rc != PBRT_HIP_OK) return rc;
    if (build_ms) *build_ms = dt.build_ms;
    if (layout_ms) *layout_ms = dt.convert_ms;
    desc.dt = &dt;
    ScenePlan plan;
    plan_scene(desc, &plan);
    return upload_scene(ctx, desc, plan, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_with_spheres(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                                  const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                                  const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                                  const PbrtLight* lights, int32_t n_lights, const float* spheres,
                                                  const int32_t* sphere_material, const int32_t* sphere_light, int32_t n_spheres,
                                                  const PbrtLinearBVHNode* nodes, int32_t n_nodes, const int32_t* prim_order,
                                                  PbrtHipScene** out) try {
    SceneDesc desc{positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights, n_lights, nodes, n_nodes, prim_order};
    desc.sa.spheres = spheres;
    desc.sa.material = sphere_material;
    desc.sa.light = sphere_light;
    desc.sa.n = n_spheres;
    return create_scene(ctx, desc, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_with_shapes(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                                 const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                                 const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                                 const PbrtLight* lights, int32_t n_lights, const PbrtShape* shapes,
                                                 int32_t n_shapes, const PbrtLinearBVHNode* nodes, int32_t n_nodes,
                                                 const int32_t* prim_order, PbrtHipScene** out) try {
    SceneDesc desc{positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights, n_lights, nodes, n_nodes, prim_order};
    desc.sa.shapes = shapes;
    desc.sa.n_shapes = n_shapes;
    return create_scene(ctx, desc, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_with_curves(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                                 const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                                 const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                                 const PbrtLight* lights, int32_t n_lights, const PbrtShape* shapes,
                                                 int32_t n_shapes, const PbrtCurve* curves, int32_t n_curves,
                                                 const PbrtLinearBVHNode* nodes, int32_t n_nodes, const int32_t* prim_order,
                                                 PbrtHipScene** out) try {
    SceneDesc desc{positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights, n_lights, nodes, n_nodes, prim_order};
    desc.sa.shapes = shapes;
    desc.sa.n_shapes = n_shapes;
    desc.curves = curves;
    desc.n_curves = n_curves;
    return create_scene(ctx, desc, out);
}
PB_ABI_CATCH

// pbrt_hip_scene_create_two_level(_moving): the combined mesh (host_scene.cpp), then the three phases. A refusal of the
// arguments is reported before the context is entered.
static int create_two_level(PbrtHipContext* ctx, const TwoLevelArgs& a, PbrtHipScene** out) {
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    CombinedMesh m;
    if (const char* why = combine_two_level(a, &m)) {
        ctx->last_error = why;
        return PBRT_HIP_ERR_INVALID;
    }
    // (no one node array: the trees are the objects' and the top-level one; n_nodes is the objects' total)
    SceneDesc desc{m.pos.data(), (int32_t)m.pos.size() / 3, m.idx.data(), (int32_t)m.mat.size(), m.mat.data(), a.materials, a.n_materials,
                   m.lgt.data(), a.lights, a.n_lights, nullptr, m.n_nodes, m.order.data(), SphereArgs(), std::move(m.ia)};
    return create_scene(ctx, desc, out);
}

extern "C" int pbrt_hip_scene_create_two_level(PbrtHipContext* ctx, const PbrtObject* objects, int32_t n_objects,
                                               const PbrtInstance* instances, const int32_t* instance_object, int32_t n_instances,
                                               const float* world_positions, int32_t n_world_verts, const int32_t* world_indices,
                                               int32_t n_world_tris, const int32_t* world_tri_material,
                                               const int32_t* world_tri_light, const PbrtMaterial* materials, int32_t n_materials,
                                               const PbrtLight* lights, int32_t n_lights, const PbrtLinearBVHNode* tlas_nodes,
                                               int32_t n_tlas_nodes, const int32_t* tlas_order, PbrtHipScene** out) try {
    return create_two_level(ctx, {objects, n_objects, instances, nullptr, instance_object, n_instances, world_positions, n_world_verts,
                                  world_indices, n_world_tris, world_tri_material, world_tri_light, materials, n_materials, lights, n_lights,
                                  tlas_nodes, n_tlas_nodes, tlas_order}, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_two_level_moving(PbrtHipContext* ctx, const PbrtObject* objects, int32_t n_objects,
                                                      const PbrtInstance* instances, const PbrtInstanceMotion* motions,
                                                      const int32_t* instance_object, int32_t n_instances,
                                                      const float* world_positions, int32_t n_world_verts,
                                                      const int32_t* world_indices, int32_t n_world_tris,
                                                      const int32_t* world_tri_material, const int32_t* world_tri_light,
                                                      const PbrtMaterial* materials, int32_t n_materials, const PbrtLight* lights,
                                                      int32_t n_lights, const PbrtLinearBVHNode* tlas_nodes, int32_t n_tlas_nodes,
                                                      const int32_t* tlas_order, PbrtHipScene** out) try {
    // a scene in which nothing moves is pbrt_hip_scene_create_two_level's scene: same records, same kernels
    bool any = false;
    for (int32_t i = 0; motions && i < n_instances; ++i) any = any || motions[i].animated != 0;
    return create_two_level(ctx, {objects, n_objects, instances, any ? motions : nullptr, instance_object, n_instances, world_positions,
                                  n_world_verts, world_indices, n_world_tris, world_tri_material, world_tri_light, materials, n_materials,
                                  lights, n_lights, tlas_nodes, n_tlas_nodes, tlas_order}, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_instanced(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                               const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                               const PbrtMaterial* materials, int32_t n_materials,
                                               const PbrtLight* lights, int32_t n_lights,
                                               const PbrtLinearBVHNode* blas_nodes, int32_t n_blas_nodes,
                                               const int32_t* blas_order, const PbrtInstance* instances,
                                               int32_t n_instances, const PbrtLinearBVHNode* tlas_nodes,
                                               int32_t n_tlas_nodes, const int32_t* tlas_order, PbrtHipScene** out) try {
    const PbrtObject obj{positions, n_verts, indices, n_tris, tri_material, blas_nodes, n_blas_nodes, blas_order};
    return create_two_level(ctx, {&obj, 1, instances, nullptr, nullptr, n_instances, nullptr, 0, nullptr, 0, nullptr, nullptr, materials, n_materials,
                                  lights, n_lights, tlas_nodes, n_tlas_nodes, tlas_order}, out);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_wide_records(const PbrtHipScene* s, int32_t* n_records, const char** reason) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    if (n_records) *n_records = s->has_wide ? s->n_wide_records : -1;
    if (reason) *reason = s->wide_reason.c_str();
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// Copies a single-level scene's wide records back: n_records x 12 dwords, n_slots x 12 floats (wide-order triangles),
// n_slots x 8 floats (leaf boxes). A diagnostic entry point (declared as such in include/pbrt_hip.h): the test that the device
// builder (wide_gpu.hip) and the host builder (host_wide.cpp) produce the same bytes reads the arrays through it.
extern "C" int pbrt_hip_debug_wide_export(PbrtHipScene* s, uint32_t* nodes, float* tris, float* boxes, int32_t n_slots) try {
    if (!s || !s->has_wide || s->d.bvh.instanced || n_slots != s->d.bvh.n_slots) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the packed form, whatever the stride on the device (WideTrees::vec_stride)
    if (nodes && s->n_wide_records > 0)
        HIP_TRY(ctx, hipMemcpy2D(nodes, 48, s->wide.nodes, (size_t)s->wide.vec_stride * 16, 48, (size_t)s->n_wide_records, hipMemcpyDeviceToHost));
    if (tris) HIP_TRY(ctx, hipMemcpy2D(tris, 48, s->wide.tris, (size_t)s->wide.vec_stride * 16, 48, (size_t)n_slots, hipMemcpyDeviceToHost));
    if (boxes) HIP_TRY(ctx, hipMemcpy(boxes, s->wide.leaf_boxes, (size_t)n_slots * 32, hipMemcpyDeviceToHost));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

extern "C" void pbrt_hip_scene_destroy(PbrtHipScene* s) {
    if (!s) return;
    PB_LOCK(s->ctx);
    (void)hipSetDevice(s->ctx->device);
    if (!s->ctx->lost) {  // a lost context: an abandoned kernel may still read the scene, and waiting for it may never end
        (void)hipStreamSynchronize(s->ctx->stream);
        for (void* p : s->allocs) (void)hipFree(p);
        for (auto& a : s->light_allocs)
            for (void* p : a) (void)hipFree(p);
    }
    delete s;
}

// ---- scene edits. Every pbrt_hip_scene_set_* entry point enters through PB_EDIT (a null scene is refused, the context is
// entered, invalid(why) refuses the call under its own name), has host_edit.cpp check the call and compute what it writes (no
// device call there), lists the writes in a SceneEdit, applies them and commits the scene's host copies. ----
#define PB_EDIT(s, name)                                \
    if (!(s)) return PBRT_HIP_ERR_INVALID;              \
    PbrtHipContext* ctx = (s)->ctx;                     \
    PB_ENTER(ctx);                                      \
    auto invalid = [ctx](const std::string& why) {      \
        ctx->last_error = std::string(name ": ") + why; \
        return PBRT_HIP_ERR_INVALID;                    \
    }

namespace {
// One edit of the scene's device tables: the writes it makes (host_edit.h: apply_writes) and the device arrays it brings. They
// are freed with the edit unless a light takes them over (write_light) or a failed rollback leaves them to the scene.
struct SceneEdit {
    PbrtHipScene* s;
    std::vector<DeviceWrite> writes;
    std::vector<void*> fresh;
    bool uploaded = true;  // every upload() so far arrived
    ~SceneEdit() {
        for (void* p : fresh) (void)hipFree(p);
    }
    // nothing reads the tables while they change
    int begin() {
        PbrtHipContext* ctx = s->ctx;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PBRT_HIP_OK;
    }
    template <class T>
    const T* upload(const std::vector<T>& v) {
        T* p = uploaded ? dev_copy(s->ctx, v.data(), v.size(), &uploaded) : nullptr;
        if (p) fresh.push_back(p);
        return p;
    }
    int apply() {
        PbrtHipContext* ctx = s->ctx;
        auto copy = [ctx](void* dst, const void* src, size_t bytes) {
            return hip_ok(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy");
        };
        const Applied a = apply_writes(writes, copy, &ctx->last_error);
        if (a == Applied::kTorn) {  // the device may still name the fresh arrays: they stay allocated until the scene is destroyed
            s->allocs.insert(s->allocs.end(), fresh.begin(), fresh.end());
            fresh.clear();
        }
        return a == Applied::kDone ? PBRT_HIP_OK : PBRT_HIP_ERR_DEVICE;
    }
};
}  // namespace

// Row `material` of the material table, written after the block of its kind that it names (DevDisney, DevLobeRow), and the host
// copies: the row, who wrote it, and which shading-kernel level the table needs beyond plastic / metal.
static int write_material(PbrtHipScene* s, int32_t material, const DevMaterial& m, int origin, const DeviceWrite* block = nullptr) {
    SceneEdit edit{s};
    if (int rc = edit.begin()) return rc;
    if (block) edit.writes.push_back(*block);
    edit.writes.push_back({(void*)(s->d.materials + material), &m, &s->h_materials[material], sizeof(DevMaterial)});
    if (int rc = edit.apply()) return rc;
    s->h_materials[material] = m;
    s->h_lobe_origin[material] = origin;
    s->bxdfs = s->disney = s->lobes = s->hair = false;
    for (const DevMaterial& row : s->h_materials) {
        s->hair = s->hair || row.type == kMatHair;
        s->lobes = s->lobes || row.type == kMatLobes;
        s->bxdfs = s->bxdfs || (row.type >= kMatOrenNayar && row.type <= kMatSubstrate);
        s->disney = s->disney || row.type == kMatDisney;
    }
    return PBRT_HIP_OK;
}

// Light `light` changed: its descriptor, its row and the power distribution go to the device from one consistent host state.
// Then the arrays of a map set before on this light are freed and the edit's take their place, the host copies follow, and a
// spatial light table already built is dropped (the next render with that strategy builds it again).
static int write_light(SceneEdit& edit, int light, const DevLight& lt, const DeviceWrite& descriptor) {
    PbrtHipScene* s = edit.s;
    const size_t n = (size_t)s->d.n_lights;
    const PowerEdit p = power_edit(s->h_lights, (int)n, light, lt.power_y);
    edit.writes = {descriptor,
                   {(void*)(s->d.lights + light), &lt, &s->h_lights[light], sizeof(DevLight)},
                   {(void*)s->d.light_distrib_power.func, p.func.data(), p.old_func.data(), n * sizeof(float)},
                   {(void*)s->d.light_distrib_power.cdf, p.cdf.data(), p.old_cdf.data(), (n + 1) * sizeof(float)}};
    if (int rc = edit.apply()) return rc;
    s->d.light_distrib_power.func_int = p.func_int;
    for (void* q : s->light_allocs[light]) (void)hipFree(q);
    s->light_allocs[light] = std::move(edit.fresh);
    edit.fresh.clear();
    s->h_lights[light] = lt;
    if (s->d_spatial) {
        (void)hipFree(s->d_spatial);
        s->allocs.erase(std::remove(s->allocs.begin(), s->allocs.end(), (void*)s->d_spatial), s->allocs.end());
        s->d_spatial = nullptr;
    }
    return PBRT_HIP_OK;
}

// TrowbridgeReitzDistribution::new(alpha_u, alpha_v, true) of a plastic / metal material with pbrt-v3's remaproughness switch
// (plastic.cpp / metal.cpp): the alphas of material `material` are replaced in the device table and its host copy.
extern "C" int pbrt_hip_scene_set_material_roughness(PbrtHipScene* s, int32_t material, float u_roughness, float v_roughness,
                                                     int32_t remap) try {
    PB_EDIT(s, "pbrt_hip_scene_set_material_roughness");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevMaterial m;
    if (const char* why = roughness_row(s->h_materials[material], u_roughness, v_roughness, remap != 0, &m)) return invalid(why);
    return write_material(s, material, m, 0);
}
PB_ABI_CATCH

// pbrt-v3's MatteMaterial (sigma), GlassMaterial (roughness) and SubstrateMaterial on the reference's OrenNayar,
// MicrofacetReflection / MicrofacetTransmission and FresnelBlend (reflection.rs:917-975, 977-1192, 1194-1280): row `material`
// of the device table and of its host copy is replaced by what the descriptor reduces to. A descriptor an existing
// PbrtMaterialType expresses becomes that row; the others become a kMatOrenNayar / kMatRoughGlass / kMatSubstrate row
// (scene.h), which the shading kernels' level-2 instantiations shade (wf_bxdfs.h).
extern "C" int pbrt_hip_scene_set_material(PbrtHipScene* s, int32_t material, const PbrtMaterialDesc* desc) try {
    PB_EDIT(s, "pbrt_hip_scene_set_material");
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevMaterial m{};
    if (const char* why = row_of_desc(*desc, &m)) return invalid(why);
    return write_material(s, material, m, 0);
}
PB_ABI_CATCH

// pbrt-v3's DisneyMaterial without subsurface (include/pbrt_hip.h): row `material` becomes a kMatDisney row
// and its DevDisney block (scene.h) gets the lobes' constants (host_edit.cpp). The shading kernels' level-3 instantiations
// shade it (wf_disney.h). The block has no host copy: a kMatDisney row is what names it, and the row is written after it.
extern "C" int pbrt_hip_scene_set_disney_material(PbrtHipScene* s, int32_t material, const PbrtDisneyDesc* desc) try {
    PB_EDIT(s, "pbrt_hip_scene_set_disney_material");
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevDisney z;
    DevMaterial m;
    const std::string why = disney_of_desc(*desc, &z, &m);
    if (!why.empty()) return invalid(why);
    const DeviceWrite block{(void*)(s->d.disney + material), &z, nullptr, sizeof(DevDisney)};
    return write_material(s, material, m, 0, &block);
}
PB_ABI_CATCH

// pbrt-v3's HairMaterial (include/pbrt_hip.h): row `material` becomes a kMatHair row and its DevHair block
// (scene.h), which lives in the row's slot of the Disney table, gets the lobes' constants (host_edit.cpp). The hair builds shade
// it (wf_hair.h, hair_kernels.hip). As with a Disney row the block has no host copy: the row, written after it, is what names it.
extern "C" int pbrt_hip_scene_set_hair_material(PbrtHipScene* s, int32_t material, const PbrtHairDesc* desc) try {
    PB_EDIT(s, "pbrt_hip_scene_set_hair_material");
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevHair z;
    DevMaterial m;
    const std::string why = hair_of_desc(*desc, &z, &m);
    if (!why.empty()) return invalid(why);
    if (!s->d.curves) return invalid("the scene holds no curves (pbrt_hip_scene_create_with_curves): a hair row needs a curve's v");
    if (s->row_off_curve[material]) return invalid("a triangle or a quadric shape names the row: only curves carry the v a hair row reads");
    const DeviceWrite block{(void*)(s->d.disney + material), &z, nullptr, sizeof(DevHair)};
    return write_material(s, material, m, 0, &block);
}
PB_ABI_CATCH

// scene_needs (kernel_select.h) as the render driver reads it, for callers and tests that want to know which builds a render runs
extern "C" int pbrt_hip_scene_shading_needs(const PbrtHipScene* s, int32_t out[8]) try {
    if (!s || !out) return PBRT_HIP_ERR_INVALID;
    PB_LOCK(s->ctx);
    const SceneNeeds n = scene_needs(s);
    const int32_t v[8] = {n.shapes, n.light_maps, n.level, n.lobes, n.moving, n.curves, n.hair, 0};
    std::memcpy(out, v, sizeof(v));
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// pbrt-v3's UberMaterial, TranslucentMaterial and MixMaterial (include/pbrt_hip.h): row `material` becomes a
// kMatLobes row and its DevLobeRow (scene.h) gets the list host_lobes.cpp makes of the descriptor. The shading kernels' lobe-list
// builds shade it (wf_lobes.h). A mix copies its operands' lists as they are now.
extern "C" int pbrt_hip_scene_set_lobe_material(PbrtHipScene* s, int32_t material, const PbrtLobeMaterialDesc* desc) try {
    PB_EDIT(s, "pbrt_hip_scene_set_lobe_material");
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevLobeRow row;
    DevMaterial m;
    const std::string why = lobe_row_of_desc(*desc, {s->h_materials, s->h_lobe_rows, s->h_lobe_origin, s->d.bvh.has_spheres == 2, s->light_maps, s->moving}, &row, &m);
    if (!why.empty()) return invalid(why);
    const DeviceWrite block{(void*)(s->d.lobe_rows + material), &row, &s->h_lobe_rows[material], sizeof(DevLobeRow)};
    if (int rc = write_material(s, material, m, desc->type, &block)) return rc;
    s->h_lobe_rows[material] = row;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// InfiniteAreaLight::new(light_to_world, L, n_samples, texmap) (lights/infinite.rs:36-82) with the texels in memory: the map's
// tables (host_envmap.cpp) go to the device for light `light`, and its power and the power distribution are recomputed.
extern "C" int pbrt_hip_scene_set_environment_map(PbrtHipScene* s, int32_t light, const float* rgb, int32_t width, int32_t height,
                                                  const float light_to_world[16]) try {
    PB_EDIT(s, "pbrt_hip_scene_set_environment_map");
    if (light < 0 || light >= s->d.n_lights) return invalid("light index out of range");
    if (s->h_lights[light].type != PBRT_LIGHT_INFINITE) return invalid("light is not PBRT_LIGHT_INFINITE");
    if (!light_to_world) return invalid("null light_to_world");
    DevEnvMap e{};
    if (const char* why = envmap_transform(light_to_world, &e)) return invalid(why);
    EnvTables t;
    if (const char* why = envmap_build(rgb, width, height, s->h_lights[light].L, &t)) return invalid(why);

    SceneEdit edit{s};
    if (int rc = edit.begin()) return rc;
    e.texels = edit.upload(texels_of_rgb(t.level0));
    e.func = edit.upload(t.func);
    e.cdf = edit.upload(t.cdf);
    e.row_int = edit.upload(t.row_int);
    e.marg_cdf = edit.upload(t.marg_cdf);
    e.marg_int = t.marg_int;
    e.w = t.w;
    e.h = t.h;
    e.nu = t.nu;
    e.nv = t.nv;
    if (edit.uploaded && !s->d.env_maps) {  // the scene's first map: the descriptors, one per light
        s->h_env.assign(s->d.n_lights, DevEnvMap{});
        s->d.env_maps = dev_upload(s, s->h_env.data(), s->h_env.size(), &edit.uploaded);
    }
    if (!edit.uploaded) return PBRT_HIP_ERR_DEVICE;
    DevLight lt = s->h_lights[light];
    lt.slot = light;
    lt.power_y = envmap_power_y(t, s->d.world_radius);
    if (int rc = write_light(edit, light, lt, {(void*)(s->d.env_maps + light), &e, &s->h_env[light], sizeof(DevEnvMap)})) return rc;
    s->h_env[light] = e;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// ProjectionLight::new / GonioPhotometricLight::new (lights/projection.rs:36-88, goniometric.rs:32-63) with the texels in memory:
// level 0 of the map's MIPMap goes to the device for light `light`, the projector's window follows the map's aspect, and the
// light's power (D89) and the power distribution are recomputed.
extern "C" int pbrt_hip_scene_set_light_map(PbrtHipScene* s, int32_t light, const float* rgb, int32_t width, int32_t height) try {
    PB_EDIT(s, "pbrt_hip_scene_set_light_map");
    if (light < 0 || light >= s->d.n_lights) return invalid("light index out of range");
    const int type = s->h_lights[light].type;
    if (type != PBRT_LIGHT_PROJECTION && type != PBRT_LIGHT_GONIOMETRIC) return invalid("light is not PBRT_LIGHT_PROJECTION or PBRT_LIGHT_GONIOMETRIC");
    if (!rgb) return invalid("null pointer");
    LightMapTables t;
    if (const char* why = light_map_build(type, s->light_fov[light], rgb, width, height, &t)) return invalid(why);

    SceneEdit edit{s};
    if (int rc = edit.begin()) return rc;
    DevLightMap m{};
    m.texels = edit.upload(texels_of_rgb(t.level0));
    if (!edit.uploaded) return PBRT_HIP_ERR_DEVICE;
    m.w = t.w;
    m.h = t.h;
    m.inv_tan = t.inv_tan;
    std::memcpy(m.screen_bounds, t.screen_bounds, sizeof(m.screen_bounds));
    DevLight lt = s->h_lights[light];
    if (type == PBRT_LIGHT_PROJECTION) lt.cos_total_width = t.cos_total_width;
    lt.power_y = light_map_power_y(t, lt.L);
    if (int rc = write_light(edit, light, lt, {(void*)(s->d.light_maps + light), &m, &s->h_light_maps[light], sizeof(DevLightMap)})) return rc;
    s->h_light_maps[light] = m;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// ------------------------------------------------------------------------------------
// batch intersect
// ------------------------------------------------------------------------------------
// Persistent-threads traversal (trace_persistent.h) over a caller-supplied ray batch
template <bool ANY>
struct BatchRayIO {
    const int* __restrict__ slot_prim;
    const int* __restrict__ slot_instance;
    const PbrtRay* __restrict__ rays;
    uint32_t count;
    PbrtHit* __restrict__ out_hits;
    uint8_t* __restrict__ out_flags;
    PB_DEV uint32_t n() const { return count; }
    PB_DEV int segments() const { return 1; }
    PB_DEV uint32_t token(uint32_t i) const { return i; }  // a batch ray's token is its position
    PB_DEV bool strict(uint32_t) const { return false; }   // pbrt_hip_intersect_p is Primitive::intersect_p
    PB_DEV bool load(uint32_t i, TravRay* r, bool* any) const {
        const float4* rp = reinterpret_cast<const float4*>(rays + i);
        float4 a = rp[0], b = rp[1];
        *r = TravRay{a.x, a.y, a.z, a.w, b.x, b.y, b.z};
        *any = ANY;
        return true;
    }
    // the MOV builds also take PbrtRay.time, as given
    PB_DEV bool load(uint32_t i, TravRay* r, bool* any, float* time) const {
        const float4* rp = reinterpret_cast<const float4*>(rays + i);
        float4 a = rp[0], b = rp[1];
        *r = TravRay{a.x, a.y, a.z, a.w, b.x, b.y, b.z};
        *any = ANY;
        *time = b.w;
        return true;
    }
    PB_DEV void store(uint32_t i, bool any, bool found, float t, float b0, float b1, float b2, int slot, int inst) const {
        if (ANY) {
            out_flags[i] = found ? 1 : 0;
        } else {
            float4 o0 = make_float4(found ? t : kInf, found ? b0 : 0.0f, found ? b1 : 0.0f, found ? b2 : 0.0f);
            int prim = found ? slot_prim[slot] : -1;
            int instance = (found && inst >= 0) ? slot_instance[inst] : -1;
            float4* op = reinterpret_cast<float4*>(out_hits + i);
            op[0] = o0;
            op[1] = make_float4(__int_as_float(prim), __int_as_float(instance), 0.0f, 0.0f);
        }
    }
};
template <bool ANY, bool COUNT, int INST, bool SPH = false>
__global__ void __launch_bounds__(kTraceBlock, (COUNT || SPH) ? 4 : (INST ? PB_INST_WAVES : PB_TRACE_WAVES))
    k_intersect_batch(DevBVH bvh, BatchRayIO<ANY> io, unsigned int* work_counter, unsigned long long* counters) {
    __shared__ uint2 lds_stack[kStackLds * kTraceBlock];
    trace_persistent<BatchRayIO<ANY>, COUNT, INST, SPH>(bvh, io, work_counter, lds_stack + threadIdx.x,
                                                        blockIdx.x * kTraceBlock + threadIdx.x, counters);
}

// scenes with general quadric shapes (shapes_quadric.h): single level, the leaf loop dispatches on the shape table
template <bool ANY, bool COUNT>
__global__ void __launch_bounds__(kTraceBlock, 4)
    k_intersect_batch_shapes(DevBVH bvh, BatchRayIO<ANY> io, unsigned int* work_counter, unsigned long long* counters) {
    __shared__ uint2 lds_stack[kStackLds * kTraceBlock];
    trace_persistent<BatchRayIO<ANY>, COUNT, 0, false, true>(bvh, io, work_counter, lds_stack + threadIdx.x,
                                                             blockIdx.x * kTraceBlock + threadIdx.x, counters);
}

// the binary records without a stack (trace_stackless.h)
template <bool ANY>
__global__ void __launch_bounds__(kTraceBlock, PB_STACKLESS_WAVES)
    k_intersect_batch_stackless(DevBVH bvh, BatchRayIO<ANY> io, unsigned int* work_counter) {
    trace_stackless<BatchRayIO<ANY>>(bvh, io, work_counter);
}

// the same batch over the 4-wide records (trace_wide.h), and the follow-up over the rays that kernel left out
template <bool ANY, bool COUNT, int INST = 0>
__global__ void __launch_bounds__(kTraceBlock, (COUNT || INST) ? PB_WIDE_INST_WAVES : PB_WIDE_WAVES)
    k_intersect_batch_wide(WideTrees wt, BatchRayIO<ANY> io, unsigned int* work_counter, unsigned long long* counters) {
    __shared__ uint2 lds_stack[wide_stack_lds(INST) * kTraceBlock];
    __shared__ float lds_world[INST ? kWideWorldFloats * kTraceBlock : 1];
    trace_wide<BatchRayIO<ANY>, COUNT, INST>(wt, io, work_counter, lds_stack + threadIdx.x, blockIdx.x * kTraceBlock + threadIdx.x,
                                             counters, lds_world + (INST ? threadIdx.x : 0));
}
template <bool ANY, int INST = 0>
__global__ void __launch_bounds__(kTraceBlock, INST ? PB_INST_WAVES : PB_TRACE_WAVES)
    k_intersect_batch_special(DevBVH bvh, SpecialListIO<BatchRayIO<ANY>> io, unsigned int* work_counter) {
    if ((unsigned long long)blockIdx.x * (kTraceBlock / 64) * kChunk >= (unsigned long long)io.n()) return;  // see k_trace_special
    __shared__ uint2 lds_stack[kStackLds * kTraceBlock];
    trace_persistent<SpecialListIO<BatchRayIO<ANY>>, false, INST, false>(bvh, io, work_counter, lds_stack + threadIdx.x,
                                                                         blockIdx.x * kTraceBlock + threadIdx.x, nullptr);
}

// two-level scenes with moving instances (trace_persistent's MOV builds; INST 1 or 2). Named after every older kernel: the
// code generated for some kernels depends on the order in which the instantiations are met (kernel_select.h).
#ifndef PB_MOVING_WAVES
#define PB_MOVING_WAVES 4  // 128 registers: the interpolation's ~40 live values on top of the two-level walk
#endif
template <bool ANY, bool COUNT, int INST>
__global__ void __launch_bounds__(kTraceBlock, PB_MOVING_WAVES)
    k_intersect_batch_moving(DevBVH bvh, const DevMotion* __restrict__ motions, BatchRayIO<ANY> io, unsigned int* work_counter,
                             unsigned long long* counters) {
    __shared__ uint2 lds_stack[kStackLds * kTraceBlock];
    trace_persistent<BatchRayIO<ANY>, COUNT, INST, false, false, true>(bvh, io, work_counter, lds_stack + threadIdx.x,
                                                                       blockIdx.x * kTraceBlock + threadIdx.x, counters, motions);
}

// scenes with curves (shapes_curve.h): the build for shapes with the curve test beside the quadrics'. Behind every older kernel, as above.
#ifndef PB_CURVE_WAVES
#define PB_CURVE_WAVES 3  // profiles/curve_resource_usage.txt
#endif
template <bool ANY, bool COUNT>
__global__ void __launch_bounds__(kTraceBlock, PB_CURVE_WAVES)
    k_intersect_batch_curves(DevBVH bvh, const DevCurve* __restrict__ curves, BatchRayIO<ANY> io, unsigned int* work_counter,
                             unsigned long long* counters) {
    __shared__ uint2 lds_stack[kStackLds * kTraceBlock];
    trace_persistent<BatchRayIO<ANY>, COUNT, 0, false, true, false, true>(bvh, io, work_counter, lds_stack + threadIdx.x,
                                                                          blockIdx.x * kTraceBlock + threadIdx.x, counters, nullptr, curves);
}

template <bool ANY>
static int launch_batch(PbrtHipScene* s, const PbrtRay* d_rays, int64_t n, PbrtHit* d_hits, uint8_t* d_flags) {
    PbrtHipContext* ctx = s->ctx;
    if (n == 0) return PBRT_HIP_OK;
    if (n >= (1ll << 32) - kChunk * 8192ll) {
        ctx->last_error = "batch too large for one launch (split it below 2^32 rays)";
        return PBRT_HIP_ERR_INVALID;
    }
    const TraceChoice choice = choose_trace(s);
    if (!choice.ok) return PBRT_HIP_ERR_INVALID;
    const bool wide = choice.kind == TraceKind::Wide;
    if (wide && ctx->special_capacity < (size_t)n) {  // room for the queue positions of the rays the wide kernel leaves out
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_special_list) (void)hipFree(ctx->d_special_list);
        ctx->d_special_list = nullptr;
        ctx->special_capacity = 0;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_special_list, (size_t)n * sizeof(uint32_t)));
        ctx->special_capacity = (size_t)n;
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_work_counter, 0, kWorkCounters * sizeof(unsigned int), ctx->stream));
    if (ctx->time_trace) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const BatchRayIO<ANY> io{s->d.slot_prim, s->d.slot_instance, d_rays, (uint32_t)n, d_hits, d_flags};
    dispatch(choice, [&](auto kind, auto count, auto inst) {
        constexpr TraceKind K = decltype(kind)::value;
        constexpr bool COUNT = decltype(count)::value;
        constexpr int INST = decltype(inst)::value;
        const dim3 grid(persistent_grid(s)), block(kTraceBlock);
        if constexpr (K == TraceKind::Stackless) {
            hipLaunchKernelGGL((k_intersect_batch_stackless<ANY>), dim3(stackless_grid(s)), block, 0, ctx->stream, s->d.bvh, io, ctx->d_work_counter);
        } else if constexpr (K == TraceKind::Wide) {  // the wide kernel, then the follow-up over the rays it left out
            WideTrees wt = s->wide;
            wt.special_list = ctx->d_special_list;
            wt.special_count = ctx->d_work_counter + kSpecialCount;
            const SpecialListIO<BatchRayIO<ANY>> sio{io, ctx->d_special_list, ctx->d_work_counter + kSpecialCount};
            hipLaunchKernelGGL((k_intersect_batch_wide<ANY, COUNT, INST>), dim3(wide_grid<COUNT, INST>(s)), block, 0, ctx->stream, wt, io,
                               ctx->d_work_counter, ctx->d_counters);
            hipLaunchKernelGGL((k_intersect_batch_special<ANY, INST>), grid, block, 0, ctx->stream, s->d.bvh, sio, ctx->d_work_counter + kFollowUpCounter);
        } else if constexpr (K == TraceKind::Shapes) {
            hipLaunchKernelGGL((k_intersect_batch_shapes<ANY, COUNT>), grid, block, 0, ctx->stream, s->d.bvh, io, ctx->d_work_counter, ctx->d_counters);
        } else if constexpr (K == TraceKind::Moving) {
            hipLaunchKernelGGL((k_intersect_batch_moving<ANY, COUNT, INST>), dim3(persistent_grid(s, PB_MOVING_WAVES)), block, 0, ctx->stream,
                               s->d.bvh, s->d_motions, io, ctx->d_work_counter, ctx->d_counters);
        } else if constexpr (K == TraceKind::Curves) {
            hipLaunchKernelGGL((k_intersect_batch_curves<ANY, COUNT>), dim3(persistent_grid(s, PB_CURVE_WAVES)), block, 0, ctx->stream, s->d.bvh,
                               s->d.curves, io, ctx->d_work_counter, ctx->d_counters);
        } else {
            hipLaunchKernelGGL((k_intersect_batch<ANY, COUNT, INST, K == TraceKind::Spheres>), grid, block, 0, ctx->stream, s->d.bvh, io,
                               ctx->d_work_counter, ctx->d_counters);
        }
    });
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->time_trace) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->trace_ms += ms;
        ctx->trace_launches += 1;
    }
    return PBRT_HIP_OK;
}

extern "C" int pbrt_hip_intersect_device(PbrtHipScene* s, const PbrtRay* d_rays, int64_t n, PbrtHit* d_out) try {
    if (!s || n < 0 || (n > 0 && (!d_rays || !d_out))) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(s->ctx);
    HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    return launch_batch<false>(s, d_rays, n, d_out, nullptr);
}
PB_ABI_CATCH
extern "C" int pbrt_hip_intersect_p_device(PbrtHipScene* s, const PbrtRay* d_rays, int64_t n, uint8_t* d_out) try {
    if (!s || n < 0 || (n > 0 && (!d_rays || !d_out))) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(s->ctx);
    HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    return launch_batch<true>(s, d_rays, n, nullptr, d_out);
}
PB_ABI_CATCH

template <bool ANY>
static int intersect_host(PbrtHipScene* s, const PbrtRay* rays, int64_t n, void* out) {
    if (!s || n < 0 || (n > 0 && (!rays || !out))) return PBRT_HIP_ERR_INVALID;
    if (n == 0) return PBRT_HIP_OK;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t out_bytes = ANY ? (size_t)n : (size_t)n * sizeof(PbrtHit);
    Staging dev(ctx);
    PbrtRay* d_rays = dev.alloc<PbrtRay>((size_t)n);
    char* d_out = dev.alloc<char>(out_bytes);
    if (dev.failed) return PBRT_HIP_ERR_DEVICE;
    int rc = PBRT_HIP_OK;
    if (!dev.upload(d_rays, rays, (size_t)n * sizeof(PbrtRay), true)) rc = PBRT_HIP_ERR_DEVICE;
    if (rc == PBRT_HIP_OK) rc = launch_batch<ANY>(s, d_rays, n, (PbrtHit*)d_out, (uint8_t*)d_out);
    if (rc == PBRT_HIP_OK && !dev.download(out, d_out, out_bytes, true)) rc = PBRT_HIP_ERR_DEVICE;
    if (!hip_ok(ctx, hipStreamSynchronize(ctx->stream), "sync") && rc == PBRT_HIP_OK) rc = PBRT_HIP_ERR_DEVICE;
    return rc;
}
extern "C" int pbrt_hip_intersect(PbrtHipScene* s, const PbrtRay* rays, int64_t n, PbrtHit* out) try {
    return intersect_host<false>(s, rays, n, out);
}
PB_ABI_CATCH
extern "C" int pbrt_hip_intersect_p(PbrtHipScene* s, const PbrtRay* rays, int64_t n, uint8_t* out) try {
    return intersect_host<true>(s, rays, n, out);
}
PB_ABI_CATCH
