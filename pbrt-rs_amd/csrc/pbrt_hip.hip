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

#include "host_envmap.h"
#include "host_lobes.h"
#include "host_motion.h"
#include "host_wide.h"
#include "kernel_select.h"
#include "motion.h"
#include "scene.h"
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
// ------------------------------------------------------------------------------------
static float tri_area(const float* a, const float* b, const float* c) {  // triangle.rs:323-328
    float e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = b[k] - a[k];
        e2[k] = c[k] - a[k];
    }
    float cx = e1[1] * e2[2] - e1[2] * e2[1];
    float cy = e1[2] * e2[0] - e1[0] * e2[2];
    float cz = e1[0] * e2[1] - e1[1] * e2[0];
    return std::sqrt(cx * cx + cy * cy + cz * cz) * 0.5f;
}

// Distribution1D::new (sampling.rs:69-93), intended (D40)
static void make_distribution(const std::vector<float>& f, std::vector<float>* cdf, float* func_int) {
    int n = (int)f.size();
    cdf->assign(n + 1, 0.0f);
    for (int i = 1; i < n + 1; ++i) (*cdf)[i] = (*cdf)[i - 1] + f[i - 1] / (float)n;
    *func_int = (*cdf)[n];
    if (*func_int == 0.0f) {
        for (int i = 1; i < n + 1; ++i) (*cdf)[i] = (float)i / (float)n;
    } else {
        for (int i = 1; i < n + 1; ++i) (*cdf)[i] /= *func_int;
    }
}

// host replica of det_sincos (dev_math.h) for the env light's sin-weighted table
static float host_det_sin(float x) {
    float q = x * 0.63661977236758134308f;
    float k = __builtin_rintf(q);
    float r = __builtin_fmaf(-k, 1.5707397460937500f, x);
    r = __builtin_fmaf(-k, 5.6579709053039550781e-05f, r);
    r = __builtin_fmaf(-k, 9.9209362947050294680e-10f, r);
    float z = r * r;
    float ps = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
    float sr = __builtin_fmaf(ps * z, r, r);
    float pc = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
    float cr = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    int ki = (int)k & 3;
    return (ki == 0) ? sr : (ki == 1) ? cr : (ki == 2) ? -sr : -cr;
}

// Validates one reference-order LinearBVHNode array and converts it to the device records
// (trace.h): interior nodes get indices base + 0.. in DFS order, leaves are encoded with count_bits.
struct TreeLayout {
    std::vector<float> inodes;   // 16 floats per interior node
    int n_interior = 0, count_bits = 0, depth = 0, max_count = 1;
    int32_t root_ref = 0;
};
// slot_base: leaf slot of the tree's first primitive in the scene's slot numbering; force_count_bits >= 0: the width
// of (n_primitives - 1) in the leaf references (several object trees share one width).
static const char* convert_tree(const PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t n_prims, int32_t base,
                                TreeLayout* out, int32_t slot_base = 0, int force_count_bits = -1, int64_t n_slots_total = -1) {
    std::vector<int32_t> interior_index(n_nodes, -1);
    int n_interior = 0, max_count = 1;
    int64_t leaf_prims = 0;
    for (int32_t i = 0; i < n_nodes; ++i) {
        const PbrtLinearBVHNode& nd = nodes[i];
        if (nd.n_primitives > 0) {
            if (nd.offset < 0 || (int64_t)nd.offset + nd.n_primitives > n_prims) return "leaf range outside the primitive list";
            max_count = std::max<int>(max_count, nd.n_primitives);
            leaf_prims += nd.n_primitives;
        } else {
            if (nd.axis > 2) return "interior node axis > 2";
            if (nd.offset <= i + 1 || nd.offset >= n_nodes || i + 1 >= n_nodes) return "second-child offset out of range";
            interior_index[i] = n_interior++;
        }
    }
    if (leaf_prims != n_prims) return "leaves do not cover the primitive list exactly once";
    {
        // the traversal stack holds one entry per level, 64 in all (bvh.rs:839 `nodes_to_visit = [0; 64]`, where the
        // reference would index out of bounds): refuse deeper trees instead of overrunning the spill slab
        std::vector<std::pair<int32_t, int>> st;  // (node, depth)
        st.emplace_back(0, 1);
        int max_depth = 0;
        int64_t visited = 0;
        while (!st.empty()) {
            auto [node, depth] = st.back();
            st.pop_back();
            if (++visited > n_nodes) return "node array is not a tree";
            max_depth = std::max(max_depth, depth);
            if (nodes[node].n_primitives == 0) {
                st.emplace_back(node + 1, depth + 1);
                st.emplace_back(nodes[node].offset, depth + 1);
            }
        }
        out->depth = max_depth;
    }
    if (n_interior != (n_nodes - 1) / 2 || (n_nodes & 1) == 0) return "node array is not a full binary tree";
    int count_bits = 0;
    while ((1 << count_bits) < max_count) ++count_bits;
    if (force_count_bits >= 0) {
        if (force_count_bits < count_bits) return "leaf larger than the shared leaf-reference width";
        count_bits = force_count_bits;
    }
    if (((n_slots_total >= 0 ? n_slots_total : (int64_t)n_prims) << count_bits) >= (1ll << 31)) return "scene too large for 31-bit leaf references";
    auto child_ref = [&](int32_t node) -> int32_t {
        const PbrtLinearBVHNode& nd = nodes[node];
        if (nd.n_primitives > 0)
            return ~(int32_t)(((uint32_t)(nd.offset + slot_base) << count_bits) | (uint32_t)(nd.n_primitives - 1));
        return base + interior_index[node];
    };
    out->inodes.assign((size_t)n_interior * 16, 0.0f);
    std::vector<int32_t> parent_record(n_nodes, -1);  // of interior nodes: the record holding them as a child (trace_stackless.h)
    for (int32_t i = 0; i < n_nodes; ++i) {
        if (interior_index[i] < 0) continue;
        parent_record[i + 1] = parent_record[nodes[i].offset] = base + interior_index[i];
    }
    for (int32_t i = 0; i < n_nodes; ++i) {
        if (interior_index[i] < 0) continue;
        const PbrtLinearBVHNode& c0 = nodes[i + 1];
        const PbrtLinearBVHNode& c1 = nodes[nodes[i].offset];
        float* r = &out->inodes[(size_t)interior_index[i] * 16];
        r[0] = c0.bounds_min[0]; r[1] = c0.bounds_min[1]; r[2] = c0.bounds_min[2];
        r[3] = c0.bounds_max[0]; r[4] = c0.bounds_max[1]; r[5] = c0.bounds_max[2];
        r[6] = c1.bounds_min[0]; r[7] = c1.bounds_min[1]; r[8] = c1.bounds_min[2];
        r[9] = c1.bounds_max[0]; r[10] = c1.bounds_max[1]; r[11] = c1.bounds_max[2];
        int32_t refs[4] = {child_ref(i + 1), child_ref(nodes[i].offset), (int32_t)nodes[i].axis, parent_record[i]};
        std::memcpy(r + 12, refs, 16);
    }
    out->n_interior = n_interior;
    out->count_bits = count_bits;
    out->max_count = max_count;
    out->root_ref = child_ref(0);
    return nullptr;
}

// Spheres next to the triangles (src/shapes/sphere.rs; BASELINE config 1): full spheres placed by a translation.
// Primitive ids n_tris .. n_tris + n - 1 in prim_order; not usable as area lights on the device.
struct SphereArgs {
    const float* spheres = nullptr;  // n x {centre.xyz, radius}
    const int32_t* material = nullptr;
    const int32_t* light = nullptr;  // per sphere: index of its DiffuseAreaLight or -1
    int32_t n = 0;
    // or general quadric shapes (pbrt_hip_scene_create_with_shapes): primitive ids n_tris .. n_tris + n_shapes - 1
    const PbrtShape* shapes = nullptr;
    int32_t n_shapes = 0;
};
// Two-level scenes: the main geometry arguments of scene_create_impl are then the COMBINED mesh (every object's
// triangles, object after object, then the world-space triangles) and prim_order the combined leaf order
// (object k's leaf order at obj_tri_offset[k], world triangles in caller order at world_tri_offset).
struct InstancingArgs {
    const PbrtInstance* instances = nullptr;
    int32_t n_instances = 0;
    const PbrtLinearBVHNode* tlas_nodes = nullptr;
    int32_t n_tlas_nodes = 0;
    const int32_t* tlas_order = nullptr;
    const PbrtObject* objects = nullptr;
    int32_t n_objects = 0;
    const int32_t* instance_object = nullptr;  // nullptr = all instances of object 0
    const PbrtInstanceMotion* motions = nullptr;  // pbrt_hip_scene_create_two_level_moving: one per instance, or nullptr
    std::vector<int32_t> obj_tri_offset;       // n_objects + 1
    int32_t n_world_tris = 0, world_tri_offset = 0;
};

static int scene_create_impl(PbrtHipContext* ctx, const float* positions, int32_t n_verts, const int32_t* indices,
                             int32_t n_tris, const int32_t* tri_material, const PbrtMaterial* materials,
                             int32_t n_materials, const int32_t* tri_light, const PbrtLight* lights, int32_t n_lights,
                             const PbrtLinearBVHNode* nodes, int32_t n_nodes, const int32_t* prim_order,
                             const InstancingArgs& ia, PbrtHipScene** out, pb::DeviceTree* dt = nullptr,
                             const SphereArgs& sa = SphereArgs());

extern "C" int pbrt_hip_scene_create(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                     const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                     const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                     const PbrtLight* lights, int32_t n_lights, const PbrtLinearBVHNode* nodes,
                                     int32_t n_nodes, const int32_t* prim_order, PbrtHipScene** out) try {
    return scene_create_impl(ctx, positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light,
                             lights, n_lights, nodes, n_nodes, prim_order, InstancingArgs(), out);
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
    auto fail = [&](const char* msg) {
        ctx->last_error = msg;
        return PBRT_HIP_ERR_INVALID;
    };
    // the checks scene_create_impl makes before it touches the device, needed here before the build
    if (n_tris <= 0 || n_verts <= 0) return fail("empty scene: n_tris and n_verts must be > 0");
    if (!positions || !indices) return fail("null geometry pointer");
    if (n_materials <= 0 || !materials) return fail("at least one material is required");
    if (n_lights < 0 || (n_lights > 0 && !lights)) return fail("bad light table");
    for (int64_t i = 0; i < 3 * (int64_t)n_tris; ++i)
        if (indices[i] < 0 || indices[i] >= n_verts) return fail("vertex index out of range");
    for (int32_t i = 0; i < n_lights; ++i)
        if (lights[i].type == PBRT_LIGHT_DIFFUSE_AREA && (lights[i].prim < 0 || lights[i].prim >= n_tris))
            return fail("area light triangle out of range");
    pb::DeviceTree dt;
    int rc = pb::hlbvh_build_scene_tree(ctx, positions, n_verts, indices, n_tris, tri_material, tri_light, lights, n_lights,
                                        max_prims_in_node, &dt);
    if (rc != PBRT_HIP_OK) return rc;
    if (build_ms) *build_ms = dt.build_ms;
    if (layout_ms) *layout_ms = dt.convert_ms;
    rc = scene_create_impl(ctx, positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light, lights,
                           n_lights, nullptr, 0, nullptr, InstancingArgs(), out, &dt);
    if (dt.inodes) {  // scene_create_impl failed before taking ownership
        (void)hipFree(dt.inodes);
        (void)hipFree(dt.tris);
        (void)hipFree(dt.slot_prim);
    }
    if (dt.wide.nodes) {
        (void)hipFree(dt.wide.nodes);
        (void)hipFree(dt.wide.tris);
        (void)hipFree(dt.wide.leaf_boxes);
    }
    return rc;
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_with_spheres(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                                  const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                                  const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                                  const PbrtLight* lights, int32_t n_lights, const float* spheres,
                                                  const int32_t* sphere_material, const int32_t* sphere_light, int32_t n_spheres,
                                                  const PbrtLinearBVHNode* nodes, int32_t n_nodes, const int32_t* prim_order,
                                                  PbrtHipScene** out) try {
    SphereArgs sa;
    sa.spheres = spheres;
    sa.material = sphere_material;
    sa.light = sphere_light;
    sa.n = n_spheres;
    return scene_create_impl(ctx, positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light,
                             lights, n_lights, nodes, n_nodes, prim_order, InstancingArgs(), out, nullptr, sa);
}
PB_ABI_CATCH

extern "C" int pbrt_hip_scene_create_with_shapes(PbrtHipContext* ctx, const float* positions, int32_t n_verts,
                                                 const int32_t* indices, int32_t n_tris, const int32_t* tri_material,
                                                 const PbrtMaterial* materials, int32_t n_materials, const int32_t* tri_light,
                                                 const PbrtLight* lights, int32_t n_lights, const PbrtShape* shapes,
                                                 int32_t n_shapes, const PbrtLinearBVHNode* nodes, int32_t n_nodes,
                                                 const int32_t* prim_order, PbrtHipScene** out) try {
    SphereArgs sa;
    sa.shapes = shapes;
    sa.n_shapes = n_shapes;
    return scene_create_impl(ctx, positions, n_verts, indices, n_tris, tri_material, materials, n_materials, tri_light,
                             lights, n_lights, nodes, n_nodes, prim_order, InstancingArgs(), out, nullptr, sa);
}
PB_ABI_CATCH

// pbrt_hip_scene_create_two_level and, with `motions`, pbrt_hip_scene_create_two_level_moving
static int create_two_level(PbrtHipContext* ctx, const PbrtObject* objects, int32_t n_objects, const PbrtInstance* instances,
                            const PbrtInstanceMotion* motions, const int32_t* instance_object, int32_t n_instances,
                            const float* world_positions, int32_t n_world_verts, const int32_t* world_indices, int32_t n_world_tris,
                            const int32_t* world_tri_material, const int32_t* world_tri_light, const PbrtMaterial* materials,
                            int32_t n_materials, const PbrtLight* lights, int32_t n_lights, const PbrtLinearBVHNode* tlas_nodes,
                            int32_t n_tlas_nodes, const int32_t* tlas_order, PbrtHipScene** out) {
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    auto fail = [&](const char* msg) {
        ctx->last_error = msg;
        return PBRT_HIP_ERR_INVALID;
    };
    if (!objects || n_objects <= 0 || !instances || n_instances <= 0 || !tlas_nodes || n_tlas_nodes <= 0 || !tlas_order)
        return fail("two-level scene needs objects, instances and a top-level node array");
    if (n_world_tris < 0 || n_world_verts < 0 || (n_world_tris > 0 && (!world_positions || !world_indices || n_world_verts <= 0)))
        return fail("bad world-space triangle arguments");
    // ---- the combined mesh: object after object, then the world-space triangles ----
    InstancingArgs ia;
    ia.instances = instances;
    ia.n_instances = n_instances;
    ia.tlas_nodes = tlas_nodes;
    ia.n_tlas_nodes = n_tlas_nodes;
    ia.tlas_order = tlas_order;
    ia.objects = objects;
    ia.n_objects = n_objects;
    ia.instance_object = instance_object;
    ia.motions = motions;
    ia.n_world_tris = n_world_tris;
    int64_t n_verts = 0, n_tris = 0, n_nodes = 0;
    ia.obj_tri_offset.assign(n_objects + 1, 0);
    for (int32_t k = 0; k < n_objects; ++k) {
        const PbrtObject& o = objects[k];
        if (!o.positions || !o.indices || !o.nodes || !o.prim_order || o.n_verts <= 0 || o.n_tris <= 0 || o.n_nodes <= 0)
            return fail("object aggregate with a null pointer or an empty mesh / tree");
        for (int64_t i = 0; i < 3 * (int64_t)o.n_tris; ++i)
            if (o.indices[i] < 0 || o.indices[i] >= o.n_verts) return fail("object vertex index out of range");
        for (int32_t i = 0; i < o.n_tris; ++i)
            if (o.prim_order[i] < 0 || o.prim_order[i] >= o.n_tris) return fail("object prim_order entry out of range");
        n_verts += o.n_verts;
        n_tris += o.n_tris;
        n_nodes += o.n_nodes;
        ia.obj_tri_offset[k + 1] = (int32_t)n_tris;
    }
    ia.world_tri_offset = (int32_t)n_tris;
    for (int64_t i = 0; i < 3 * (int64_t)n_world_tris; ++i)
        if (world_indices[i] < 0 || world_indices[i] >= n_world_verts) return fail("world triangle vertex index out of range");
    n_verts += n_world_verts;
    n_tris += n_world_tris;
    if (n_tris >= (1ll << 30) || n_verts >= (1ll << 31)) return fail("two-level scene too large");
    for (int32_t i = 0; i < n_instances; ++i)
        if (instance_object && (instance_object[i] < 0 || instance_object[i] >= n_objects)) return fail("instance_object out of range");
    for (int32_t i = 0; i < n_lights; ++i)
        if (lights[i].type == PBRT_LIGHT_DIFFUSE_AREA && (lights[i].prim < 0 || lights[i].prim >= n_world_tris))
            return fail("area lights sit on world-space triangles (instanced primitives cannot be area lights): prim out of range");
    std::vector<float> pos((size_t)n_verts * 3);
    std::vector<int32_t> idx((size_t)n_tris * 3), mat((size_t)n_tris, 0), lgt((size_t)n_tris, -1), order((size_t)n_tris);
    int64_t v0 = 0, t0 = 0;
    for (int32_t k = 0; k < n_objects; ++k) {
        const PbrtObject& o = objects[k];
        std::memcpy(&pos[(size_t)v0 * 3], o.positions, (size_t)o.n_verts * 12);
        for (int64_t i = 0; i < 3 * (int64_t)o.n_tris; ++i) idx[(size_t)t0 * 3 + i] = o.indices[i] + (int32_t)v0;
        for (int32_t i = 0; i < o.n_tris; ++i) {
            mat[(size_t)t0 + i] = o.tri_material ? o.tri_material[i] : 0;
            order[(size_t)t0 + i] = o.prim_order[i] + (int32_t)t0;
        }
        v0 += o.n_verts;
        t0 += o.n_tris;
    }
    if (n_world_tris > 0) {
        std::memcpy(&pos[(size_t)v0 * 3], world_positions, (size_t)n_world_verts * 12);
        for (int64_t i = 0; i < 3 * (int64_t)n_world_tris; ++i) idx[(size_t)t0 * 3 + i] = world_indices[i] + (int32_t)v0;
        for (int32_t i = 0; i < n_world_tris; ++i) {
            mat[(size_t)t0 + i] = world_tri_material ? world_tri_material[i] : 0;
            lgt[(size_t)t0 + i] = world_tri_light ? world_tri_light[i] : -1;
            order[(size_t)t0 + i] = (int32_t)t0 + i;
        }
    }
    return scene_create_impl(ctx, pos.data(), (int32_t)n_verts, idx.data(), (int32_t)n_tris, mat.data(), materials, n_materials,
                             lgt.data(), lights, n_lights, nullptr, (int32_t)n_nodes, order.data(), ia, out);
}

extern "C" int pbrt_hip_scene_create_two_level(PbrtHipContext* ctx, const PbrtObject* objects, int32_t n_objects,
                                               const PbrtInstance* instances, const int32_t* instance_object, int32_t n_instances,
                                               const float* world_positions, int32_t n_world_verts, const int32_t* world_indices,
                                               int32_t n_world_tris, const int32_t* world_tri_material,
                                               const int32_t* world_tri_light, const PbrtMaterial* materials, int32_t n_materials,
                                               const PbrtLight* lights, int32_t n_lights, const PbrtLinearBVHNode* tlas_nodes,
                                               int32_t n_tlas_nodes, const int32_t* tlas_order, PbrtHipScene** out) try {
    return create_two_level(ctx, objects, n_objects, instances, nullptr, instance_object, n_instances, world_positions, n_world_verts,
                            world_indices, n_world_tris, world_tri_material, world_tri_light, materials, n_materials, lights, n_lights,
                            tlas_nodes, n_tlas_nodes, tlas_order, out);
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
    return create_two_level(ctx, objects, n_objects, instances, any ? motions : nullptr, instance_object, n_instances, world_positions,
                            n_world_verts, world_indices, n_world_tris, world_tri_material, world_tri_light, materials, n_materials,
                            lights, n_lights, tlas_nodes, n_tlas_nodes, tlas_order, out);
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
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    PbrtObject obj;
    obj.positions = positions;
    obj.n_verts = n_verts;
    obj.indices = indices;
    obj.n_tris = n_tris;
    obj.tri_material = tri_material;
    obj.nodes = blas_nodes;
    obj.n_nodes = n_blas_nodes;
    obj.prim_order = blas_order;
    return pbrt_hip_scene_create_two_level(ctx, &obj, 1, instances, nullptr, n_instances, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                           materials, n_materials, lights, n_lights, tlas_nodes, n_tlas_nodes, tlas_order, out);
}
PB_ABI_CATCH

// roughness_to_alpha, roughness_invalid and material_invalid (the one place materials are checked): host_lobes.h

// ---- PbrtShape: what the constructors make of the arguments (Sphere::new sphere.rs:208-226, Disk::new disk.rs:24-40,
// Cylinder::new cylinder.rs:23-39): z ordered (sphere: clamped to the radius), phi_max clamped and in radians ----
static float shape_phi_max(const PbrtShape& sh) {
    float deg = sh.phi_max < 0.0f ? 0.0f : (sh.phi_max > 360.0f ? 360.0f : sh.phi_max);
    return deg * (kPi / 180.0f);
}
static void shape_z_range(const PbrtShape& sh, float* z0, float* z1) {
    float lo = sh.z_min < sh.z_max ? sh.z_min : sh.z_max, hi = sh.z_max > sh.z_min ? sh.z_max : sh.z_min;
    if (sh.type == PBRT_SHAPE_SPHERE) {
        lo = lo < -sh.radius ? -sh.radius : (lo > sh.radius ? sh.radius : lo);
        hi = hi < -sh.radius ? -sh.radius : (hi > sh.radius ? sh.radius : hi);
    }
    if (sh.type == PBRT_SHAPE_DISK) lo = hi = sh.z_min;
    *z0 = lo;
    *z1 = hi;
}
static const char* shape_invalid(const PbrtShape& sh, int32_t n_materials, int32_t n_lights) {
    if (sh.type < PBRT_SHAPE_SPHERE || sh.type > PBRT_SHAPE_CYLINDER) return "unknown shape type";
    if (!(sh.radius > 0.0f) || !std::isfinite(sh.radius)) return "shape radius must be positive";
    if (sh.type == PBRT_SHAPE_DISK && !(sh.inner_radius >= 0.0f && sh.inner_radius < sh.radius))
        return "disk inner_radius must lie in [0, radius)";
    if (!std::isfinite(sh.z_min) || (sh.type != PBRT_SHAPE_DISK && !std::isfinite(sh.z_max))) return "shape z range must be finite";
    if (sh.type == PBRT_SHAPE_CYLINDER && sh.z_min == sh.z_max) return "cylinder z_min and z_max must differ";
    if (!(sh.phi_max > 0.0f)) return "shape phi_max must be positive";
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(sh.to_world[k]) || !std::isfinite(sh.to_object[k])) return "shape transforms must be finite";
    if (sh.to_world[12] != 0.0f || sh.to_world[13] != 0.0f || sh.to_world[14] != 0.0f || sh.to_world[15] != 1.0f ||
        sh.to_object[12] != 0.0f || sh.to_object[13] != 0.0f || sh.to_object[14] != 0.0f || sh.to_object[15] != 1.0f)
        return "shape transforms must be affine (last row 0 0 0 1)";
    if (sh.material < 0 || sh.material >= n_materials) return "shape material out of range";
    if (sh.light < -1 || sh.light >= n_lights) return "shape light out of range";
    if (sh.type == PBRT_SHAPE_SPHERE && sh.light >= 0) {
        float z0, z1;
        shape_z_range(sh, &z0, &z1);
        if (z0 > -sh.radius || z1 < sh.radius || sh.phi_max < 360.0f)
            return "a partial sphere cannot carry an area light (Sphere::sample covers the full sphere)";
    }
    if (sh.type == PBRT_SHAPE_DISK && sh.light >= 0 && (sh.inner_radius > 0.0f || sh.phi_max < 360.0f))
        return "a partial disk cannot carry an area light (Disk::sample covers the full disk)";
    if (sh.light >= 0) {
        // Transform::has_scale (pbrt-v3): each transformed axis keeps its length; the same bound on the axes' mutual dot products
        // (no shear). Shape::area and the sphere's cone are object-space quantities used in world space.
        const float* m = sh.to_world;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                const float d = m[a] * m[b] + m[4 + a] * m[4 + b] + m[8 + a] * m[8 + b];
                const float want = a == b ? 1.0f : 0.0f;
                if (!(d > want - 0.001f && d < want + 0.001f))
                    return "a shape under a transform that scales or shears cannot carry an area light (Shape::area is the object-space area)";
            }
    }
    return nullptr;
}
// Shape::area in object space: Sphere (sphere.rs:99-101), Disk (disk.rs:129-131), Cylinder after pbrt-v3 (D80)
static float shape_area(const PbrtShape& sh) {
    float z0, z1;
    shape_z_range(sh, &z0, &z1);
    const float phi_max = shape_phi_max(sh), r = sh.radius;
    if (sh.type == PBRT_SHAPE_SPHERE) return phi_max * r * (z1 - z0);
    if (sh.type == PBRT_SHAPE_DISK) return phi_max * 0.5f * (r * r - sh.inner_radius * sh.inner_radius);
    return (z1 - z0) * r * phi_max;
}
static pb::DevShape shape_row(const PbrtShape& sh) {
    pb::DevShape d;
    std::memcpy(d.w2o, sh.to_object, 48);
    std::memcpy(d.o2w, sh.to_world, 48);
    d.radius = sh.radius;
    shape_z_range(sh, &d.z_min, &d.z_max);
    d.z_clip_min = (sh.type == PBRT_SHAPE_SPHERE && !(d.z_min > -sh.radius)) ? -INFINITY : d.z_min;
    d.z_clip_max = (sh.type == PBRT_SHAPE_SPHERE && !(d.z_max < sh.radius)) ? INFINITY : d.z_max;
    d.theta_min = d.theta_max = 0.0f;  // k_shape_angles
    d.phi_max = shape_phi_max(sh);
    d.inner_radius = sh.type == PBRT_SHAPE_DISK ? sh.inner_radius : 0.0f;
    // Transform::swaps_handedness (transform.rs): the upper 3x3's determinant is negative
    const float* m = sh.to_world;
    const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    const bool reverse = sh.reverse_orientation != 0;
    d.flags = sh.type | ((reverse != (det < 0.0f)) ? pb::kShapeFlipNormal : 0);
    return d;
}
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

static int scene_create_impl(PbrtHipContext* ctx, const float* positions, int32_t n_verts, const int32_t* indices,
                             int32_t n_tris, const int32_t* tri_material, const PbrtMaterial* materials,
                             int32_t n_materials, const int32_t* tri_light, const PbrtLight* lights, int32_t n_lights,
                             const PbrtLinearBVHNode* nodes, int32_t n_nodes, const int32_t* prim_order,
                             const InstancingArgs& ia, PbrtHipScene** out, pb::DeviceTree* dt, const SphereArgs& sa) {
    // dt != nullptr: the tree, the triangle records and the leaf order are already on the device
    // (pbrt_hip_scene_create_hlbvh); nodes / prim_order are then unused.
    if (!ctx || !out) return PBRT_HIP_ERR_INVALID;
    PB_ENTER(ctx);
    *out = nullptr;
    if (dt) n_nodes = dt->n_nodes;
    auto fail = [&](const char* msg) {
        ctx->last_error = msg;
        return PBRT_HIP_ERR_INVALID;
    };
    if (n_tris <= 0 || n_verts <= 0 || n_nodes <= 0) return fail("empty scene: n_tris, n_verts and n_nodes must be > 0");
    if (!positions || !indices || (!dt && ((!nodes && ia.n_instances == 0) || !prim_order))) return fail("null geometry / BVH pointer");
    if (n_materials <= 0 || !materials) return fail("at least one material is required");
    if (n_lights < 0 || (n_lights > 0 && !lights)) return fail("bad light table");
    for (int64_t i = 0; i < 3 * (int64_t)n_tris; ++i)
        if (indices[i] < 0 || indices[i] >= n_verts) return fail("vertex index out of range");
    const int32_t n_prims = n_tris + sa.n + sa.n_shapes;
    if (sa.n < 0 || (sa.n > 0 && (!sa.spheres || dt || ia.n_instances > 0))) return fail("bad sphere arguments");
    for (int32_t i = 0; i < sa.n; ++i) {
        if (!(sa.spheres[4 * i + 3] > 0.0f)) return fail("sphere radius must be positive");
        if (sa.material && (sa.material[i] < 0 || sa.material[i] >= n_materials)) return fail("sphere material out of range");
        if (sa.light && (sa.light[i] < -1 || sa.light[i] >= n_lights)) return fail("sphere light out of range");
    }
    if (sa.n_shapes < 0 || (sa.n_shapes > 0 && (!sa.shapes || sa.n > 0 || dt || ia.n_instances > 0))) return fail("bad shape arguments");
    for (int32_t i = 0; i < sa.n_shapes; ++i) {
        if (const char* why = shape_invalid(sa.shapes[i], n_materials, n_lights)) return fail(why);
    }
    for (int32_t i = 0; i < n_prims && !dt; ++i)
        if (prim_order[i] < 0 || prim_order[i] >= n_prims) return fail("prim_order entry out of range");
    for (int32_t i = 0; i < n_tris; ++i) {
        if (tri_material && (tri_material[i] < 0 || tri_material[i] >= n_materials)) return fail("tri_material out of range");
        if (tri_light && (tri_light[i] < -1 || tri_light[i] >= n_lights)) return fail("tri_light out of range");
    }
    for (int32_t i = 0; i < n_materials; ++i) {
        if (const char* why = material_invalid(materials[i])) return fail(why);
    }
    for (int32_t i = 0; i < n_lights; ++i) {
        if (lights[i].type < PBRT_LIGHT_DIFFUSE_AREA || lights[i].type > PBRT_LIGHT_GONIOMETRIC) return fail("unknown light type");
        if (lights[i].type == PBRT_LIGHT_PROJECTION || lights[i].type == PBRT_LIGHT_GONIOMETRIC) {
            const PbrtLight& l = lights[i];
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(l.pos[k]) || !std::isfinite(l.L[k])) return fail("projection / goniometric light: pos and L must be finite");
            for (int k = 0; k < 9; ++k)
                if (!std::isfinite(l.world_to_light[k])) return fail("projection / goniometric light: world_to_light must be finite");
            if (l.type == PBRT_LIGHT_PROJECTION && !(std::isfinite(l.fov) && l.fov > 0.0f && l.fov < 180.0f))
                return fail("projection light: fov must be finite and in (0, 180)");
        }
        if (lights[i].type == PBRT_LIGHT_DIFFUSE_AREA &&
            (lights[i].prim < 0 || lights[i].prim >= (ia.n_instances > 0 ? ia.n_world_tris : n_prims)))
            return fail("area light primitive out of range");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // ---- validate the tree(s) and lay out the interior records ----
    // single level: one tree over the triangles. Two levels (instancing): top-level tree over the
    // instances first, then the object-level tree over the triangles, in one record array.
    const bool instanced = ia.n_instances > 0;
    const int32_t n_top = ia.n_instances + ia.n_world_tris;  // primitives of the top-level aggregate
    TreeLayout top, obj;
    std::vector<TreeLayout> obj_trees;
    std::vector<DevMotion> motion_rows;  // moving instances: one row per INSTANCE here, per top-level slot on the device
    if (instanced) {
        for (int32_t i = 0; i < n_top; ++i)
            if (ia.tlas_order[i] < 0 || ia.tlas_order[i] >= n_top) return fail("tlas_order entry out of range");
        for (int32_t i = 0; i < ia.n_instances; ++i) {
            const float* m = ia.instances[i].to_world;
            const float* mi = ia.instances[i].to_object;
            if (m[12] != 0.0f || m[13] != 0.0f || m[14] != 0.0f || m[15] != 1.0f || mi[12] != 0.0f || mi[13] != 0.0f ||
                mi[14] != 0.0f || mi[15] != 1.0f)
                return fail("instance transforms must be affine (last row 0 0 0 1)");
            if (ia.instances[i].material >= n_materials) return fail("instance material out of range");
        }
        if (const char* e = convert_tree(ia.tlas_nodes, ia.n_tlas_nodes, n_top, 0, &top)) return fail(e);
        if (ia.motions) {
            // moving instances (host_motion.cpp); the limits of their one general shading build per integrator family: DESIGN.md D96
            for (int32_t i = 0; i < n_lights; ++i)
                if (lights[i].type == PBRT_LIGHT_PROJECTION || lights[i].type == PBRT_LIGHT_GONIOMETRIC)
                    return fail("scenes with moving instances take no projection or goniometric light");
            motion_rows.resize(ia.n_instances);
            for (int32_t i = 0; i < ia.n_instances; ++i)
                if (const char* why = motion_row(ia.instances[i], ia.motions[i], &motion_rows[i])) {
                    ctx->last_error = "moving instance " + std::to_string(i) + ": " + why;
                    return PBRT_HIP_ERR_INVALID;
                }
            // The caller built the top-level tree; one built over the static bounds would silently drop hits: every
            // instance's motion bound must lie inside the leaf box that holds it.
            for (int32_t nd = 0; nd < ia.n_tlas_nodes; ++nd) {
                const PbrtLinearBVHNode& leaf = ia.tlas_nodes[nd];
                for (int32_t k = 0; k < (int32_t)leaf.n_primitives; ++k) {
                    const int32_t slot = leaf.offset + k;
                    if (slot < 0 || slot >= n_top) return fail("top-level leaf slot out of range");
                    const int32_t id = ia.tlas_order[slot];
                    if (id >= ia.n_instances) continue;
                    const PbrtLinearBVHNode& root = ia.objects[ia.instance_object ? ia.instance_object[id] : 0].nodes[0];
                    float lo[3], hi[3];
                    if (pbrt_hip_instance_motion_bounds(root.bounds_min, root.bounds_max, ia.instances + id, ia.motions + id, 1, lo, hi) != PBRT_HIP_OK)
                        return fail("moving instance: no motion bound");
                    for (int c = 0; c < 3; ++c)
                        if (!(lo[c] >= leaf.bounds_min[c] && hi[c] <= leaf.bounds_max[c])) {
                            ctx->last_error = "instance " + std::to_string(id) + ": its motion bound (pbrt_hip_instance_motion_bounds) leaves the top-level "
                                              "leaf box that holds it; build the top-level tree over the motion bounds";
                            return PBRT_HIP_ERR_INVALID;
                        }
                }
            }
        }
        // the object-level trees behind it in one record array; one leaf-reference width for all of them
        int max_count = 1;
        for (int32_t k = 0; k < ia.n_objects; ++k)
            for (int32_t i = 0; i < ia.objects[k].n_nodes; ++i) max_count = std::max<int>(max_count, ia.objects[k].nodes[i].n_primitives);
        int bits = 0;
        while ((1 << bits) < max_count) ++bits;
        int base = top.n_interior, deepest = 0;
        obj_trees.resize(ia.n_objects);
        for (int32_t k = 0; k < ia.n_objects; ++k) {
            const PbrtObject& o = ia.objects[k];
            if (const char* e = convert_tree(o.nodes, o.n_nodes, o.n_tris, base, &obj_trees[k], ia.obj_tri_offset[k], bits, n_tris)) return fail(e);
            base += obj_trees[k].n_interior;
            deepest = std::max(deepest, obj_trees[k].depth);
            obj.inodes.insert(obj.inodes.end(), obj_trees[k].inodes.begin(), obj_trees[k].inodes.end());
        }
        obj.n_interior = base - top.n_interior;
        obj.count_bits = bits;
        obj.depth = deepest;
    } else if (dt) {
        top.n_interior = dt->n_interior;
        top.root_ref = dt->root_ref;
        top.count_bits = dt->count_bits;
    } else {
        if (const char* e = convert_tree(nodes, n_nodes, n_prims, 0, &top)) return fail(e);
    }
    const int n_interior = top.n_interior + obj.n_interior;
    if (top.depth + obj.depth > 64) return fail("BVH deeper than the 64-entry traversal stack (bvh.rs:839)");

    PbrtHipScene* s = new PbrtHipScene();
    s->ctx = ctx;
    s->n_tris = n_tris;
    s->n_nodes = n_nodes;
    s->n_interior = n_interior;
    bool ok = true;

    // ---- interior records: both children's boxes + references + axis (64 B) ----
    std::vector<float> inodes(top.inodes);
    inodes.insert(inodes.end(), obj.inodes.begin(), obj.inodes.end());
    if (inodes.empty()) inodes.assign(16, 0.0f);
    // ---- triangles in leaf order (48 B) ----
    std::vector<float> tris(dt ? 0 : (size_t)n_prims * 12);
    std::vector<int32_t> prim_slot(dt ? 0 : n_prims, -1);
    for (int32_t slot = 0; slot < n_prims && !dt; ++slot) {
        int32_t prim = prim_order[slot];
        if (prim_slot[prim] != -1) {
            delete s;
            return fail("prim_order is not a permutation");
        }
        prim_slot[prim] = slot;
        if (prim >= n_tris && sa.n_shapes > 0) {  // shape record: - | - | (row of DevBVH::shapes, prim, material, kPrimSphere)
            const PbrtShape& sh = sa.shapes[prim - n_tris];
            float* t = &tris[(size_t)slot * 12];
            for (int k = 0; k < 8; ++k) t[k] = 0.0f;
            int32_t meta[4] = {prim - n_tris, prim, sh.material, (sh.light + 1) | kPrimSphere};
            std::memcpy(t + 8, meta, 16);
            continue;
        }
        if (prim >= n_tris) {  // sphere record: (centre.xyz, radius) | - | (-, prim, material, kPrimSphere)
            const float* sp = sa.spheres + 4 * (size_t)(prim - n_tris);
            float* t = &tris[(size_t)slot * 12];
            t[0] = sp[0]; t[1] = sp[1]; t[2] = sp[2]; t[3] = sp[3];
            for (int k = 4; k < 9; ++k) t[k] = 0.0f;
            int32_t meta[3] = {prim, sa.material ? sa.material[prim - n_tris] : 0,
                               (sa.light ? sa.light[prim - n_tris] + 1 : 0) | kPrimSphere};
            std::memcpy(t + 9, meta, 12);
            continue;
        }
        const float* a = positions + 3 * (size_t)indices[3 * (size_t)prim];
        const float* b = positions + 3 * (size_t)indices[3 * (size_t)prim + 1];
        const float* c = positions + 3 * (size_t)indices[3 * (size_t)prim + 2];
        float* t = &tris[(size_t)slot * 12];
        t[0] = a[0]; t[1] = a[1]; t[2] = a[2];
        t[3] = b[0]; t[4] = b[1]; t[5] = b[2];
        t[6] = c[0]; t[7] = c[1]; t[8] = c[2];
        int32_t meta[3];
        meta[0] = prim;
        meta[1] = tri_material ? tri_material[prim] : 0;
        meta[2] = (tri_light ? tri_light[prim] + 1 : 0) | (triangle_rejected_by_intersect(a, b, c) ? kTriDegenerate : 0);
        std::memcpy(t + 9, meta, 12);
    }
    // ---- lights / materials ----
    std::vector<DevLight> dl(std::max(1, n_lights));
    std::vector<int> infinite_ids;
    float world_center[3], world_radius;
    {
        // Bounds3::bounding_sphere of the root bounds (infinite.rs:135-139)
        const float* mn = dt ? dt->root_min : (ia.n_instances > 0 ? ia.tlas_nodes[0] : nodes[0]).bounds_min;
        const float* mx = dt ? dt->root_max : (ia.n_instances > 0 ? ia.tlas_nodes[0] : nodes[0]).bounds_max;
        float dx[3];
        for (int k = 0; k < 3; ++k) {
            world_center[k] = (mn[k] + mx[k]) / 2.0f;
            dx[k] = world_center[k] - mx[k];
        }
        bool inside = true;
        for (int k = 0; k < 3; ++k) inside = inside && world_center[k] >= mn[k] && world_center[k] <= mx[k];
        world_radius = inside ? std::sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]) : 0.0f;
    }
    std::vector<float> power_y(n_lights);
    for (int32_t i = 0; i < n_lights; ++i) {
        DevLight& l = dl[i];
        l.type = lights[i].type;
        std::memcpy(l.L, lights[i].L, 12);
        l.two_sided = lights[i].two_sided;
        l.slot = -1;
        l.area = 0.0f;
        float scale;
        std::memcpy(l.pos, lights[i].pos, 12);
        l.cos_total_width = lights[i].cos_total_width;
        l.cos_falloff_start = lights[i].cos_falloff_start;
        std::memcpy(l.w2l, lights[i].world_to_light, 36);
        const bool map_light = l.type == PBRT_LIGHT_PROJECTION || l.type == PBRT_LIGHT_GONIOMETRIC;
        l.delta = (l.type == PBRT_LIGHT_POINT || l.type == PBRT_LIGHT_SPOT || l.type == PBRT_LIGHT_DISTANT || map_light) ? 1 : 0;
        if (l.type == PBRT_LIGHT_DIFFUSE_AREA) {
            int32_t prim = lights[i].prim + (instanced ? ia.world_tri_offset : 0);  // two-level: prim counts the world-space triangles
            l.slot = dt ? dt->light_slot[i] : prim_slot[prim];
            if (prim >= n_tris && sa.n_shapes > 0) {
                l.area = shape_area(sa.shapes[prim - n_tris]);
            } else if (prim >= n_tris) {
                float r = sa.spheres[4 * (size_t)(prim - n_tris) + 3];
                l.area = (360.0f * (kPi / 180.0f)) * r * (r - (-r));  // Sphere::area (sphere.rs:99-101)
            } else {
                const float* a = positions + 3 * (size_t)indices[3 * (size_t)prim];
                const float* b = positions + 3 * (size_t)indices[3 * (size_t)prim + 1];
                const float* c = positions + 3 * (size_t)indices[3 * (size_t)prim + 2];
                l.area = tri_area(a, b, c);
            }
            scale = (l.two_sided ? 2.0f : 1.0f) * l.area * kPi;  // diffuse.rs:83-85
        } else if (l.type == PBRT_LIGHT_POINT) {
            scale = 4.0f * kPi;  // point.rs:65-67
        } else if (l.type == PBRT_LIGHT_SPOT) {
            scale = 2.0f * kPi * (1.0f - 0.5f * (l.cos_falloff_start + l.cos_total_width));  // spot.rs:90-92
        } else if (l.type == PBRT_LIGHT_DISTANT) {
            scale = kPi * world_radius * world_radius;  // distant.rs:76-78
        } else if (map_light) {
            // without a map (pbrt_hip_scene_set_light_map attaches one): goniometric.rs:105-113 = the point light's 4 pi I;
            // projection: pbrt-v3's I 2 pi (1 - cos_total_width) (D89). slot names the light's DevLightMap.
            l.slot = i;
            s->light_maps = true;
            if (s->h_light_maps.empty()) {
                s->h_light_maps.assign(n_lights, DevLightMap{});
                s->light_fov.assign(n_lights, 0.0f);
            }
            s->light_fov[i] = lights[i].fov;
            DevLightMap& m = s->h_light_maps[i];
            const double cos_total_width = light_map_geometry(l.type, lights[i].fov, 0, 0, m.screen_bounds, &m.inv_tan);
            l.cos_total_width = (float)cos_total_width;
            scale = l.type == PBRT_LIGHT_GONIOMETRIC ? 4.0f * kPi : (float)(2.0 * 3.14159265358979323846 * (1.0 - cos_total_width));
        } else {
            infinite_ids.push_back(i);
            scale = kPi * world_radius * world_radius;  // infinite.rs:131-133
        }
        float p[3] = {l.L[0] * scale, l.L[1] * scale, l.L[2] * scale};
        l.power_y = 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2];  // spectrum.rs:679-682
        power_y[i] = l.power_y;
    }
    s->h_lights = dl;
    s->light_samples.resize(n_lights);
    for (int32_t i = 0; i < n_lights; ++i) s->light_samples[i] = (dl[i].type == PBRT_LIGHT_PROJECTION || dl[i].type == PBRT_LIGHT_GONIOMETRIC) ? 1 : std::max(1, lights[i].n_samples);
    std::vector<DevMaterial> dm(n_materials);
    for (int32_t i = 0; i < n_materials; ++i) {
        dm[i] = row_of_material(materials[i]);
        const bool glossy = materials[i].type == PBRT_MAT_PLASTIC || materials[i].type == PBRT_MAT_METAL;
        s->glossy = s->glossy || glossy;
    }
    s->h_materials = dm;

    DevSceneData& d = s->d;
    std::memset(&d, 0, sizeof(d));
    std::vector<float> top_slot_records;  // two-level scenes: the 112-B records of the top-level leaf slots
    if (dt) {
        d.bvh.inodes = dt->inodes;
        d.bvh.tris = dt->tris;
        d.slot_prim = dt->slot_prim;
        s->allocs.push_back(dt->inodes);
        s->allocs.push_back(dt->tris);
        s->allocs.push_back(dt->slot_prim);
        dt->inodes = dt->tris = nullptr;  // owned by the scene from here on
        dt->slot_prim = nullptr;
        std::memcpy(d.bvh.root_min, dt->root_min, 12);
        std::memcpy(d.bvh.root_max, dt->root_max, 12);
    } else {
        d.bvh.inodes = (const float4*)dev_upload(s, inodes.data(), inodes.size(), &ok);
        d.bvh.tris = (const float4*)dev_upload(s, tris.data(), tris.size(), &ok);
        const PbrtLinearBVHNode& root = instanced ? ia.tlas_nodes[0] : nodes[0];
        std::memcpy(d.bvh.root_min, root.bounds_min, 12);
        std::memcpy(d.bvh.root_max, root.bounds_max, 12);
    }
    d.bvh.root_ref = top.root_ref;
    d.bvh.count_bits = top.count_bits;
    d.bvh.n_slots = n_prims;
    d.bvh.has_spheres = sa.n_shapes > 0 ? 2 : (sa.n > 0 ? 1 : 0);
    if (sa.n_shapes > 0) {
        std::vector<DevShape> rows(sa.n_shapes);
        for (int32_t i = 0; i < sa.n_shapes; ++i) rows[i] = shape_row(sa.shapes[i]);
        DevShape* d_rows = dev_upload(s, rows.data(), rows.size(), &ok);
        if (ok) {  // theta_min / theta_max with the kernels' own acos
            hipLaunchKernelGGL(k_shape_angles, dim3((sa.n_shapes + 63) / 64), dim3(64), 0, ctx->stream, d_rows, sa.n_shapes);
            ok = hip_ok(ctx, hipGetLastError(), "k_shape_angles") && hip_ok(ctx, hipStreamSynchronize(ctx->stream), "k_shape_angles");
        }
        d.bvh.shapes = d_rows;
    }
    d.bvh.instanced = instanced ? 1 : 0;
    if (instanced) {
        d.bvh.blas_count_bits = obj.count_bits;
        d.bvh.general_top = (ia.n_objects > 1 || ia.n_world_tris > 0) ? 1 : 0;
        d.bvh.blas_root_ref = obj_trees[0].root_ref;
        std::memcpy(d.bvh.blas_root_min, ia.objects[0].nodes[0].bounds_min, 12);
        std::memcpy(d.bvh.blas_root_max, ia.objects[0].nodes[0].bounds_max, 12);
        // object table: (root box min, root reference) (root box max, -)
        std::vector<float> objs((size_t)ia.n_objects * 8, 0.0f);
        for (int32_t k = 0; k < ia.n_objects; ++k) {
            const PbrtLinearBVHNode& root = ia.objects[k].nodes[0];
            float* r = &objs[(size_t)k * 8];
            std::memcpy(r, root.bounds_min, 12);
            std::memcpy(r + 3, &obj_trees[k].root_ref, 4);
            std::memcpy(r + 4, root.bounds_max, 12);
        }
        d.bvh.objects = (const float4*)dev_upload(s, objs.data(), objs.size(), &ok);
        // records of the top-level leaf slots: to_object rows 0-2, to_world rows 0-2, (material, instance id, object, kind);
        // a world-space triangle beside the instances: kind 1, its leaf slot in the third field
        std::vector<float>& inst = top_slot_records;
        inst.assign((size_t)n_top * 28, 0.0f);
        std::vector<int32_t> slot_inst(n_top);
        std::vector<char> seen(n_top, 0);
        for (int32_t slot = 0; slot < n_top; ++slot) {
            int32_t id = ia.tlas_order[slot];
            if (seen[id]) ok = false;
            seen[id] = 1;
            float* r = &inst[(size_t)slot * 28];
            if (id < ia.n_instances) {
                slot_inst[slot] = id;
                std::memcpy(r, ia.instances[id].to_object, 48);
                std::memcpy(r + 12, ia.instances[id].to_world, 48);
                int32_t meta[4] = {ia.instances[id].material, id, ia.instance_object ? ia.instance_object[id] : 0, 0};
                std::memcpy(r + 24, meta, 16);
            } else {
                slot_inst[slot] = -1;
                int32_t meta[4] = {-1, -1, prim_slot[ia.world_tri_offset + (id - ia.n_instances)], 1};
                std::memcpy(r + 24, meta, 16);
            }
        }
        if (!ok) ctx->last_error = "tlas_order is not a permutation";
        d.bvh.instances = (const float4*)dev_upload(s, inst.data(), inst.size(), &ok);
        d.slot_instance = dev_upload(s, slot_inst.data(), slot_inst.size(), &ok);
        s->n_instances = ia.n_instances;
        if (!motion_rows.empty()) {
            std::vector<DevMotion> by_slot(n_top, DevMotion{});
            for (int32_t slot = 0; slot < n_top; ++slot)
                if (slot_inst[slot] >= 0) by_slot[slot] = motion_rows[slot_inst[slot]];
            s->d_motions = dev_upload(s, by_slot.data(), by_slot.size(), &ok);
            s->moving = true;
        }
    }
    // ---- 4-wide quantised records over the same tree (wide_bvh.h): single-level triangle scenes whose tree came
    // from the host; PBRT_WIDE_BUILD_NONE keeps the scene on the binary records ----
    int spill_entries = kStackSpill;
    {
        if (ctx->wide_build == PBRT_WIDE_BUILD_NONE) {
            s->wide_reason = "disabled by PBRT_WIDE_BUILD_NONE";
        } else if (sa.n_shapes > 0) {
            s->wide_reason = "scene with shapes";
        } else if (sa.n > 0) {
            s->wide_reason = "scene with spheres";
        } else if (s->moving) {
            s->wide_reason = "scene with moving instances";
        } else if (dt && dt->wide.n_records >= 0) {
            // laid out on the device beside the tree (wide_gpu.hip): the scene takes the arrays over
            s->wide.nodes = (const uint4*)dt->wide.nodes;
            s->wide.tris = (const float4*)dt->wide.tris;
            s->wide.leaf_boxes = (const float4*)dt->wide.leaf_boxes;
            s->allocs.push_back(dt->wide.nodes);
            s->allocs.push_back(dt->wide.tris);
            s->allocs.push_back(dt->wide.leaf_boxes);
            dt->wide.nodes = nullptr;
            dt->wide.tris = dt->wide.leaf_boxes = nullptr;
            s->wide.root_ref = dt->wide.root_ref;
            s->n_wide_records = dt->wide.n_records;
            s->has_wide = true;
            s->wide_stack_need = dt->wide.stack_need;
            spill_entries = std::max(spill_entries, dt->wide.stack_need + 1 - kWideStackLds);
        } else if (dt && dt->h_nodes.empty()) {
            s->wide_reason = dt->wide_reason ? dt->wide_reason : "tree built on the device: no wide records";
        } else if (instanced) {
            // two levels: the top-level tree's records first (its leaves keep their exact boxes and name top-level
            // primitives in wide order), then every object aggregate's; one triangle / leaf-box array for all objects
            pb::WideTree top;
            const char* why = pb::build_wide_tree(ia.tlas_nodes, ia.n_tlas_nodes, nullptr, n_top, &top);
            std::vector<pb::WideTree> wobj(ia.n_objects);
            int record_base = why ? 0 : top.n_records, deepest = 0;
            for (int32_t k = 0; k < ia.n_objects && !why; ++k) {
                pb::WideBase b;
                b.record = record_base;
                b.tri = b.slot = ia.obj_tri_offset[k];
                why = pb::build_wide_tree(ia.objects[k].nodes, ia.objects[k].n_nodes, tris.data() + 12 * (size_t)ia.obj_tri_offset[k],
                                          ia.objects[k].n_tris, &wobj[k], b);
                if (!why) {
                    record_base += wobj[k].n_records;
                    deepest = std::max(deepest, wobj[k].stack_need);
                }
            }
            if (why) {
                s->wide_reason = why;
            } else {
                std::vector<uint32_t> wn;
                wn.insert(wn.end(), top.nodes.begin(), top.nodes.begin() + (size_t)top.n_records * kWideNodeDwords);
                std::vector<float> wt((size_t)n_prims * 12, 0.0f), wb((size_t)n_prims * 8, 0.0f), wo((size_t)ia.n_objects * 8, 0.0f);
                for (int32_t k = 0; k < ia.n_objects; ++k) {
                    wn.insert(wn.end(), wobj[k].nodes.begin(), wobj[k].nodes.begin() + (size_t)wobj[k].n_records * kWideNodeDwords);
                    std::memcpy(&wt[12 * (size_t)ia.obj_tri_offset[k]], wobj[k].tris.data(), wobj[k].tris.size() * 4);
                    std::memcpy(&wb[8 * (size_t)ia.obj_tri_offset[k]], wobj[k].leaf_boxes.data(), wobj[k].leaf_boxes.size() * 4);
                    const PbrtLinearBVHNode& root = ia.objects[k].nodes[0];
                    float* r = &wo[(size_t)k * 8];
                    std::memcpy(r, root.bounds_min, 12);
                    std::memcpy(r + 3, &wobj[k].root_ref, 4);
                    std::memcpy(r + 4, root.bounds_max, 12);
                }
                if (wn.empty()) wn.assign(kWideNodeDwords, 0u);
                // the top-level entries as the wide kernel reads them, in wide order, 20 floats each: the exact box of the leaf
                // the entry belongs to with two words in the w fields — the binary-layout top slot (hit records name it) and
                // the object index (an instance) or 0x40000000 | leaf slot (a world-space triangle) — then the three
                // world-to-object rows
                std::vector<float> ws((size_t)n_top * 20);
                for (int32_t pos = 0; pos < n_top; ++pos) {
                    const int32_t slot = top.order[pos];
                    const float* src = &top_slot_records[(size_t)slot * 28];
                    float* dst = &ws[(size_t)pos * 20];
                    int32_t meta[4];
                    std::memcpy(meta, src + 24, 16);  // (material, id, object | leaf slot, kind)
                    const int32_t word = meta[3] == 1 ? (0x40000000 | meta[2]) : meta[2];
                    std::memcpy(dst, &top.leaf_boxes[(size_t)pos * 8], 12);
                    std::memcpy(dst + 3, &slot, 4);
                    std::memcpy(dst + 4, &top.leaf_boxes[(size_t)pos * 8 + 4], 12);
                    std::memcpy(dst + 7, &word, 4);
                    std::memcpy(dst + 8, src, 48);
                }
                s->wide.nodes = (const uint4*)dev_upload(s, wn.data(), wn.size(), &ok);
                s->wide.tris = (const float4*)dev_upload(s, wt.data(), wt.size(), &ok);
                s->wide.leaf_boxes = (const float4*)dev_upload(s, wb.data(), wb.size(), &ok);
                s->wide.top_slots = (const float4*)dev_upload(s, ws.data(), ws.size(), &ok);
                s->wide.top_boxes = (const float4*)dev_upload(s, top.leaf_boxes.data(), top.leaf_boxes.size(), &ok);
                s->wide.objects = (const float4*)dev_upload(s, wo.data(), wo.size(), &ok);
                s->wide.slot_tris = d.bvh.tris;
                s->wide.root_ref = top.root_ref;
                s->wide.general_top = d.bvh.general_top;
                s->wide.obj0_root = wobj[0].root_ref;
                std::memcpy(s->wide.obj0_min, ia.objects[0].nodes[0].bounds_min, 12);
                std::memcpy(s->wide.obj0_max, ia.objects[0].nodes[0].bounds_max, 12);
                s->n_wide_records = record_base;
                s->has_wide = true;
                spill_entries = std::max(spill_entries, top.stack_need + deepest + 2 - pb::wide_stack_lds(1));
            }
        } else if (!dt && ok && ctx->wide_build != PBRT_WIDE_BUILD_HOST) {
            // a tree from the host: its flat nodes go up once, the records are laid out on the device from them and from
            // the triangle records already there (wide_gpu.hip; the host builder produces the same bytes, tens of ms per
            // million triangles slower: PBRT_WIDE_BUILD_HOST)
            bool up = true;
            PbrtLinearBVHNode* d_flat = dev_upload(s, nodes, (size_t)n_nodes, &up);
            pb::WideDeviceTree wd;
            const char* why = nullptr;
            if (!up || !pb::build_wide_tree_device(ctx, d_flat, n_nodes, (const float*)d.bvh.tris, n_prims, nodes[0], &wd, &why)) {
                ok = false;
            } else if (why) {
                s->wide_reason = why;
            } else {
                s->wide.nodes = (const uint4*)wd.nodes;
                s->wide.tris = (const float4*)wd.tris;
                s->wide.leaf_boxes = (const float4*)wd.leaf_boxes;
                s->allocs.push_back(wd.nodes);
                s->allocs.push_back(wd.tris);
                s->allocs.push_back(wd.leaf_boxes);
                s->wide.root_ref = wd.root_ref;
                s->n_wide_records = wd.n_records;
                s->has_wide = true;
                s->wide_stack_need = wd.stack_need;
            spill_entries = std::max(spill_entries, wd.stack_need + 1 - kWideStackLds);
            }
            if (d_flat) {  // only the builder needed it
                (void)hipFree(d_flat);
                s->allocs.erase(std::remove(s->allocs.begin(), s->allocs.end(), (void*)d_flat), s->allocs.end());
            }
        } else {
            pb::WideTree wt;
            const char* why = dt ? pb::build_wide_tree(dt->h_nodes.data(), n_nodes, dt->h_tris.data(), n_prims, &wt)
                                 : pb::build_wide_tree(nodes, n_nodes, tris.data(), n_prims, &wt);
            if (why) {
                s->wide_reason = why;
            } else {
                s->wide.nodes = (const uint4*)dev_upload(s, wt.nodes.data(), wt.nodes.size(), &ok);
                s->wide.tris = (const float4*)dev_upload(s, wt.tris.data(), wt.tris.size(), &ok);
                s->wide.leaf_boxes = (const float4*)dev_upload(s, wt.leaf_boxes.data(), wt.leaf_boxes.size(), &ok);
                s->wide.root_ref = wt.root_ref;
                s->n_wide_records = wt.n_records;
                s->has_wide = true;
                s->wide_stack_need = wt.stack_need;
            spill_entries = std::max(spill_entries, wt.stack_need + 1 - kWideStackLds);
            }
        }
    }
    // one 64-byte line per record / wide-order triangle where the tree is too large for L2 (wide_bvh.h: kWideLineAlignBytes;
    // pbrt_hip_context_set_wide_layout overrides): the builders' packed arrays are spread on the device and released
    s->wide.vec_stride = 3;
    if (s->has_wide && ok) {
        const size_t packed_bytes = ((size_t)std::max(s->n_wide_records, 1) + (size_t)n_prims) * 48;
        // (two-level scenes stay packed: the trees of a scene of instances are small, and trace_wide<.., INST> keeps its compile-time stride)
        const bool lines = !instanced && (ctx->wide_layout == PBRT_WIDE_LAYOUT_LINES || (ctx->wide_layout == PBRT_WIDE_LAYOUT_AUTO && packed_bytes > pb::kWideLineAlignBytes));
        auto spread = [&](const void* packed, size_t count) -> void* {
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
        };
        if (lines) {
            void* n4 = spread(s->wide.nodes, (size_t)std::max(s->n_wide_records, 1));
            void* t4 = n4 ? spread(s->wide.tris, (size_t)n_prims) : nullptr;
            if (!n4 || !t4) {
                ok = false;
            } else {
                s->wide.nodes = (const uint4*)n4;
                s->wide.tris = (const float4*)t4;
                s->wide.vec_stride = 4;
            }
        }
    }
    // spill slab for the deepest stack entries of every resident lane of the traversal grid
    s->spill_lanes = ctx->n_cus * 2048;
    {
        void* p = nullptr;
        if (!hip_ok(ctx, hipMalloc(&p, (size_t)s->spill_lanes * spill_entries * sizeof(uint2)), "hipMalloc spill")) ok = false;
        else s->allocs.push_back(p);
        d.bvh.spill = (uint2*)p;
        d.bvh.spill_stride = s->spill_lanes;
        s->wide.spill = (uint2*)p;
        s->wide.spill_stride = s->spill_lanes;
    }
    if (!dt && !instanced) d.slot_prim = dev_upload(s, prim_order, n_prims, &ok);
    if (instanced) {  // hit records name a triangle by its index inside its own object (world triangles: their own list)
        std::vector<int32_t> local(n_prims);
        int32_t k = 0;
        for (int32_t slot = 0; slot < n_prims; ++slot) {
            while (k < ia.n_objects && slot >= ia.obj_tri_offset[k + 1]) ++k;
            local[slot] = prim_order[slot] - (k < ia.n_objects ? ia.obj_tri_offset[k] : ia.world_tri_offset);
        }
        d.slot_prim = dev_upload(s, local.data(), local.size(), &ok);
    }
    d.materials = dev_upload(s, dm.data(), dm.size(), &ok);
    {
        std::vector<DevDisney> dz(n_materials, DevDisney{});  // pbrt_hip_scene_set_disney_material fills a row's block
        d.disney = dev_upload(s, dz.data(), dz.size(), &ok);
        s->h_lobe_rows.assign(n_materials, DevLobeRow{});  // pbrt_hip_scene_set_lobe_material fills a row's list
        s->h_lobe_origin.assign(n_materials, 0);
        d.lobe_rows = dev_upload(s, s->h_lobe_rows.data(), s->h_lobe_rows.size(), &ok);
    }
    d.lights = dev_upload(s, dl.data(), dl.size(), &ok);
    if (s->light_maps) {
        d.light_maps = dev_upload(s, s->h_light_maps.data(), s->h_light_maps.size(), &ok);
        s->light_map_allocs.assign(n_lights, nullptr);
    }
    d.n_lights = n_lights;
    d.n_materials = n_materials;
    d.n_infinite = (int)infinite_ids.size();
    d.infinite_ids = dev_upload(s, infinite_ids.data(), infinite_ids.size(), &ok);
    std::memcpy(d.world_center, world_center, 12);
    d.world_radius = world_radius;
    // InfiniteAreaLight's Distribution2D over a 2x2 sin-weighted image of the constant map
    // (infinite.rs:59-73); all infinite lights here are constant so one table per light would be
    // identical up to the luminance scale -- built for the first infinite light, rescaled per use.
    {
        for (int v = 0; v < 2; ++v) {
            float vp = ((float)v + 0.5f) / 2.0f;
            float sin_theta = host_det_sin(kPi * vp);
            std::vector<float> row(2);
            for (int u = 0; u < 2; ++u) {
                float y = 1.0f;
                if (!infinite_ids.empty()) {
                    const float* L = dl[infinite_ids[0]].L;
                    y = 0.212671f * L[0] + 0.715160f * L[1] + 0.072169f * L[2];
                }
                row[u] = y;
                row[u] *= sin_theta;
            }
            std::vector<float> cdf;
            float fi;
            make_distribution(row, &cdf, &fi);
            for (int u = 0; u < 2; ++u) d.env_cond_func[v][u] = row[u];
            for (int u = 0; u < 3; ++u) d.env_cond_cdf[v][u] = cdf[u];
            d.env_cond_int[v] = fi;
        }
        std::vector<float> mf = {d.env_cond_int[0], d.env_cond_int[1]}, cdf;
        float fi;
        make_distribution(mf, &cdf, &fi);
        for (int u = 0; u < 2; ++u) d.env_marg_func[u] = mf[u];
        for (int u = 0; u < 3; ++u) d.env_marg_cdf[u] = cdf[u];
        d.env_marg_int = fi;
    }
    // light sampling distributions (lightdistrib.rs:21-69, integrator.rs:268-277)
    if (n_lights > 0) {
        std::vector<float> uni(n_lights, 1.0f), cdf;
        float fi;
        make_distribution(uni, &cdf, &fi);
        d.light_distrib_uniform.func = dev_upload(s, uni.data(), uni.size(), &ok);
        d.light_distrib_uniform.cdf = dev_upload(s, cdf.data(), cdf.size(), &ok);
        d.light_distrib_uniform.func_int = fi;
        d.light_distrib_uniform.n = n_lights;
        make_distribution(power_y, &cdf, &fi);
        d.light_distrib_power.func = dev_upload(s, power_y.data(), power_y.size(), &ok);
        d.light_distrib_power.cdf = dev_upload(s, cdf.data(), cdf.size(), &ok);
        d.light_distrib_power.func_int = fi;
        d.light_distrib_power.n = n_lights;
    }
    if (!ok) {
        pbrt_hip_scene_destroy(s);
        return PBRT_HIP_ERR_DEVICE;
    }
    *out = s;
    return PBRT_HIP_OK;
}

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
        for (auto& a : s->env_allocs)
            for (void* p : a) (void)hipFree(p);
        for (void* p : s->light_map_allocs)
            if (p) (void)hipFree(p);
    }
    delete s;
}

// TrowbridgeReitzDistribution::new(alpha_u, alpha_v, true) of a plastic / metal material with pbrt-v3's remaproughness switch
// (plastic.cpp / metal.cpp): the alphas of material `material` are replaced in the device table and its host copy.
extern "C" int pbrt_hip_scene_set_material_roughness(PbrtHipScene* s, int32_t material, float u_roughness, float v_roughness,
                                                     int32_t remap) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_material_roughness: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevMaterial m = s->h_materials[material];
    if (m.type != PBRT_MAT_PLASTIC && m.type != PBRT_MAT_METAL) return invalid("material is not PBRT_MAT_PLASTIC or PBRT_MAT_METAL");
    if (const char* why = roughness_invalid(u_roughness, v_roughness, remap != 0)) return invalid(why);
    if (m.type == PBRT_MAT_PLASTIC && u_roughness != v_roughness) return invalid("plastic is isotropic: u_roughness must equal v_roughness");
    m.alpha_u = remap ? roughness_to_alpha(u_roughness) : u_roughness;
    m.alpha_v = remap ? roughness_to_alpha(v_roughness) : v_roughness;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.materials + material), &m, sizeof(DevMaterial), hipMemcpyHostToDevice));
    s->h_materials[material] = m;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// which shading-kernel level the table needs beyond plastic / metal, after a row was replaced
static void refresh_material_levels(PbrtHipScene* s) {
    s->bxdfs = s->disney = s->lobes = false;
    for (const DevMaterial& row : s->h_materials) {
        s->lobes = s->lobes || row.type == kMatLobes;
        s->bxdfs = s->bxdfs || (row.type >= kMatOrenNayar && row.type <= kMatSubstrate);
        s->disney = s->disney || row.type == kMatDisney;
    }
}

// pbrt-v3's MatteMaterial (sigma), GlassMaterial (roughness) and SubstrateMaterial on the reference's OrenNayar,
// MicrofacetReflection / MicrofacetTransmission and FresnelBlend (reflection.rs:917-975, 977-1192, 1194-1280): row `material`
// of the device table and of its host copy is replaced by what the descriptor reduces to. A descriptor an existing
// PbrtMaterialType expresses becomes that row; the others become a kMatOrenNayar / kMatRoughGlass / kMatSubstrate row
// (scene.h), which the shading kernels' level-2 instantiations shade (wf_bxdfs.h).
extern "C" int pbrt_hip_scene_set_material(PbrtHipScene* s, int32_t material, const PbrtMaterialDesc* desc) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_material: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    DevMaterial m{};
    if (const char* why = row_of_desc(*desc, &m)) return invalid(why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.materials + material), &m, sizeof(DevMaterial), hipMemcpyHostToDevice));
    s->h_materials[material] = m;
    s->h_lobe_origin[material] = 0;
    refresh_material_levels(s);
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// pbrt-v3's DisneyMaterial without subsurface (include/pbrt_hip.h): row `material` becomes a kMatDisney row
// and its DevDisney block (scene.h) gets the lobes' constants, computed here in double and rounded once. The shading kernels'
// level-3 instantiations shade it (wf_disney.h).
extern "C" int pbrt_hip_scene_set_disney_material(PbrtHipScene* s, int32_t material, const PbrtDisneyDesc* desc) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_disney_material: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    const PbrtDisneyDesc& p = *desc;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p.color[k]) || p.color[k] < 0.0f) return invalid("color must be finite and >= 0");
    const struct {
        const char* name;
        float v, max;
    } scalars[] = {{"metallic", p.metallic, 1.0f}, {"eta", p.eta, INFINITY}, {"roughness", p.roughness, 1.0f},
                   {"specular_tint", p.specular_tint, 1.0f}, {"anisotropic", p.anisotropic, 1.0f}, {"sheen", p.sheen, INFINITY},
                   {"sheen_tint", p.sheen_tint, 1.0f}, {"clearcoat", p.clearcoat, INFINITY}, {"clearcoat_gloss", p.clearcoat_gloss, 1.0f},
                   {"spec_trans", p.spec_trans, 1.0f}, {"flatness", p.flatness, 1.0f}, {"diff_trans", p.diff_trans, 2.0f}};
    for (const auto& sv : scalars) {
        if (!std::isfinite(sv.v) || sv.v < 0.0f) return invalid(std::string(sv.name) + " must be finite and >= 0");
        if (sv.v > sv.max) return invalid(std::string(sv.name) + (sv.max == 2.0f ? " must be <= 2" : " must be <= 1"));
    }
    if (!(p.eta > 0.0f)) return invalid("eta must be > 0");

    const bool thin = p.thin != 0;
    const double c[3] = {p.color[0], p.color[1], p.color[2]};
    const double lum = 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2];
    const double metallic = p.metallic, eta = p.eta, rough = p.roughness, strans = p.spec_trans, flat = p.flatness;
    const double dw = (1.0 - metallic) * (1.0 - strans), dt = p.diff_trans / 2.0;
    const double aspect = std::sqrt(1.0 - 0.9 * p.anisotropic);
    const double r0 = ((eta - 1.0) / (eta + 1.0)) * ((eta - 1.0) / (eta + 1.0));
    auto lerp = [](double t, double a, double b) { return (1.0 - t) * a + t * b; };
    DevDisney z{};
    z.metallic = p.metallic;
    z.eta = p.eta;
    z.roughness = p.roughness;
    z.ax = (float)std::max(1e-3, rough * rough / aspect);
    z.ay = (float)std::max(1e-3, rough * rough * aspect);
    z.tax = z.ax;
    z.tay = z.ay;
    z.sep_trans = thin ? 0 : 1;
    z.lobes = kDzMicro;
    if (dw > 0.0) z.lobes |= kDzDiffuse | kDzRetro | (thin ? kDzFakeSS : 0) | (p.sheen > 0.0f ? kDzSheen : 0);
    if (p.clearcoat > 0.0f) z.lobes |= kDzClearcoat;
    if (p.spec_trans > 0.0f) z.lobes |= kDzTrans;
    if (thin) z.lobes |= kDzLambertT;
    for (int k = 0; k < 3; ++k) {
        const double tint = lum > 0.0 ? c[k] / lum : 1.0;
        z.cspec0[k] = (float)lerp(metallic, r0 * lerp(p.specular_tint, 1.0, tint), c[k]);
        if (z.lobes & kDzDiffuse) z.diffuse[k] = (float)(thin ? dw * (1.0 - flat) * (1.0 - dt) * c[k] : dw * c[k]);
        if (z.lobes & kDzFakeSS) z.fakess[k] = (float)(dw * flat * (1.0 - dt) * c[k]);
        if (z.lobes & kDzRetro) z.retro[k] = (float)(dw * c[k]);
        if (z.lobes & kDzSheen) z.sheen[k] = (float)(dw * p.sheen * lerp(p.sheen_tint, 1.0, tint));
        if (z.lobes & kDzTrans) z.trans[k] = (float)(strans * std::sqrt(c[k]));
        if (z.lobes & kDzLambertT) z.lambert_t[k] = (float)(dt * c[k]);
    }
    {
        const double g = lerp(p.clearcoat_gloss, 0.1, 0.001), a2 = g * g;
        z.clearcoat = p.clearcoat;
        z.cc_a2 = (float)a2;
        z.cc_ln_a2 = (float)std::log(a2);
        z.cc_norm = (float)((a2 - 1.0) / (3.14159265358979323846 * std::log(a2)));
    }
    if ((z.lobes & kDzTrans) && thin) {
        const double rs = (0.65 * eta - 0.35) * rough;
        z.tax = (float)std::max(1e-3, rs * rs / aspect);
        z.tay = (float)std::max(1e-3, rs * rs * aspect);
    }
    z.n = __builtin_popcount((unsigned)z.lobes);
    DevMaterial m{};
    m.type = kMatDisney;
    std::memcpy(m.kd, p.color, 12);
    m.eta = p.eta;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.disney + material), &z, sizeof(DevDisney), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.materials + material), &m, sizeof(DevMaterial), hipMemcpyHostToDevice));
    s->h_materials[material] = m;
    s->h_lobe_origin[material] = 0;
    refresh_material_levels(s);
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// pbrt-v3's UberMaterial, TranslucentMaterial and MixMaterial (include/pbrt_hip.h): row `material` becomes a
// kMatLobes row and its DevLobeRow (scene.h) gets the list host_lobes.cpp makes of the descriptor. The shading kernels' lobe-list
// builds shade it (wf_lobes.h). A mix copies its operands' lists as they are now.
extern "C" int pbrt_hip_scene_set_lobe_material(PbrtHipScene* s, int32_t material, const PbrtLobeMaterialDesc* desc) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_lobe_material: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (!desc) return invalid("null desc");
    if (material < 0 || material >= (int32_t)s->h_materials.size()) return invalid("material index out of range");
    if (s->d.bvh.has_spheres == 2) return invalid("scenes with general quadric shapes take no lobe rows (their shading builds stay at level 3)");
    if (s->light_maps) return invalid("scenes with a projection or goniometric light take no lobe rows (their shading builds stay at level 3)");
    if (s->moving) return invalid("scenes with moving instances take no lobe rows");
    LobeList la, lb, L;
    if (desc->type == PBRT_LOBEMAT_MIX) {
        const int32_t ops[2] = {desc->material_a, desc->material_b};
        LobeList* lists[2] = {&la, &lb};
        for (int k = 0; k < 2; ++k) {
            const std::string name = k ? "material_b" : "material_a";
            if (ops[k] < 0 || ops[k] >= (int32_t)s->h_materials.size()) return invalid(name + " out of range");
            const DevMaterial& om = s->h_materials[ops[k]];
            if (om.type == kMatLobes) {
                if (s->h_lobe_origin[ops[k]] == PBRT_LOBEMAT_MIX) return invalid(name + " is a mix row");
                const DevLobeRow& r = s->h_lobe_rows[ops[k]];
                lists[k]->n = r.n;
                lists[k]->eta = r.eta;
                for (int i = 0; i < r.n; ++i) lists[k]->lobes[i] = r.lobes[i];
            } else if (const char* why = lobes_of_row(om, lists[k])) {
                return invalid(name + ": " + why);
            }
        }
    }
    if (const char* why = lobes_of_lobe_desc(*desc, &la, &lb, &L)) return invalid(why);
    const DevLobeRow row = lobe_row_of(L);
    DevMaterial m{};
    m.type = kMatLobes;
    m.eta = L.eta;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.lobe_rows + material), &row, sizeof(DevLobeRow), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy((void*)(s->d.materials + material), &m, sizeof(DevMaterial), hipMemcpyHostToDevice));
    s->h_materials[material] = m;
    s->h_lobe_rows[material] = row;
    s->h_lobe_origin[material] = desc->type;
    refresh_material_levels(s);
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// InfiniteAreaLight::new(light_to_world, L, n_samples, texmap) (lights/infinite.rs:36-82) with the texels in memory: the map's
// tables (host_envmap.cpp) go to the device for light `light`, its power and the power distribution are recomputed, and a
// spatial light table already built is dropped (the next render with that strategy builds it again).
extern "C" int pbrt_hip_scene_set_environment_map(PbrtHipScene* s, int32_t light, const float* rgb, int32_t width, int32_t height,
                                                  const float light_to_world[16]) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_environment_map: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (light < 0 || light >= s->d.n_lights) return invalid("light index out of range");
    if (s->h_lights[light].type != PBRT_LIGHT_INFINITE) return invalid("light is not PBRT_LIGHT_INFINITE");
    if (!light_to_world) return invalid("null light_to_world");
    const float* m = light_to_world;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return invalid("light_to_world is not finite");
    if (m[12] != 0.0f || m[13] != 0.0f || m[14] != 0.0f || m[15] != 1.0f) return invalid("light_to_world's last row is not (0, 0, 0, 1)");
    // world_to_light's directions: the inverse of the upper 3x3, in double
    double a[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[3 * r + c] = m[4 * r + c];
    double inv[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                     a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                     a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    double det = a[0] * inv[0] + a[1] * inv[3] + a[2] * inv[6];
    DevEnvMap e{};
    for (int k = 0; k < 9; ++k) {
        e.l2w[k] = (float)a[k];
        e.w2l[k] = det != 0.0 ? (float)(inv[k] / det) : 0.0f;
        if (det == 0.0 || !std::isfinite(e.w2l[k])) return invalid("light_to_world is singular");
    }
    EnvTables t;
    if (const char* why = envmap_build(rgb, width, height, s->h_lights[light].L, &t)) return invalid(why);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<void*> fresh;
    auto release = [&]() {
        for (void* p : fresh) (void)hipFree(p);
    };
    auto upload = [&](const void* src, size_t bytes) -> void* {
        void* p = nullptr;
        if (!hip_ok(ctx, hipMalloc(&p, bytes), "hipMalloc environment map")) return nullptr;
        fresh.push_back(p);
        if (!hip_ok(ctx, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice), "hipMemcpy environment map")) return nullptr;
        return p;
    };
    std::vector<float4> texels((size_t)t.w * t.h);
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = make_float4(t.level0[3 * i], t.level0[3 * i + 1], t.level0[3 * i + 2], 0.0f);
    e.texels = (const float4*)upload(texels.data(), texels.size() * sizeof(float4));
    e.func = e.texels ? (const float*)upload(t.func.data(), t.func.size() * sizeof(float)) : nullptr;
    e.cdf = e.func ? (const float*)upload(t.cdf.data(), t.cdf.size() * sizeof(float)) : nullptr;
    e.row_int = e.cdf ? (const float*)upload(t.row_int.data(), t.row_int.size() * sizeof(float)) : nullptr;
    e.marg_cdf = e.row_int ? (const float*)upload(t.marg_cdf.data(), t.marg_cdf.size() * sizeof(float)) : nullptr;
    if (!e.marg_cdf) {
        release();
        return PBRT_HIP_ERR_DEVICE;
    }
    e.marg_int = t.marg_int;
    e.w = t.w;
    e.h = t.h;
    e.nu = t.nu;
    e.nv = t.nv;
    const int n = s->d.n_lights;
    if (!s->d.env_maps) {
        void* p = nullptr;
        if (!hip_ok(ctx, hipMalloc(&p, (size_t)n * sizeof(DevEnvMap)), "hipMalloc environment maps")) {
            release();
            return PBRT_HIP_ERR_DEVICE;
        }
        s->allocs.push_back(p);
        s->d.env_maps = (const DevEnvMap*)p;
        s->h_env.assign(n, DevEnvMap{});
        s->env_allocs.assign(n, {});
    }
    // the light itself: its map, and InfiniteAreaLight::power (infinite.rs:131-133) for the power distribution
    DevLight lt = s->h_lights[light];
    lt.slot = light;
    const float scale = kPi * s->d.world_radius * s->d.world_radius;
    float p[3] = {t.power_rgb[0] * scale, t.power_rgb[1] * scale, t.power_rgb[2] * scale};
    lt.power_y = 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2];
    std::vector<float> power_y(n), cdf;
    for (int i = 0; i < n; ++i) power_y[i] = i == light ? lt.power_y : s->h_lights[i].power_y;
    float fi;
    make_distribution(power_y, &cdf, &fi);
    std::vector<DevEnvMap> h_env = s->h_env;
    h_env[light] = e;
    std::vector<float> old_power_y(n), old_cdf;
    for (int i = 0; i < n; ++i) old_power_y[i] = s->h_lights[i].power_y;
    float old_fi;
    make_distribution(old_power_y, &old_cdf, &old_fi);
    // the device copies of the descriptors, the light and the power distribution, from one consistent host state
    auto write_state = [&](const std::vector<DevEnvMap>& env, const DevLight& l, const std::vector<float>& py, const std::vector<float>& pc) {
        return hip_ok(ctx, hipMemcpy((void*)s->d.env_maps, env.data(), (size_t)n * sizeof(DevEnvMap), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)(s->d.lights + light), &l, sizeof(DevLight), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)s->d.light_distrib_power.func, py.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)s->d.light_distrib_power.cdf, pc.data(), (size_t)(n + 1) * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
    };
    if (!write_state(h_env, lt, power_y, cdf)) {
        // put the previous state back; if that fails as well the device may still point at the new arrays: they then stay
        // allocated until the scene is destroyed instead of being freed under a descriptor that names them
        std::string why = ctx->last_error;
        if (write_state(s->h_env, s->h_lights[light], old_power_y, old_cdf)) {
            release();
        } else {
            s->allocs.insert(s->allocs.end(), fresh.begin(), fresh.end());
        }
        ctx->last_error = why;
        return PBRT_HIP_ERR_DEVICE;
    }
    s->d.light_distrib_power.func_int = fi;
    for (void* q : s->env_allocs[light]) (void)hipFree(q);  // a map set before on this light
    s->env_allocs[light].swap(fresh);
    s->h_env.swap(h_env);
    s->h_lights[light] = lt;
    if (s->d_spatial) {
        (void)hipFree(s->d_spatial);
        s->allocs.erase(std::remove(s->allocs.begin(), s->allocs.end(), (void*)s->d_spatial), s->allocs.end());
        s->d_spatial = nullptr;
    }
    return PBRT_HIP_OK;
}
PB_ABI_CATCH

// ProjectionLight::new / GonioPhotometricLight::new (lights/projection.rs:36-88, goniometric.rs:32-63) with the texels in memory:
// level 0 of the map's MIPMap goes to the device for light `light`, the projector's window follows the map's aspect, the light's
// power (D89) and the power distribution are recomputed, and a spatial light table already built is dropped.
extern "C" int pbrt_hip_scene_set_light_map(PbrtHipScene* s, int32_t light, const float* rgb, int32_t width, int32_t height) try {
    if (!s) return PBRT_HIP_ERR_INVALID;
    PbrtHipContext* ctx = s->ctx;
    PB_ENTER(ctx);
    auto invalid = [&](const std::string& why) {
        ctx->last_error = "pbrt_hip_scene_set_light_map: " + why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (light < 0 || light >= s->d.n_lights) return invalid("light index out of range");
    const int type = s->h_lights[light].type;
    if (type != PBRT_LIGHT_PROJECTION && type != PBRT_LIGHT_GONIOMETRIC) return invalid("light is not PBRT_LIGHT_PROJECTION or PBRT_LIGHT_GONIOMETRIC");
    if (!rgb) return invalid("null pointer");
    LightMapTables t;
    if (const char* why = light_map_build(type, s->light_fov[light], rgb, width, height, &t)) return invalid(why);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float4> texels((size_t)t.w * t.h);
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = make_float4(t.level0[3 * i], t.level0[3 * i + 1], t.level0[3 * i + 2], 0.0f);
    void* fresh = nullptr;
    if (!hip_ok(ctx, hipMalloc(&fresh, texels.size() * sizeof(float4)), "hipMalloc light map")) return PBRT_HIP_ERR_DEVICE;
    if (!hip_ok(ctx, hipMemcpy(fresh, texels.data(), texels.size() * sizeof(float4), hipMemcpyHostToDevice), "hipMemcpy light map")) {
        (void)hipFree(fresh);
        return PBRT_HIP_ERR_DEVICE;
    }
    DevLightMap m{};
    m.texels = (const float4*)fresh;
    m.w = t.w;
    m.h = t.h;
    m.inv_tan = t.inv_tan;
    std::memcpy(m.screen_bounds, t.screen_bounds, sizeof(m.screen_bounds));
    // the light itself: its power for the power distribution
    const int n = s->d.n_lights;
    DevLight lt = s->h_lights[light];
    if (type == PBRT_LIGHT_PROJECTION) lt.cos_total_width = t.cos_total_width;
    float p[3] = {lt.L[0] * t.power_rgb[0], lt.L[1] * t.power_rgb[1], lt.L[2] * t.power_rgb[2]};
    lt.power_y = 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2];
    std::vector<float> power_y(n), cdf, old_power_y(n), old_cdf;
    for (int i = 0; i < n; ++i) {
        old_power_y[i] = s->h_lights[i].power_y;
        power_y[i] = i == light ? lt.power_y : old_power_y[i];
    }
    float fi, old_fi;
    make_distribution(power_y, &cdf, &fi);
    make_distribution(old_power_y, &old_cdf, &old_fi);
    // the device copies of the descriptor, the light and the power distribution, from one consistent host state
    auto write_state = [&](const DevLightMap& dm, const DevLight& l, const std::vector<float>& py, const std::vector<float>& pc) {
        return hip_ok(ctx, hipMemcpy((void*)(s->d.light_maps + light), &dm, sizeof(DevLightMap), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)(s->d.lights + light), &l, sizeof(DevLight), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)s->d.light_distrib_power.func, py.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy") &&
               hip_ok(ctx, hipMemcpy((void*)s->d.light_distrib_power.cdf, pc.data(), (size_t)(n + 1) * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
    };
    if (!write_state(m, lt, power_y, cdf)) {
        // put the previous state back; if that fails as well the device may still point at the new texels: they then stay
        // allocated until the scene is destroyed instead of being freed under a descriptor that names them
        std::string why = ctx->last_error;
        if (write_state(s->h_light_maps[light], s->h_lights[light], old_power_y, old_cdf)) (void)hipFree(fresh);
        else s->allocs.push_back(fresh);
        ctx->last_error = why;
        return PBRT_HIP_ERR_DEVICE;
    }
    s->d.light_distrib_power.func_int = fi;
    if (s->light_map_allocs[light]) (void)hipFree(s->light_map_allocs[light]);  // a map set before on this light
    s->light_map_allocs[light] = fresh;
    s->h_light_maps[light] = m;
    s->h_lights[light] = lt;
    if (s->d_spatial) {
        (void)hipFree(s->d_spatial);
        s->allocs.erase(std::remove(s->allocs.begin(), s->allocs.end(), (void*)s->d_spatial), s->allocs.end());
        s->d_spatial = nullptr;
    }
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
    PbrtRay* d_rays = nullptr;
    void* d_out = nullptr;
    size_t out_bytes = ANY ? (size_t)n : (size_t)n * sizeof(PbrtHit);
    HIP_TRY(ctx, hipMalloc((void**)&d_rays, (size_t)n * sizeof(PbrtRay)));
    if (!hip_ok(ctx, hipMalloc(&d_out, out_bytes), "hipMalloc")) {
        (void)hipFree(d_rays);
        return PBRT_HIP_ERR_DEVICE;
    }
    int rc = PBRT_HIP_OK;
    if (!hip_ok(ctx, hipMemcpyAsync(d_rays, rays, (size_t)n * sizeof(PbrtRay), hipMemcpyHostToDevice, ctx->stream), "H2D"))
        rc = PBRT_HIP_ERR_DEVICE;
    if (rc == PBRT_HIP_OK) rc = launch_batch<ANY>(s, d_rays, n, (PbrtHit*)d_out, (uint8_t*)d_out);
    if (rc == PBRT_HIP_OK &&
        !hip_ok(ctx, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream), "D2H"))
        rc = PBRT_HIP_ERR_DEVICE;
    if (!hip_ok(ctx, hipStreamSynchronize(ctx->stream), "sync") && rc == PBRT_HIP_OK) rc = PBRT_HIP_ERR_DEVICE;
    (void)hipFree(d_rays);
    (void)hipFree(d_out);
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
