// scene.h — context / scene objects behind the C ABI and the device tables' rows. The tables are laid out on the host by
// host_scene.cpp (creation) and host_edit.cpp (the pbrt_hip_scene_set_* edits); pbrt_hip.hip puts them on the device.
//
// Scene::new (src/core/scene.rs:18-34) + GeometricPrimitive (src/core/primitive.rs:33-55) +
// BVHAccel's flat node array (src/accelerators/bvh.rs:129-135, 774-811), re-laid out for the
// gfx950 traversal kernel (layout described in trace.h).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"
#include "trace.h"
#include "wide_bvh.h"

// Calls that reach the device through one context are serialised: the reference's Primitive is Sync + Send and li() is
// re-entrant (src/core/primitive.rs:179, integrator.rs:412-452), so a drop-in may be entered from several host threads.
#define PB_LOCK(ctx) std::lock_guard<std::recursive_mutex> pb_lock_((ctx)->mu)
// ... and refused once the context is lost (a wavefront ran into the deadline: a kernel of that call may still be running
// on the stream, over buffers the call has abandoned; nothing else may be queued behind it or handed its memory)
#define PB_ENTER(ctx)                                                                                              \
    PB_LOCK(ctx);                                                                                                  \
    if ((ctx)->lost) {                                                                                             \
        (ctx)->last_error = "context lost: an earlier call ran into the wavefront deadline; destroy the context";  \
        return PBRT_HIP_ERR_DEVICE;                                                                                \
    }

struct PbrtHipContext {
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n_cus = 0;
    std::string last_error;
    // sticky: set when a call gave up on a kernel that did not finish (render.hip); every entry point then fails
    // (atomic: pbrt_hip_context_is_lost polls it from other threads without the lock)
    std::atomic<bool> lost{false};
    bool trace_log = false;  // PBRT_HIP_TRACE_LOG was set when the context was created: one stderr line per traversal launch
    double wavefront_deadline_s = 120.0;  // no wavefront of a render takes this long (pbrt_hip_context_set_deadline)
    // traversal-kernel timing (HIP events on `stream`)
    double trace_ms = 0.0;
    uint64_t trace_launches = 0;
    bool time_trace = true;
    // instrumented traversal (roofline accounting): device counters {node_tests, prim_tests}
    // 0 = off; 1 = the binary kernels count the reference's box / triangle tests; 2 = the wide kernels count their own
    // record / leaf / triangle fetches (pbrt_hip_set_counting)
    int count_traversal = 0;
    int traversal = 0;  // PBRT_TRAVERSAL_*: pbrt_hip_context_set_traversal
    int wide_build = 0;  // PBRT_WIDE_BUILD_*: pbrt_hip_context_set_wide_build
    int wide_layout = 0;  // PBRT_WIDE_LAYOUT_*: pbrt_hip_context_set_wide_layout
    int camera_packets = 0;  // 0 auto, 1 off: pbrt_hip_context_set_camera_packets (kernel_select.h: use_camera_packets)
    int camera_kernel = 0;   // PBRT_CAMERA_KERNEL_*: what traced wavefront 0 of the last render (pbrt_hip_context_camera_kernel)
    unsigned long long* d_counters = nullptr;  // [0..3] mode 1: node, prim, rays, instance tests; [4..7] mode 2
    uint64_t counted_rays = 0;
    // ray-queue heads of the persistent traversal kernels: [0, kQueueSegments) the launch's segments,
    // [kFollowUpCounter] the follow-up launch over the rays the wide kernel left out, [kSpecialCount] their number
    unsigned int* d_work_counter = nullptr;
    uint32_t* d_special_list = nullptr;  // batch calls: tokens (IO::token) of those rays (grown on demand)
    size_t special_capacity = 0;
    // the render loop reads the queue lengths back once per wavefront: pinned landing buffer + an event the host
    // spins on (a blocking stream sync costs a scheduler wake-up per wavefront, milliseconds on a busy host)
    unsigned long long* h_counts = nullptr;
    hipEvent_t ev_sync = nullptr;
    // Device blocks of finished renders, kept for the next one: a 64-spp 1080p frame holds 50 GB of path state and
    // hipMalloc / hipFree of that much costs seconds. Freed with the context (or when an allocation fails).
    struct CachedBlock {
        void* ptr;
        size_t bytes;
        bool in_use;
    };
    std::vector<CachedBlock> block_cache;
    // HaltonSampler tables, uploaded on first use: primes + prime sums, radical-inverse digit permutations
    uint32_t* d_halton_primes = nullptr;
    uint16_t* d_halton_perms = nullptr;
};

namespace pb {

constexpr int kWorkCounters = 16, kFollowUpCounter = 8, kSpecialCount = 12;

// device-side light / material tables
struct DevLight {
    int type;       // PbrtLightType
    float L[3];
    int slot;       // area light: leaf slot of its triangle; infinite light: its DevEnvMap (= its own index) or -1 (constant map);
                    // projection / goniometric light: its DevLightMap (= its own index)
    int two_sided;
    float area;     // Triangle::area (triangle.rs:323-328)
    float power_y;  // Light::power().y_value() for the power distribution
    // delta lights (lights/point.rs, spot.rs, distant.rs): p_light or w_light, spot cone, world_to_light 3x3
    float pos[3];
    float cos_total_width, cos_falloff_start;
    float w2l[9];
    int delta;      // is_delta_light (light.rs:28-31): no BSDF-sampling half, no MIS weight
};
struct DevMaterial {
    int type;
    float kd[3], kt[3];
    float eta;
    float alpha_u, alpha_v;  // plastic / metal: TrowbridgeReitzDistribution's alphas, computed on the host
};
// DevMaterial::type past PbrtMaterialType: the rows pbrt_hip_scene_set_material writes (wf_bxdfs.h). kMatOrenNayar: kd,
// OrenNayar's A / B in alpha_u / alpha_v; kMatRoughGlass: kd = Kr, kt = Kt, eta, the alphas; kMatSubstrate: kd, kt = Ks, the alphas
constexpr int kMatOrenNayar = 6, kMatRoughGlass = 7, kMatSubstrate = 8;
// kMatDisney: a row of pbrt_hip_scene_set_disney_material (wf_disney.h). The DevMaterial row keeps the colour in kd and eta; what
// the lobes read is the DevDisney block of the same index in DevSceneData::disney, computed on the host in double and rounded once (host_edit.cpp).
constexpr int kMatDisney = 9;
// DevDisney::lobes, in the order DisneyMaterial adds them (BSDF::sample_f picks a lobe by index)
constexpr int kDzDiffuse = 1, kDzFakeSS = 2, kDzRetro = 4, kDzSheen = 8, kDzMicro = 16, kDzClearcoat = 32, kDzTrans = 64, kDzLambertT = 128;
struct DevDisney {
    float diffuse[3];    // DisneyDiffuse R
    float fakess[3];     // DisneyFakeSS R (thin)
    float retro[3];      // DisneyRetro R
    float sheen[3];      // DisneySheen R
    float cspec0[3];     // DisneyFresnel R0
    float trans[3];      // MicrofacetTransmission T
    float lambert_t[3];  // LambertianTransmission T (thin)
    float metallic, eta, roughness;
    float ax, ay;        // the reflection lobe's alphas
    float tax, tay;      // the transmission lobe's (thin: the scaled roughness)
    float clearcoat;     // DisneyClearcoat weight
    float cc_a2, cc_ln_a2, cc_norm;  // its gloss g: g^2, ln g^2, (g^2 - 1) / (pi ln g^2)
    int lobes;           // kDz* bits
    int n;               // number of lobes, 1..8
    int sep_trans;       // the transmission lobe masks with G1(wo) G1(wi) (not thin)
};

// kMatLobes: a row of pbrt_hip_scene_set_lobe_material (wf_lobes.h): the reference's general BSDF, a list of up to 8 lobes of any
// kind matched by BxDFType flags. The DevMaterial row keeps the BSDF's eta; the list is the DevLobeRow of the same index in
// DevSceneData::lobe_rows, written by the host (host_lobes.cpp). A lobe is the public PbrtLobe (include/pbrt_hip.h).
constexpr int kMatLobes = 10;
constexpr int kMaxLobes = 8;
typedef PbrtLobe DevLobe;
struct DevLobeRow {
    int n;            // 0..8
    float eta;        // BSDF::eta
    int n_nonspec;    // num_components(BSDF_ALL & !BSDF_SPECULAR)
    int type_or;      // the lobes' BxDFType bits or-ed
    DevLobe lobes[kMaxLobes];
};

// kMatHair: a row of pbrt_hip_scene_set_hair_material (wf_hair.h): pbrt-v3's HairBSDF on a curve. The DevMaterial row keeps eta;
// the lobes' constants are the DevHair block, computed on the host in double and rounded once per field (host_edit.cpp). The block
// lives in the row's slot of DevSceneData::disney (a row is a Disney row or a hair row, never both; the row's type says how the
// slot reads), so no kernel's argument block grows.
constexpr int kMatHair = 11;
struct DevHair {
    float sigma_a[3];
    float eta;
    float v[4];               // longitudinal variances of p = 0, 1, 2 and of the residual
    float s;                  // the azimuthal logistic's scale
    float sin2k[3], cos2k[3]; // sin / cos of 2^k alpha
    float trim_k, cdf_lo;     // logistic cdf(pi, s) - cdf(-pi, s) and cdf(-pi, s): the trimmed logistic's normalisation
};
static_assert(sizeof(DevHair) <= sizeof(DevDisney), "a hair row's block lives in the row's slot of the Disney table");

// Distribution1D (src/core/sampling.rs:62-154) flattened: func[n], cdf[n+1]
struct DevDistribution1D {
    const float* func;
    const float* cdf;
    float func_int;
    int n;
};

// InfiniteAreaLight with an image map (pbrt_hip_scene_set_environment_map; lights/infinite.rs:36-82): level 0 of the
// MIPMap (the lookups are bilinear there) and the 2w x 2h sin-weighted Distribution2D (host_envmap.cpp). One per light.
struct DevEnvMap {
    const float4* texels;   // w * h, row t = 0 is theta = 0 (light-space +z)
    const float* func;      // nv * nu: the conditional rows (nu = 2w, nv = 2h)
    const float* cdf;       // nv * (nu + 1)
    const float* row_int;   // nv: the rows' integrals = the marginal's function
    const float* marg_cdf;  // nv + 1
    float marg_int;
    int w, h, nu, nv;
    float w2l[9], l2w[9];  // upper 3x3 of world_to_light / light_to_world, row-major
};

// ProjectionLight / GonioPhotometricLight (lights/projection.rs, goniometric.rs): what the light needs beyond DevLight's pos / L /
// w2l. One per light of a scene that holds such a light, named by DevLight::slot (= the light's own index). Level 0 of the map's
// MIPMap (pbrt_hip_scene_set_light_map; the lookups are bilinear there), not multiplied by I; texels == null: no map, the
// lookup is exactly 1.
struct DevLightMap {
    const float4* texels;    // w * h, row t = 0: projection the lowest screen y, goniometric theta = 0 (light-space +y)
    int w, h;
    float inv_tan;           // projection: 1 / tan(radians(fov) / 2), Transform::perspective's x / y scale
    float screen_bounds[4];  // projection: min.x, min.y, max.x, max.y
};

struct DevSceneData {
    DevBVH bvh;
    const int* slot_prim;       // leaf slot -> caller's triangle index
    const int* slot_instance;   // top-level leaf slot -> caller's instance index (instanced scenes)
    const DevMaterial* materials;
    const DevLight* lights;
    int n_lights;
    int n_materials;
    int n_infinite;             // number of lights with the INFINITE flag (scene.rs:29-31, D29 intended)
    const int* infinite_ids;
    // InfiniteAreaLight's 2x2 sin-weighted Distribution2D (lights/infinite.rs:59-73): conditional rows + marginal
    float env_cond_func[2][2], env_cond_cdf[2][3], env_cond_int[2];
    float env_marg_func[2], env_marg_cdf[3], env_marg_int;
    float world_center[3], world_radius;  // lights/infinite.rs:135-139
    DevDistribution1D light_distrib_uniform, light_distrib_power;
    const DevEnvMap* env_maps;  // [n_lights] once a map was set (DevLight::slot names the entry), else null
    const DevDisney* disney;    // [n_materials]: the blocks of the kMatDisney rows
    const DevLightMap* light_maps;  // [n_lights] when the scene holds a projection or goniometric light, else null
    const DevLobeRow* lobe_rows;    // [n_materials]: the lists of the kMatLobes rows
    const DevCurve* curves;         // [n_curves]: the rows of the curve segments (shapes_curve.h), null in a scene without curves
    int n_curves;
};

}  // namespace pb

namespace pb {
struct DevMotion;  // motion.h
}
struct PbrtHipScene {
    PbrtHipContext* ctx = nullptr;
    pb::DevSceneData d;          // device pointers inside
    std::vector<void*> allocs;   // everything to hipFree
    int n_tris = 0, n_nodes = 0, n_interior = 0, n_instances = 0;
    int spill_lanes = 0;
    std::vector<pb::DevLight> h_lights;
    std::vector<pb::DevMaterial> h_materials;  // the device table's host copy (pbrt_hip_scene_set_material_roughness)
    bool glossy = false;  // a plastic or metal material in the table: the shading kernels' glossy instantiations run
    bool bxdfs = false;   // a kMatOrenNayar / kMatRoughGlass / kMatSubstrate row in the table: their level-2 instantiations run
    bool disney = false;  // a kMatDisney row in the table: their level-3 instantiations run
    bool lobes = false;   // a kMatLobes row in the table: the shading kernels' lobe-list builds run
    bool hair = false;    // a kMatHair row in the table: the hair builds run (hair_kernels.hip)
    std::vector<uint8_t> row_off_curve;  // per material row: a triangle or a quadric shape names it (a hair row needs a curve's v)
    std::vector<pb::DevLobeRow> h_lobe_rows;  // the device table's host copy: a mix reads its operands' lists
    std::vector<int> h_lobe_origin;           // per row: the PbrtLobeMaterialType that wrote it, 0 for any other row
    bool light_maps = false;  // a projection or goniometric light in the table: the shading kernels' map-light builds run
    std::vector<pb::DevLightMap> h_light_maps;  // the device table's host copy
    std::vector<float> light_fov;                // per light: PbrtLight.fov (projection)
    std::vector<int> light_samples;  // max(1, n_samples) per light (light.rs:76)
    std::vector<pb::DevEnvMap> h_env;  // image maps of infinite lights (pbrt_hip_scene_set_environment_map): the descriptors' host copy
    // per light: the device arrays of its map (an infinite light's five, a projection / goniometric light's texels), to hipFree
    std::vector<std::vector<void*>> light_allocs;
    // SpatialLightDistribution tables (lightdistrib.rs:76-220), built on first use by a render with that strategy
    float* d_spatial = nullptr;
    int spatial_voxels[3] = {0, 0, 0};
    // 4-wide quantised records over the same tree (wide_bvh.h): the traversal kernels' fast path when present
    bool has_wide = false;
    pb::WideTrees wide{};
    int n_wide_records = 0;
    int wide_stack_need = 0;  // one-level scenes: WideTree::stack_need (the packet kernel's stack holds kPacketStack entries)
    std::string wide_reason;  // why the scene has none
    // moving instances (pbrt_hip_scene_create_two_level_moving): an instance with PbrtInstanceMotion.animated; the side table
    // (motion.h) has one row per top-level leaf slot and rides in the MOV kernels' arguments, not in DevBVH
    bool moving = false;
    const pb::DevMotion* d_motions = nullptr;
};

namespace pb {

inline bool hip_ok(PbrtHipContext* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    if (ctx) ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

// a device copy of n elements that the caller owns ...
template <class T>
inline T* dev_copy(PbrtHipContext* ctx, const T* src, size_t n, bool* ok) {
    void* p = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    if (!hip_ok(ctx, hipMalloc(&p, bytes), "hipMalloc")) {
        *ok = false;
        return nullptr;
    }
    if (n && !hip_ok(ctx, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D")) *ok = false;
    return (T*)p;
}
// ... and one that the scene owns
template <class T>
inline T* dev_upload(PbrtHipScene* s, const T* src, size_t n, bool* ok) {
    T* p = dev_copy(s->ctx, src, n, ok);
    if (p) s->allocs.push_back(p);
    return p;
}

// true when every one of the 3 * n_tris indices names a vertex (host_scene.cpp); whoever takes a mesh from the caller asks
// before the indices become subscripts and reports "vertex index out of range"
bool mesh_indices_in_range(const int32_t* indices, int64_t n_tris, int32_t n_verts);

// Device arrays of the 4-wide records of one tree, whoever laid them out (wide_gpu.hip on the device, host_wide.cpp on the
// host). The struct frees what it still owns; a scene that takes the arrays over nulls the pointers.
struct WideDeviceTree {
    uint32_t* nodes = nullptr;    // 12 dwords per record
    float* tris = nullptr;        // 12 floats per wide-order triangle
    float* leaf_boxes = nullptr;  // 8 floats per wide-order triangle position
    int32_t root_ref = 0;
    int n_records = -1;  // -1: not built (reason says why, where the builder reports it here)
    int stack_need = 0;
    const char* reason = nullptr;
    WideDeviceTree() = default;
    WideDeviceTree(const WideDeviceTree&) = delete;
    WideDeviceTree& operator=(const WideDeviceTree&) = delete;
    ~WideDeviceTree() {
        if (nodes) (void)hipFree(nodes);
        if (tris) (void)hipFree(tris);
        if (leaf_boxes) (void)hipFree(leaf_boxes);
    }
};
bool build_wide_tree_device(PbrtHipContext* ctx, const PbrtLinearBVHNode* d_nodes, int32_t n_nodes, const float* d_tris, int32_t n_slots,
                            const PbrtLinearBVHNode& root, WideDeviceTree* out, const char** reason);

// A single-level scene tree built and re-laid out on the device (hlbvh_gpu.hip). The struct frees the device arrays it
// still owns; the scene takes them over by nulling the pointers.
struct DeviceTree {
    DeviceTree() = default;
    DeviceTree(const DeviceTree&) = delete;
    DeviceTree& operator=(const DeviceTree&) = delete;
    ~DeviceTree() {
        if (inodes) (void)hipFree(inodes);
        if (tris) (void)hipFree(tris);
        if (slot_prim) (void)hipFree(slot_prim);
    }
    float4* inodes = nullptr;   // 64-B child-pair records
    float4* tris = nullptr;     // 48-B triangles in leaf order
    int* slot_prim = nullptr;   // leaf slot -> caller's triangle index
    float root_min[3], root_max[3];
    int root_ref = 0, count_bits = 0, n_interior = 0, n_nodes = 0;
    std::vector<int32_t> light_slot;  // per light: leaf slot of an area light's triangle, -1 otherwise
    // the 4-wide records (wide_bvh.h) laid over the device-built tree, on the device as well (wide_gpu.hip);
    // wide.n_records < 0: not built (wide_reason says why: PBRT_WIDE_BUILD_NONE, or the tree does not qualify).
    // PBRT_WIDE_BUILD_HOST: the host builder instead, on copies of the tree (the test of host == device).
    WideDeviceTree wide;
    const char* wide_reason = nullptr;
    std::vector<PbrtLinearBVHNode> h_nodes;
    std::vector<float> h_tris;
    double build_ms = 0.0;            // tree build; convert_ms: re-layout into the traversal format
    double convert_ms = 0.0;
};

// Evaluation of "Triangle::intersect returns false" (triangle.rs:197-216) with the default
// uv set (triangle.rs:66-70): degenerate uv frame or dpdu x dpdv == 0, and a zero geometric
// normal. Ray independent, so it is a per-triangle flag. Same float operation order as the kernel
// side (this file is compiled with -ffp-contract=off).
__host__ __device__ inline bool triangle_rejected_by_intersect(const float* a, const float* b, const float* c,
                                                              const float* uv6 = nullptr) {
    float uv[3][2] = {{0.0f, 0.0f}, {1.0f, 0.0f}, {1.0f, 1.0f}};
    if (uv6)  // per-vertex uvs of the mesh (triangle.rs:60-65)
        for (int k = 0; k < 6; ++k) uv[k / 2][k % 2] = uv6[k];
    float duv02[2] = {uv[0][0] - uv[2][0], uv[0][1] - uv[2][1]};
    float duv12[2] = {uv[1][0] - uv[2][0], uv[1][1] - uv[2][1]};
    float dp02[3], dp12[3];
    for (int k = 0; k < 3; ++k) {
        dp02[k] = a[k] - c[k];
        dp12[k] = b[k] - c[k];
    }
    float determinant = duv02[0] * duv12[1] - duv02[1] * duv12[0];
    bool degenerate_uv = __builtin_fabsf(determinant) < 1e-8f;
    float dpdu[3] = {0, 0, 0}, dpdv[3] = {0, 0, 0};
    if (!degenerate_uv) {
        float inv_det = 1.0f / determinant;
        for (int k = 0; k < 3; ++k) {
            dpdu[k] = (dp02[k] * duv12[1] - dp12[k] * duv02[1]) * inv_det;
            dpdv[k] = (dp02[k] * -duv12[0] + dp12[k] * duv02[0]) * inv_det;
        }
    }
    float cx = dpdu[1] * dpdv[2] - dpdu[2] * dpdv[1];
    float cy = dpdu[2] * dpdv[0] - dpdu[0] * dpdv[2];
    float cz = dpdu[0] * dpdv[1] - dpdu[1] * dpdv[0];
    if (degenerate_uv || (cx * cx + cy * cy + cz * cz) == 0.0f) {
        float e1[3], e2[3];
        for (int k = 0; k < 3; ++k) {
            e1[k] = c[k] - a[k];
            e2[k] = b[k] - a[k];
        }
        float nx = e1[1] * e2[2] - e1[2] * e2[1];
        float ny = e1[2] * e2[0] - e1[0] * e2[2];
        float nz = e1[0] * e2[1] - e1[1] * e2[0];
        if ((nx * nx + ny * ny + nz * nz) == 0.0f) return true;
    }
    return false;
}

// persistent kernels: enough blocks to fill every CU (LDS: 160 KiB / (kStackLds * 2 KiB) blocks of 256, at most 8)
inline int persistent_grid(const PbrtHipScene* s, int waves = PB_TRACE_WAVES, int stack_lds = kStackLds, int other_lds_bytes = 0) {
    int per_cu = std::min(waves, (160 * 1024) / (stack_lds * kTraceBlock * (int)sizeof(uint2) + other_lds_bytes));
    return std::min(s->ctx->n_cus * per_cu, s->spill_lanes / kTraceBlock);
}

// the stackless walk (trace_stackless.h) keeps no LDS: its grid is set by the registers alone
#ifndef PB_STACKLESS_WAVES
#define PB_STACKLESS_WAVES 5  // 80 registers: 6 waves spill 11 of them (config 3 trace-only: 5 -> 1137, 6 -> 1110, 8 -> 963 Mrays/s)
#endif
inline int stackless_grid(const PbrtHipScene* s) { return s->ctx->n_cus * PB_STACKLESS_WAVES; }
// PBRT_TRAVERSAL_STACKLESS covers single-level triangle scenes; sets last_error otherwise
inline bool stackless_applies(const PbrtHipScene* s) {
    if (!s->d.bvh.instanced && !s->d.bvh.has_spheres && s->ctx->count_traversal == 0) return true;
    s->ctx->last_error = s->ctx->count_traversal ? "PBRT_TRAVERSAL_STACKLESS has no counting variant (pbrt_hip_set_counting)"
                                                 : "PBRT_TRAVERSAL_STACKLESS: single-level triangle scenes only";
    return false;
}

}  // namespace pb

#define HIP_TRY(ctx, call)                                                 \
    do {                                                                   \
        if (!pb::hip_ok((ctx), (call), #call)) return PBRT_HIP_ERR_DEVICE; \
    } while (0)
