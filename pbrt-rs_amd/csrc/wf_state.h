// wf_state.h — path state in HBM, ray / shade queues and their block-aggregated append, camera and tile records (part of wavefront.h)
#pragma once
#include <hip/hip_runtime.h>

#include "scene.h"
#include "trace.h"
#include "trace_persistent.h"
#include "trace_wide.h"
#include "trace_stackless.h"
#include "wf_ray_expand.h"
#include "wf_params.h"

namespace pb {

constexpr int kTile = 16;  // integrator.rs:404 TILE_SIZE
enum PathFlags : int {
    PF_SPECULAR_BOUNCE = 1,
    PF_ALIVE = 2,       // a continuation ray is pending in ray slot 0
    PF_NEE_SHADOW = 4,  // a shadow ray is pending in slot 2
    PF_NEE_MIS = 8,     // a BSDF-sampled MIS ray is pending in slot 1
    PF_VALID = 16,      // the path belongs to a pixel inside pixel_bounds
};
enum RaySlot : int { RS_CONT = 0, RS_MIS = 1, RS_SHADOW = 2 };
// A trace-queue entry is record << 2 | what. `record` is the index of the path's transient records (PathState: rays, hits,
// pending estimate): the path's position in the shade queue of the launch that will read them, NOT the path number — the
// traversal kernels only ever use it as an index into ps.ray / ps.hit. `what`: the three ray slots, and RS_MIS_BOOL = the
// path's MIS ray (slot RS_MIS) of which only `found` is wanted. estimate_direct (integrator.rs:232-262) calls scene.intersect for the BSDF-sampled direction and
// then looks at the hit only if the light is an area light (`light_isect.primitive.get_area_light() == light`); for an
// infinite light everything that follows depends on `found_surface_interaction` alone. BVHAccel::intersect finds its first
// hit under the ray's original t_max, walking exactly as intersect_p walks, so `found` = "some leaf whose box passes holds a
// triangle that Triangle::intersect accepts" — a boolean that does not depend on the visiting order and needs no closest
// hit: such a ray is traced as an any-hit ray that skips the triangles Triangle::intersect rejects (IO::strict), ends at its
// first hit, and sorts with the shadow rays (+2.3 % of a config-3 frame, +4.3 % of config 5's: profiles/r04_wide_kernel_ladder.txt).
constexpr uint32_t RS_MIS_BOOL = 3;
static_assert(kTokCont == RS_CONT && kTokMis == RS_MIS && kTokShadow == RS_SHADOW && kTokMisBool == RS_MIS_BOOL,
              "wf_ray_expand.h writes the tokens of this format");
// estimate_direct_emit's return value carries this beside the PF_NEE_* bits (it is not a path flag)
constexpr int NEE_MIS_BOOL = 0x100;

// Two kinds of per-path data. PERSISTENT state (L, beta, rng, samp, pfilm) lives for the whole pass at the path's number p:
// the film kernels and the sampler find it there. TRANSIENT records (the three rays, their hit records, the pending
// direct-lighting estimate nee_*) live for one bounce: shade launch k-1 writes them, trace launch k and shade launch k read
// them, nothing looks at them again. In the path integrator they are indexed by the path's POSITION j IN THE SHADE QUEUE of
// launch k (the position block_reserve hands out), so that they stay dense while the paths die: at index p a survivor of
// bounce 3 sat alone in its cache line. Generation 0 is the identity (k_generate: j = p). Launch k reads generation k at its
// own thread index while it writes generation k+1 at other indices, so rays and nee_* exist twice (`*_next`; the host
// swaps the two after every launch); the hit records do not: trace launch k writes them after shade launch k-1 has read the
// previous ones. The stage machine of the other integrators (k_shade_direct) keeps all of it at p and uses no `*_next`.
struct PathState {
    float4* ray;     // [ray_index(j, slot) + k]: (o.xyz, d.x) (d.yz, t_max, -)
    // [hit_index(j, slot)]: (leaf slot of the hit or -1 as int bits, b0, b1, b2) — t is not kept: nothing downstream reads it
    // (the hit point comes from the barycentrics, triangle.rs:160-178) and ONE 16-B store per closest-hit ray is one memory
    // instruction less on the traversal kernel's refill path; [.. + 1]: (instance slot, -, -, -), written and read in two-level
    // scenes only; shadow slot: .x = occluded
    float4* hit;
    size_t n_paths;  // paths of a pass (the stride between the three slots' arrays)
    uint64_t* rng;   // [p] PCG32 state (inc is recomputed from the sample index)
    float4* L;       // [p] L.rgb, eta_scale
    float4* beta;    // [p] beta.rgb, (bounces << 8 | flags) as int bits
    float4* nee_a;   // [j] light-sampling contribution (if unoccluded) rgb, light pick pdf
    float4* nee_f;   // [j] BSDF-sampled f * |cos| rgb, MIS weight
    float4* nee_b;   // [j] beta at the NEE vertex rgb, scattering pdf
    int* nee_light;  // [j] light index of the pending estimate
    float2* pfilm;   // [p] CameraSample::p_film
    int* samp;       // [p] sampler counters: current_1d_dimension (Halton: dimension) | current_2d_dimension << 10 | array_2d_offset << 16
    // the generation k_shade writes (path integrator only)
    float4* ray_next;
    float4 *nee_a_next, *nee_f_next, *nee_b_next;
    int* nee_light_next;
    int two_level;   // the scene has instances: hit records carry the instance slot in their second float4
};
// the instance slot of a hit record (-1: none)
PB_DEV int hit_instance(const PathState& ps, size_t hit_base) { return ps.two_level ? __float_as_int(ps.hit[hit_base + 1].x) : -1; }

// Rays and hit records are kept slot-major, [slot][path][2 x float4]: the lanes of a wave that write (k_generate,
// k_shade) or read (the unsorted wavefronts of k_trace) the same slot of consecutive paths touch consecutive 32-B
// pieces, i.e. whole cache lines; path-major [path][slot] left two thirds of every written line untouched.
#ifndef PB_RAY_PATH_MAJOR
#define PB_RAY_PATH_MAJOR 0
#endif
#ifndef PB_HIT_PATH_MAJOR
#define PB_HIT_PATH_MAJOR 0
#endif
PB_DEV size_t ray_index(const PathState& ps, uint32_t j, int slot) {
    return PB_RAY_PATH_MAJOR ? ((size_t)j * 3 + slot) * 2 : ((size_t)slot * ps.n_paths + j) * 2;
}
PB_DEV size_t hit_index(const PathState& ps, uint32_t j, int slot) {
    return PB_HIT_PATH_MAJOR ? ((size_t)j * 3 + slot) * 2 : ((size_t)slot * ps.n_paths + j) * 2;
}

// SamplerParams, PassParams: wf_params.h

// path number <-> (sample of the pass, pixel of the tile set). Paths are laid out wave by wave: wave w holds the pixel block
// b = w % (n_pix / Pw) (Pw = 64 >> group_shift consecutive pixels) and the sample group g = w / (n_pix / Pw) (G = 1 << group_shift
// consecutive samples); lane l of it is pixel b Pw + l % Pw, sample g G + l / Pw. group_shift 0 is path = sample * n_pix + pixel.
PB_DEV void path_to_sample_pixel(const PassParams& pp, uint32_t p, int* s_local, int* pix) {
    const uint32_t sh = (uint32_t)pp.group_shift, pw_bits = 6u - sh;
    const uint32_t w = p >> 6, l = p & 63u, blocks = (uint32_t)pp.n_pix >> pw_bits;
    const uint32_t g = w / blocks, b = w - g * blocks;
    *pix = (int)((b << pw_bits) | (l & ((1u << pw_bits) - 1u)));
    *s_local = (int)((g << sh) | (l >> pw_bits));
}
PB_DEV uint32_t sample_pixel_to_path(const PassParams& pp, int s_local, uint32_t pix) {
    const uint32_t sh = (uint32_t)pp.group_shift, pw_bits = 6u - sh;
    const uint32_t g = (uint32_t)s_local >> sh, b = pix >> pw_bits, blocks = (uint32_t)pp.n_pix >> pw_bits;
    const uint32_t l = (((uint32_t)s_local & ((1u << sh) - 1u)) << pw_bits) | (pix & ((1u << pw_bits) - 1u));
    return ((g * blocks + b) << 6) | l;
}

struct Queues {
    uint32_t* trace;   // entries: record*4 + slot (record = the path's position in `shade`; k_shade_direct: the path)
    uint32_t* shade;   // entries: path; entry j's transient records are at index j (k_shade_direct: at the path's number)
    // counts64[0]: low 32 bits = trace-queue length, high 32 bits = shadow rays among them;
    // counts64[1]: shade-queue length
    unsigned long long* counts64;
    // set when the next wavefront will be traced in Morton order, null otherwise. While set, the shading kernel writes no
    // trace-queue entries: per path that emits a ray it leaves ONE sort pair at the path's position j in `shade`, the key
    // (ray_sort_cell of the point its rays leave from) in keys[j] and the value (path_entry_pack: record, which rays) in
    // trace[j]; the host sorts the pairs and expands them into `trace` (wf_ray_expand.h). counts64 means what it always means.
    uint32_t* keys;
    float key_lo[3], key_inv[3];  // scene bounds: lower corner, 1 / extent
};

#ifndef PB_SORT_AXIS_BITS
#define PB_SORT_AXIS_BITS 5
#endif
constexpr int kSortKeyBits = 3 * PB_SORT_AXIS_BITS;  // the any-hit rays are split off after the sort (wf_ray_expand.h), not by a key bit
// Morton code of the cell of `o` in the scene bounds, PB_SORT_AXIS_BITS bits per axis
PB_DEV uint32_t ray_sort_cell(float ox, float oy, float oz, const float* lo, const float* inv) {
    constexpr float kCells = (float)(1 << PB_SORT_AXIS_BITS);
    float fx = (ox - lo[0]) * inv[0], fy = (oy - lo[1]) * inv[1], fz = (oz - lo[2]) * inv[2];
    uint32_t q[3] = {(uint32_t)fminf(fmaxf(fx * kCells, 0.0f), kCells - 1.0f), (uint32_t)fminf(fmaxf(fy * kCells, 0.0f), kCells - 1.0f),
                     (uint32_t)fminf(fmaxf(fz * kCells, 0.0f), kCells - 1.0f)};
    uint32_t code = 0;
    for (int b = 0; b < PB_SORT_AXIS_BITS; ++b)
        for (int k = 0; k < 3; ++k) code |= ((q[k] >> b) & 1u) << (3 * b + k);
    return code;
}

// The pixel's number over the film's sample bounds (film.rs:76-81): with the 0.5 box filter that is y * width + x;
// with a wider filter the pixels sampled left of / above the film get numbers of their own ((width, y) and (0, y + 1)
// would share y * width + x, and with it their random streams).
PB_DEV int64_t pixel_number(const PassParams& pp, int x, int y) {
    return (int64_t)(y - pp.sb_y0) * pp.sb_w + (x - pp.sb_x0);
}
PB_DEV uint64_t sample_sequence(const PassParams& pp, int x, int y, int s) {
    return pp.seed ^ (uint64_t)(pixel_number(pp, x, y) * (int64_t)pp.spp + s);
}

// Block-aggregated queue append. Same-address atomics saturate near 10^2 per microsecond on the
// whole chip, so one atomic per wave (260 k waves per launch) would cost milliseconds: lanes are
// ranked inside the wave with ballot + mbcnt, waves inside the block through LDS, and ONE lane
// per block reserves the block's range with a single 64-bit atomicAdd per queue.
struct BlockAppend {
    uint32_t wave_rays[16];   // per-wave totals (blocks of up to 1024 threads)
    uint32_t wave_shadow[16];
    uint32_t wave_paths[16];
    uint32_t base_rays, base_paths;
};
PB_DEV uint32_t lane_prefix(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
// Every thread of the block must call block_reserve. cont/mis/shadow: the path queues that ray; again = it stays in the
// shade queue. Returns where the thread's entries go; `shade` is the path's position in the output shade queue, i.e. the
// record index of everything it hands to the next launch (known only here, after the block-wide count).
struct AppendSlots {
    uint32_t cont, mis, shadow, shade;
};
PB_DEV AppendSlots block_reserve(BlockAppend& sh, const Queues& q, bool cont, bool mis, bool shadow, bool again) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63) >> 6;
    unsigned long long mc = __ballot(cont), mm = __ballot(mis), ms = __ballot(shadow), ma = __ballot(again);
    uint32_t wc = (uint32_t)__popcll(mc), wm = (uint32_t)__popcll(mm), ws = (uint32_t)__popcll(ms);
    if (lane == 0) {
        sh.wave_rays[wave] = wc + wm + ws;
        sh.wave_shadow[wave] = ws;
        sh.wave_paths[wave] = (uint32_t)__popcll(ma);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tr = 0, tsd = 0, tp = 0;
        for (int w = 0; w < n_waves; ++w) {
            uint32_t r = sh.wave_rays[w], pth = sh.wave_paths[w];
            sh.wave_rays[w] = tr;   // exclusive prefix
            sh.wave_paths[w] = tp;
            tr += r;
            tsd += sh.wave_shadow[w];
            tp += pth;
        }
        unsigned long long old = 0;
        if (tr) old = atomicAdd(&q.counts64[0], (unsigned long long)tr | ((unsigned long long)tsd << 32));
        sh.base_rays = (uint32_t)old;
        sh.base_paths = tp ? (uint32_t)atomicAdd(&q.counts64[1], (unsigned long long)tp) : 0u;
    }
    __syncthreads();
    uint32_t rbase = sh.base_rays + sh.wave_rays[wave];
    // within the wave: all continuation rays, then MIS rays, then shadow rays
    AppendSlots a;
    a.cont = rbase + lane_prefix(mc);
    a.mis = rbase + wc + lane_prefix(mm);
    a.shadow = rbase + wc + wm + lane_prefix(ms);
    a.shade = sh.base_paths + sh.wave_paths[wave] + lane_prefix(ma);
    return a;
}
// The queue writes that go with a reservation: path p into the shade queue, its rays (records at index `rec`) into the
// trace queue. mis_bool: the MIS ray is queued as RS_MIS_BOOL. With q.keys set the path's rays go into one sort pair at its
// shade-queue position instead (see Queues::keys): the three rays leave from the same surface point, so one cell
// (ray_sort_cell of that point) serves them all; a path that stays in the shade queue emits at least one ray.
PB_DEV void block_write(const Queues& q, const AppendSlots& a, uint32_t p, uint32_t rec, bool cont, bool mis, bool shadow, bool again,
                        uint32_t cell, bool mis_bool) {
    if (q.keys) {
        if (again) {
            q.keys[a.shade] = cell;
            q.trace[a.shade] = path_entry_pack(rec, cont, mis, shadow, mis_bool);  // rec < 2^kPathRecBits: RenderJob::alloc_path_buffers
            q.shade[a.shade] = p;
        }
        return;
    }
    if (cont) q.trace[a.cont] = rec * 4u + RS_CONT;
    if (mis) q.trace[a.mis] = rec * 4u + (mis_bool ? RS_MIS_BOOL : (uint32_t)RS_MIS);
    if (shadow) q.trace[a.shadow] = rec * 4u + RS_SHADOW;
    if (again) q.shade[a.shade] = p;
}
// both at once, for a kernel that keeps its records at the path's number (k_shade_direct)
PB_DEV void block_append(BlockAppend& sh, const Queues& q, uint32_t p, bool cont, bool mis, bool shadow, bool again,
                         uint32_t cell = 0, bool mis_bool = false) {
    const AppendSlots a = block_reserve(sh, q, cont, mis, shadow, again);
    block_write(q, a, p, p, cont, mis, shadow, again, cell, mis_bool);
}

PB_DEV void store_ray(const PathState& ps, uint32_t j, int slot, V3 o, V3 d, float tmax) {
    size_t i = ray_index(ps, j, slot);
    ps.ray[i] = make_float4(o.x, o.y, o.z, d.x);
    ps.ray[i + 1] = make_float4(d.y, d.z, tmax, 0.0f);
}

// Where a shading kernel leaves the transient records it produces for the next launch (estimate_direct_emit writes through
// one of these). RecordSink: straight into the path state at a known index (k_shade_direct: the path's number).
struct RecordSink {
    const PathState& ps;
    uint32_t rec;
    PB_DEV void ray(int slot, V3 o, V3 d, float tmax) const { store_ray(ps, rec, slot, o, d, tmax); }
    PB_DEV void nee_a(float4 v) const { ps.nee_a[rec] = v; }
    PB_DEV void nee_f(float4 v) const { ps.nee_f[rec] = v; }
    PB_DEV void nee_b(float4 v) const { ps.nee_b[rec] = v; }
    PB_DEV void nee_light(int v) const { ps.nee_light[rec] = v; }
};
// StagedRecords: k_shade learns a path's output position only after the block-wide count, long after the values were
// computed; holding the up to 34 of them in registers would push the kernel over its 168-VGPR budget (three waves per
// SIMD), so they wait in LDS (37 KB per block of 256, three blocks per CU fit), each thread in its own column, and
// flush() moves them to generation k+1 at the reserved index. Values pass through unchanged.
struct StagedRecords {
    float4 ray[3][2][256];
    float4 nee_a[256], nee_f[256], nee_b[256];
    int nee_light[256];
};
struct StageSink {
    StagedRecords& st;
    PB_DEV void ray(int slot, V3 o, V3 d, float tmax) const {
        st.ray[slot][0][threadIdx.x] = make_float4(o.x, o.y, o.z, d.x);
        st.ray[slot][1][threadIdx.x] = make_float4(d.y, d.z, tmax, 0.0f);
    }
    PB_DEV void nee_a(float4 v) const { st.nee_a[threadIdx.x] = v; }
    PB_DEV void nee_f(float4 v) const { st.nee_f[threadIdx.x] = v; }
    PB_DEV void nee_b(float4 v) const { st.nee_b[threadIdx.x] = v; }
    PB_DEV void nee_light(int v) const { st.nee_light[threadIdx.x] = v; }
    // the thread's own staged records -> the next generation at record index j (what the path emitted, nothing else:
    // a specular bounce holds a slot with its continuation ray only)
    PB_DEV void flush(const PathState& ps, uint32_t j, bool cont, bool mis, bool shadow) const {
        const uint32_t t = threadIdx.x;
        if (cont) {
            size_t i = ray_index(ps, j, RS_CONT);
            ps.ray_next[i] = st.ray[RS_CONT][0][t];
            ps.ray_next[i + 1] = st.ray[RS_CONT][1][t];
        }
        if (mis) {
            size_t i = ray_index(ps, j, RS_MIS);
            ps.ray_next[i] = st.ray[RS_MIS][0][t];
            ps.ray_next[i + 1] = st.ray[RS_MIS][1][t];
            ps.nee_f_next[j] = st.nee_f[t];
        }
        if (shadow) {
            size_t i = ray_index(ps, j, RS_SHADOW);
            ps.ray_next[i] = st.ray[RS_SHADOW][0][t];
            ps.ray_next[i + 1] = st.ray[RS_SHADOW][1][t];
        }
        if (mis || shadow) {
            ps.nee_a_next[j] = st.nee_a[t];
            ps.nee_b_next[j] = st.nee_b[t];
            ps.nee_light_next[j] = st.nee_light[t];
        }
    }
};

// ---- camera: PerspectiveCamera::generate_ray (cameras/perspective.rs:90-112) ----
struct DevCamera {
    float c2w[16], r2c[16];
    float lens_radius, focal_distance, shutter_open, shutter_close;
    int kind;  // PbrtCameraKind
};
PB_DEV V3 xform_point(const float* m, V3 p) {  // transform.rs:351-370
    float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    if (wp == 1.0f) return V3{xp, yp, zp};
    return V3{xp, yp, zp} / wp;
}
PB_DEV V3 xform_vector(const float* m, V3 v) {  // transform.rs:372-385
    return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z,
              m[8] * v.x + m[9] * v.y + m[10] * v.z};
}

struct TileList {
    const int2* origin;  // tile origins of this GPU
    int n_tiles;
};

}  // namespace pb
