// trace_wide_packet.h — the camera wavefront over the 4-wide records (wide_bvh.h), walked ONCE PER WAVE.
//
// Since the path layout of round 5 a wave of camera paths is the 64 samples of one pixel (PassParams::group_shift == 6): 64 rays
// from one point through one pixel, about a quarter of a triangle wide on config 3. In trace_wide every one of the 64 lanes
// fetches the same record, decodes the same descriptor bytes, orders the same children by the same three sign bits, keeps the
// same stack and fetches the same triangle. Here the wave does all of that once, on the scalar unit: records and triangles arrive
// as wave-uniform data (scalar loads; no vector-memory instruction in the walk), order and descriptors are scalar arithmetic, there
// is one stack of child references per wave, and a lane keeps only what is its own: its ray, the four box tests of a record and
// the reference's slab and triangle tests of a leaf.
//
// Why the results are the reference's (the argument of wide_bvh.h, one step further). The reference's result for a ray is "for
// every leaf in near-first depth-first order: if the leaf's exact box passes Bounds3f::intersect_p with the t_max of that
// moment, test its triangles". That order depends on the ray only through its three dir_is_neg bits (bvh.rs:857-865), so all
// rays of one `negmask` share one total order of the leaves. The wave walks that order once per negmask group: a child of a
// record is visited when ANY lane of the group passes wide_child_test with its own ray and its own t_max — for every lane a
// superset of the leaves its own walk (trace_wide) would reach, in the same order. At a leaf every lane runs the reference's
// slab test on the exact leaf box with its own current t_max and then Triangle::intersect_test: a lane that would not have come
// here on its own sees extra leaves only, each of which fails or passes exactly as the reference's test says. Lanes outside
// the group, placeholders of paths outside pixel_bounds and positions past the end of the queue are inert: their walk t_max
// is negative, with which no child test and no triangle test can pass. As in trace_wide, a ray wide_ray_covered rejects and a
// ray whose t_max moves UP by an ulp (see `raised` there) go to `special_list` and are traced by the binary kernel afterwards.
// The host model of this walk is tests/native/packet_walk_check.cpp.
//
// Closest-hit rays of one-level scenes only (the camera wavefront has no others); no counting variant.
#pragma once
#include "trace_wide.h"

namespace pb {

#ifndef PB_PACKET_WAVES
#define PB_PACKET_WAVES 8  // waves per SIMD: no per-lane stack, 64 VGPRs (12 bytes of scratch outside the walk); 7 (66 VGPRs, none) measures the same
#endif
#ifndef PB_PACKET_FETCH
#define PB_PACKET_FETCH 0  // 0: scalar loads (s_load_dwordx8 + x4); 1: one global_load_dword (lane i = dword i) + v_readlane. The bare fetch is 6 % faster
                           // in form 1 (pbrt_hip_probe_packet_fetch), the kernel 4 % slower (twelve v_readlane per step): profiles/r14_camera_packets.txt
#endif
constexpr int kPacketStack = 64;  // child references per wave in LDS; a tree whose WideTree::stack_need exceeds it keeps trace_wide
constexpr int kPacketGrab = 2;    // units (of 64 queue positions) per grab from the queue head, = kChunk rays

template <class IO>
PB_DEV void trace_wide_packet(const WideTrees& wt, const IO& io, unsigned int* __restrict__ work_counter, uint32_t* lds_wave_stack) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) uint32_t LdsRef;
#else  // the host pass only parses this function
    typedef uint32_t LdsRef;
#endif
    LdsRef* const stack = (LdsRef*)lds_wave_stack;
    const uint32_t packed_mask = wt.vec_stride == 3 ? ~0u : 0u;  // (trace_wide: wide_vec_offset)
    auto vec_offset = [&](uint32_t i) -> size_t { return (size_t)((i << 2) - (i & packed_mask)); };
    // three 16-byte vectors at a wave-uniform index. Form 0 is written as the two instructions themselves: through a pointer
    // into the constant address space the compiler fetches the first 16 bytes with a (uniform) global_load_dwordx4 and only the
    // rest with a scalar load.
    auto fetch3 = [&](const void* base, uint32_t i, uint4* a, uint4* b, uint4* c) {
#if !defined(__HIP_DEVICE_COMPILE__)
        *a = *b = *c = make_uint4(0u, 0u, 0u, 0u);  // the host pass only parses this function
        (void)vec_offset;
#elif PB_PACKET_FETCH == 0
        typedef uint32_t U8 __attribute__((ext_vector_type(8)));
        typedef uint32_t U4 __attribute__((ext_vector_type(4)));
        const uint4* p = (const uint4*)base + vec_offset(i);
        U8 lo;
        U4 hi;
        asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(lo), "=&s"(hi) : "s"(p) : "memory");
        *a = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *b = make_uint4(lo[4], lo[5], lo[6], lo[7]);
        *c = make_uint4(hi[0], hi[1], hi[2], hi[3]);
#else
        const int l = (int)(threadIdx.x & 63u);
        const uint32_t w = ((const uint32_t*)((const uint4*)base + vec_offset(i)))[l < 12 ? l : 0];
        *a = make_uint4(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 1), __builtin_amdgcn_readlane(w, 2), __builtin_amdgcn_readlane(w, 3));
        *b = make_uint4(__builtin_amdgcn_readlane(w, 4), __builtin_amdgcn_readlane(w, 5), __builtin_amdgcn_readlane(w, 6), __builtin_amdgcn_readlane(w, 7));
        *c = make_uint4(__builtin_amdgcn_readlane(w, 8), __builtin_amdgcn_readlane(w, 9), __builtin_amdgcn_readlane(w, 10), __builtin_amdgcn_readlane(w, 11));
#endif
    };
    // two 16-byte vectors at a wave-uniform address (a leaf's exact box), scalar in either form
    auto fetch2 = [&](const uint4* p, uint4* a, uint4* b) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef uint32_t U8 __attribute__((ext_vector_type(8)));
        U8 v;
        asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(p) : "memory");
        *a = make_uint4(v[0], v[1], v[2], v[3]);
        *b = make_uint4(v[4], v[5], v[6], v[7]);
#else
        *a = *b = make_uint4(0u, 0u, 0u, 0u);
#endif
    };
    const uint32_t n = io.n();
    const uint32_t n_units = (n + 63u) >> 6;
    const int lane = threadIdx.x & 63;
    const int n_seg = io.segments();
    int seg = (int)(blockIdx.x % (unsigned)n_seg), seg_tries = 0;
    uint32_t unit_next = 0, unit_end = 0;
    constexpr int kNone = (int)0x80000000;  // no child reference (a leaf reference is ~(first << 2 | n - 1), first < 2^29)

    for (;;) {
        // ---------------- the wave's next unit: 64 consecutive, 64-aligned queue positions ----------------
        if (unit_next >= unit_end) {
            while (seg_tries < n_seg) {
                const uint32_t seg_begin = (uint32_t)(((unsigned long long)n_units * (unsigned)seg) / (unsigned)n_seg);
                const uint32_t seg_end = (uint32_t)(((unsigned long long)n_units * (unsigned)(seg + 1)) / (unsigned)n_seg);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(work_counter + seg, (unsigned int)kPacketGrab);
                base = (uint32_t)__builtin_amdgcn_readfirstlane(base) + seg_begin;
                if (base < seg_end && base >= seg_begin) {
                    unit_next = base;
                    unit_end = (base + kPacketGrab) < seg_end ? (base + kPacketGrab) : seg_end;
                    break;
                }
                seg = (seg + 1 == n_seg) ? 0 : seg + 1;
                seg_tries += 1;
            }
            if (unit_next >= unit_end) break;
        }
        const uint32_t pos = (unit_next << 6) + (uint32_t)lane;
        unit_next += 1;

        // ---------------- the lane's own ray (tokens, rays and hit records at the lane's own index: full lines) ----------------
        const bool in_queue = pos < n;
        uint32_t index = 0;
        TravRay r;
        r.ox = r.oy = r.oz = 0.0f;
        r.dx = r.dy = 0.0f;
        r.dz = 1.0f;
        r.tmax = -1.0f;
        bool real = false;
        if (in_queue) {
            bool any;
            index = io.token(pos);
            real = io.load(index, &r, &any);  // (closest-hit rays only; false: the placeholder of a path outside pixel_bounds)
        }
        if (!real) {  // an inert lane computes with finite numbers
            r.dx = r.dy = r.dz = 1.0f;
            r.tmax = -1.0f;
        }
        const float idx = 1.0f / r.dx, idy = 1.0f / r.dy, idz = 1.0f / r.dz;  // bvh.rs:831
        const uint32_t negmask = (idx < 0.0f ? 1u : 0u) | (idy < 0.0f ? 2u : 0u) | (idz < 0.0f ? 4u : 0u);  // bvh.rs:832-836
        bool special = real && !wide_ray_covered(r.ox, r.oy, r.oz, idx, idy, idz);
        float tmax = r.tmax, hb0 = 0.0f, hb1 = 0.0f, hb2 = 0.0f;
        int hit_slot = -1;
        {
            const unsigned long long sm = __ballot(special);
            if (sm) {  // traced by the binary kernel afterwards (results written there)
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(wt.special_count, (unsigned int)popc64(sm));
                base = (uint32_t)__builtin_amdgcn_readfirstlane(base);
                if (special)
                    wt.special_list[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm, 0))] = index;
            }
        }

        // ---------------- one walk per negmask group (a perspective camera: one, but on the image's centre row and column) ----------------
        unsigned long long todo = __ballot(real && !special);
        while (todo) {
            const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)negmask, __builtin_ctzll(todo));
            const bool in_group = real && !special && negmask == g;
            todo &= ~__ballot(in_group);
            const bool gx = (g & 1u) != 0, gy = (g & 2u) != 0, gz = (g & 4u) != 0;
            float tm = in_group ? tmax : -1.0f;  // the walk's t_max: negative = inert
            bool raised = false;
            int cur = wt.root_ref, sp = 0;
            for (;;) {
                if (cur >= 0) {
                    // ---- a record: the four box tests per lane, everything else once per wave ----
                    uint4 q0, q1, q2;
                    fetch3(wt.nodes, (uint32_t)cur, &q0, &q1, &q2);
                    const uint32_t dw3 = q0.w;
                    const WideSetup ws = wide_setup(q0.x, q0.y, q0.z, dw3, r.ox, r.oy, r.oz, idx, idy, idz);
                    const uint32_t nqx = gx ? q1.y : q1.x, fqx = gx ? q1.x : q1.y;
                    const uint32_t nqy = gy ? q1.w : q1.z, fqy = gy ? q1.z : q1.w;
                    const uint32_t nqz = gz ? q2.y : q2.x, fqz = gz ? q2.x : q2.y;
                    // slots in record order (static byte selects); which of them any lane passes, as four bits
                    const uint32_t mslot = (q0.x & 0xffu) | ((q0.y & 0xffu) << 8) | ((q0.z & 0xffu) << 16) | (dw3 & 0xff000000u);
                    uint32_t hits = 0;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float tn;
                        const bool h = wide_child_test(ws, nqx, nqy, nqz, fqx, fqy, fqz, s, tm, &tn);
                        if (__ballot(h) != 0ull && ((mslot >> (8 * s)) & 0xffu) != 0xffu) hits |= 1u << s;
                    }
                    // The reference's visiting order of the four slots (trace_wide: `sel`, byte k = the slot visited k-th), from
                    // the group's sign bits; the children any lane passes are taken in that order, the later ones go on the
                    // stack, last one deepest.
                    const uint32_t f_root = (g >> ((dw3 >> 18) & 3u)) & 1u;
                    const uint32_t f_c0 = (g >> ((dw3 >> 20) & 3u)) & 1u, f_c1 = (g >> ((dw3 >> 22) & 3u)) & 1u;
                    uint32_t sel = 0x03020100u ^ (f_c0 ? 0x00000101u : 0u) ^ (f_c1 ? 0x01010000u : 0u);
                    if (f_root) sel = (sel >> 16) | (sel << 16);
                    const uint32_t child_base = q2.z, ntb = q2.w;
                    int next = kNone;
#pragma unroll
                    for (int k = 3; k >= 0; --k) {
                        const uint32_t s = (sel >> (8 * k)) & 3u;
                        if ((hits >> s) & 1u) {
                            const uint32_t m = (mslot >> (8 * s)) & 0xffu;
                            if (next != kNone) {
                                stack[sp] = (uint32_t)next;
                                sp += 1;
                            }
                            next = (m & 0x80u) ? (int)(child_base + (m & 3u)) : (int)(ntb - m);
                        }
                    }
                    cur = next;
                } else {
                    // ---- a leaf: the reference's box test on the exact leaf box, then its triangles (trace_wide's leaf phase) ----
                    const int v = ~cur;
                    const int cnt = (v & 3) + 1;
                    const uint32_t first = (uint32_t)(v >> 2);
                    uint4 ua, ub, uc;
                    fetch3(wt.tris, first, &ua, &ub, &uc);
                    float ax = wide_as_float(ua.x), ay = wide_as_float(ua.y), az = wide_as_float(ua.z), bx = wide_as_float(ua.w);
                    float by = wide_as_float(ub.x), bz = wide_as_float(ub.y), cx = wide_as_float(ub.z), cy = wide_as_float(ub.w);
                    float cz = wide_as_float(uc.x);
                    uint32_t tslot = uc.y, tflags = uc.z;
                    float lox, loy, loz, hix, hiy, hiz;
                    if (cnt == 1) {
                        // Triangle::world_bound (the union of the three vertices): exact, so it is the leaf node's box
                        lox = wide_fmin(ax, wide_fmin(bx, cx));
                        hix = wide_fmax(ax, wide_fmax(bx, cx));
                        loy = wide_fmin(ay, wide_fmin(by, cy));
                        hiy = wide_fmax(ay, wide_fmax(by, cy));
                        loz = wide_fmin(az, wide_fmin(bz, cz));
                        hiz = wide_fmax(az, wide_fmax(bz, cz));
                    } else {
                        uint4 b0, b1;
                        fetch2((const uint4*)wt.leaf_boxes + 2 * (size_t)first, &b0, &b1);
                        lox = wide_as_float(b0.x);
                        loy = wide_as_float(b0.y);
                        loz = wide_as_float(b0.z);
                        hix = wide_as_float(b1.x);
                        hiy = wide_as_float(b1.y);
                        hiz = wide_as_float(b1.z);
                    }
                    float entry;
                    const bool pass = tm >= 0.0f && slab_test(gx ? hix : lox, gx ? lox : hix, gy ? hiy : loy, gy ? loy : hiy, gz ? hiz : loz, gz ? loz : hiz, r,
                                                idx, idy, idz, tm, &entry);
                    if (__ballot(pass) != 0ull) {
                        const TriRayConst trc = tri_ray_setup(r, idx, idy, idz);  // (per leaf, as trace_wide: four registers less across the walk)
                        for (int i = 0;;) {
                            float b0, b1, b2, t;
                            if (pass && triangle_test(V3{ax, ay, az}, V3{bx, by, bz}, V3{cx, cy, cz}, r, trc, tm, &b0, &b1, &b2, &t) &&
                                !((int)tflags & kTriDegenerate)) {
                                if (t > tm) raised = true;  // t_max would move UP (trace_wide: `raised`): the ray leaves this kernel, below
                                tm = t;                     // primitive.rs:70
                                hb0 = b0;
                                hb1 = b1;
                                hb2 = b2;
                                hit_slot = (int)tslot;
                            }
                            if (++i >= cnt) break;
                            fetch3(wt.tris, first + (uint32_t)i, &ua, &ub, &uc);
                            ax = wide_as_float(ua.x), ay = wide_as_float(ua.y), az = wide_as_float(ua.z), bx = wide_as_float(ua.w);
                            by = wide_as_float(ub.x), bz = wide_as_float(ub.y), cx = wide_as_float(ub.z), cy = wide_as_float(ub.w);
                            cz = wide_as_float(uc.x);
                            tslot = uc.y;
                            tflags = uc.z;
                        }
                        if (__ballot(raised) != 0ull) {
                            if (raised) {  // (one list append per such ray: they are rare)
                                wt.special_list[atomicAdd(wt.special_count, 1u)] = index;
                                special = true;
                                tm = -1.0f;
                                raised = false;
                            }
                        }
                    }
                    cur = kNone;
                }
                if (cur == kNone) {  // out of children: the wave's next stack entry
                    if (sp == 0) break;
                    sp -= 1;
                    cur = __builtin_amdgcn_readfirstlane((int)stack[sp]);
                }
            }
            if (in_group) tmax = tm;
        }

        // ---------------- results, at the lane's own index ----------------
        if (in_queue && !special) io.store(index, false, hit_slot >= 0, tmax, hb0, hb1, hb2, hit_slot, -1);
    }
}

// The camera wavefront of a one-level scene (render.hip: trace_wavefront selects it, with IO = WavefrontRayIO<false>);
// k_trace_special follows as after k_trace_wide.
template <class IO>
__global__ void __launch_bounds__(kTraceBlock, PB_PACKET_WAVES) k_trace_wide_packet(WideTrees wt, IO io, unsigned int* work_counter) {
    __shared__ uint32_t lds_stack[kPacketStack * (kTraceBlock / 64)];
    trace_wide_packet<IO>(wt, io, work_counter, lds_stack + kPacketStack * (threadIdx.x >> 6));
}

}  // namespace pb
