// wf_ray_expand.h — the sorted ray queue: one sort entry per PATH, expanded into the trace queue after the sort (part of wavefront.h)
//
// The up to three rays a path emits at a bounce leave from one surface point, so they share one sort cell (ray_sort_cell). When the
// next wavefront is traced in Morton order, k_shade therefore writes ONE (key, value) pair per path that emits anything, at the path's
// position in the output shade queue: key = the cell, value = path_entry_pack(record, which rays). The host sorts those pairs
// (a third of the entries a pair per ray would take) and the kernels below turn the sorted values into the token stream the
// traversal kernels read (record * 4 + slot, wf_state.h):
//   [0, C)      every closest-hit ray in sorted path order: a path's continuation ray, then its MIS ray unless that one is boolean;
//   [C, C + A)  every any-hit ray in sorted path order: a path's boolean MIS ray, then its shadow ray.
// The stream is a pure function of the sorted list: k_ray_expand_count leaves each block's (closest, any-hit) token counts, an
// exclusive scan over the blocks turns them into the blocks' offsets (the extra last element: the totals, i.e. C), and
// k_ray_expand_scatter ranks the tokens inside a block and writes them. No atomics: block completion order decides nothing.
//
// The packing and the section arithmetic are plain functions, compiled for the host too (tests/native/path_sort_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PB_XHD __host__ __device__ __forceinline__
#ifndef PB_PLAIN_KERNEL  // dev_math.h
#define PB_PLAIN_KERNEL __global__
#endif
#else
#define PB_XHD inline
#endif

namespace pb {

// value of a path's sort entry: rec << 4 | cont | mis << 1 | shadow << 2 | mis_bool << 3
constexpr int kPathFlagBits = 4;
constexpr int kPathRecBits = 28;  // records of a pass the packing holds: RenderJob sorts only passes of up to 2^28 paths
static_assert(kPathRecBits + kPathFlagBits == 32, "a path entry is one 32-bit sort value");
enum PathEntryFlags : uint32_t { PE_CONT = 1, PE_MIS = 2, PE_SHADOW = 4, PE_MIS_BOOL = 8 };
// the `what` of a trace-queue token (wf_state.h pins these to RaySlot / RS_MIS_BOOL)
constexpr uint32_t kTokCont = 0, kTokMis = 1, kTokShadow = 2, kTokMisBool = 3;

PB_XHD uint32_t path_entry_pack(uint32_t rec, bool cont, bool mis, bool shadow, bool mis_bool) {
    return (rec << kPathFlagBits) | (cont ? PE_CONT : 0u) | (mis ? PE_MIS : 0u) | (shadow ? PE_SHADOW : 0u) | (mis_bool ? PE_MIS_BOOL : 0u);
}
PB_XHD uint32_t path_entry_rec(uint32_t v) { return v >> kPathFlagBits; }
// the MIS ray goes to one section or the other; PE_MIS_BOOL without PE_MIS means nothing
PB_XHD bool path_entry_mis_closest(uint32_t v) { return (v & (PE_MIS | PE_MIS_BOOL)) == PE_MIS; }
PB_XHD bool path_entry_mis_anyhit(uint32_t v) { return (v & (PE_MIS | PE_MIS_BOOL)) == (PE_MIS | PE_MIS_BOOL); }
// tokens the entry adds to the closest-hit / any-hit section (0..2 each)
PB_XHD uint32_t path_entry_closest(uint32_t v) { return (v & PE_CONT ? 1u : 0u) + (path_entry_mis_closest(v) ? 1u : 0u); }
PB_XHD uint32_t path_entry_anyhit(uint32_t v) { return (path_entry_mis_anyhit(v) ? 1u : 0u) + (v & PE_SHADOW ? 1u : 0u); }
// writes path_entry_closest(v) tokens to `closest` and path_entry_anyhit(v) tokens to `anyhit`, in section order
PB_XHD void path_entry_tokens(uint32_t v, uint32_t* closest, uint32_t* anyhit) {
    const uint32_t t = path_entry_rec(v) * 4u;
    if (v & PE_CONT) *closest++ = t + kTokCont;
    if (path_entry_mis_closest(v)) *closest = t + kTokMis;
    if (path_entry_mis_anyhit(v)) *anyhit++ = t + kTokMisBool;
    if (v & PE_SHADOW) *anyhit = t + kTokShadow;
}

// a block of the expansion kernels takes kExpandTile consecutive entries, four per thread
constexpr int kExpandBlock = 256, kExpandItems = 4, kExpandTile = kExpandBlock * kExpandItems;
inline uint32_t ray_expand_blocks(uint32_t n_entries) { return (n_entries + kExpandTile - 1) / kExpandTile; }

#if defined(__HIPCC__)
// the thread's four entries (0 = past the end: no rays); `entries` is 16-byte aligned and the tile starts at a multiple of four
__device__ __forceinline__ uint4 expand_load(const uint32_t* __restrict__ entries, uint32_t n, uint32_t first) {
    if (first + 4 <= n) return *reinterpret_cast<const uint4*>(entries + first);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (first < n) v.x = entries[first];
    if (first + 1 < n) v.y = entries[first + 1];
    if (first + 2 < n) v.z = entries[first + 2];
    return v;
}
// closest count | any-hit count << 16 of four entries (a tile's totals are at most 2048 each)
__device__ __forceinline__ uint32_t expand_counts(uint4 v) {
    const uint32_t c = path_entry_closest(v.x) + path_entry_closest(v.y) + path_entry_closest(v.z) + path_entry_closest(v.w);
    const uint32_t a = path_entry_anyhit(v.x) + path_entry_anyhit(v.y) + path_entry_anyhit(v.z) + path_entry_anyhit(v.w);
    return c | (a << 16);
}

// block_counts[b] = closest tokens of tile b | any-hit tokens << 32; block_counts[gridDim.x] = 0 (the scan's totals slot)
PB_PLAIN_KERNEL void __launch_bounds__(kExpandBlock) k_ray_expand_count(const uint32_t* __restrict__ entries, uint32_t n,
                                                                   unsigned long long* __restrict__ block_counts) {
    __shared__ uint32_t wave_sum[kExpandBlock / 64];
    uint32_t s = expand_counts(expand_load(entries, n, blockIdx.x * kExpandTile + threadIdx.x * kExpandItems));
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kExpandBlock / 64; ++w) t += wave_sum[w];
        block_counts[blockIdx.x] = (unsigned long long)(t & 0xffffu) | ((unsigned long long)(t >> 16) << 32);
        if (blockIdx.x == 0) block_counts[gridDim.x] = 0ull;
    }
}

// block_offsets: the exclusive scan of block_counts over gridDim.x + 1 elements. Tokens are ranked inside the tile (threads in
// entry order), staged in LDS and copied out in whole lines. n_tokens = the queue's length as the host knows it; the sections
// add up to it, and nothing is written past it whatever the entries hold.
PB_PLAIN_KERNEL void __launch_bounds__(kExpandBlock) k_ray_expand_scatter(const uint32_t* __restrict__ entries, uint32_t n,
                                                                     const unsigned long long* __restrict__ block_offsets,
                                                                     uint32_t* __restrict__ tokens, uint32_t n_tokens) {
    __shared__ uint32_t wave_sum[kExpandBlock / 64];
    __shared__ uint32_t stage_c[2 * kExpandTile], stage_a[2 * kExpandTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint4 v = expand_load(entries, n, blockIdx.x * kExpandTile + threadIdx.x * kExpandItems);
    const uint32_t mine = expand_counts(v);
    uint32_t incl = mine;  // inclusive scan over the wave, both halves at once (no carry: a tile's totals fit 16 bits)
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < kExpandBlock / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    const uint32_t excl = before + incl - mine;
    uint32_t c = excl & 0xffffu, a = excl >> 16;
    const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        path_entry_tokens(e[k], &stage_c[c], &stage_a[a]);
        c += path_entry_closest(e[k]);
        a += path_entry_anyhit(e[k]);
    }
    __syncthreads();
    const unsigned long long off = block_offsets[blockIdx.x], totals = block_offsets[gridDim.x];
    const uint32_t base_c = (uint32_t)off, base_a = (uint32_t)totals + (uint32_t)(off >> 32);  // any-hit section: behind all closest-hit tokens
    const uint32_t n_c = total & 0xffffu, n_a = total >> 16;
    for (uint32_t i = threadIdx.x; i < n_c; i += kExpandBlock)
        if (base_c + i < n_tokens) tokens[base_c + i] = stage_c[i];
    for (uint32_t i = threadIdx.x; i < n_a; i += kExpandBlock)
        if (base_a + i < n_tokens) tokens[base_a + i] = stage_a[i];
}
#endif  // __HIPCC__

}  // namespace pb
