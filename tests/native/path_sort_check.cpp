// path_sort_check.cpp — host-side checker of the ray queue's one-entry-per-path packing and of its expansion into the trace
// queue (test infrastructure, built by tests/test_path_sort_host.py with g++; not part of the product library).
//
// Compiles the product's own packing and section arithmetic (pbrt-rs_amd/csrc/wf_ray_expand.h: the functions k_shade and the
// expansion kernels call) for the host.
#include <cstdint>
#include <vector>

#include "../../pbrt-rs_amd/csrc/wf_ray_expand.h"

extern "C" {

// pack -> unpack for every flag set at the given record; 0 when all sixteen come back as they went in, else 1 + the flag set
int path_sort_roundtrip(uint32_t rec) {
    for (uint32_t f = 0; f < 16; ++f) {
        const bool cont = f & 1, mis = f & 2, shadow = f & 4, mis_bool = f & 8;
        const uint32_t v = pb::path_entry_pack(rec, cont, mis, shadow, mis_bool);
        if (pb::path_entry_rec(v) != rec) return 1 + (int)f;
        if (((v & pb::PE_CONT) != 0) != cont || ((v & pb::PE_MIS) != 0) != mis || ((v & pb::PE_SHADOW) != 0) != shadow ||
            ((v & pb::PE_MIS_BOOL) != 0) != mis_bool)
            return 1 + (int)f;
        if ((v & 15u) != f) return 1 + (int)f;
        // the sections: a boolean MIS ray is an any-hit ray, any other MIS ray a closest-hit ray
        if (pb::path_entry_closest(v) != (uint32_t)cont + (uint32_t)(mis && !mis_bool)) return 1 + (int)f;
        if (pb::path_entry_anyhit(v) != (uint32_t)shadow + (uint32_t)(mis && mis_bool)) return 1 + (int)f;
    }
    return 0;
}

int path_sort_rec_bits() { return pb::kPathRecBits; }

uint32_t path_sort_pack(uint32_t rec, int cont, int mis, int shadow, int mis_bool) {
    return pb::path_entry_pack(rec, cont != 0, mis != 0, shadow != 0, mis_bool != 0);
}

// The expansion, entry after entry: tokens[0, *n_closest) then tokens[*n_closest, return value). `tokens` has room for
// 3 n values.
uint32_t path_sort_expand(const uint32_t* entries, uint32_t n, uint32_t* tokens, uint32_t* n_closest) {
    std::vector<uint32_t> closest, anyhit;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c[2], a[2];
        pb::path_entry_tokens(entries[i], c, a);
        for (uint32_t k = 0; k < pb::path_entry_closest(entries[i]); ++k) closest.push_back(c[k]);
        for (uint32_t k = 0; k < pb::path_entry_anyhit(entries[i]); ++k) anyhit.push_back(a[k]);
    }
    uint32_t o = 0;
    for (uint32_t t : closest) tokens[o++] = t;
    for (uint32_t t : anyhit) tokens[o++] = t;
    *n_closest = (uint32_t)closest.size();
    return o;
}

// The same by the kernels' plan: counts per tile of kExpandTile entries (closest | any-hit << 32), an exclusive scan over
// the tiles with the totals behind it, then every tile writes at its own offsets.
uint32_t path_sort_expand_tiled(const uint32_t* entries, uint32_t n, uint32_t* tokens, uint32_t* n_closest) {
    const uint32_t blocks = pb::ray_expand_blocks(n);
    std::vector<unsigned long long> counts(blocks + 1, 0ull), offsets(blocks + 1, 0ull);
    for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t i = b * pb::kExpandTile; i < n && i < (b + 1) * pb::kExpandTile; ++i)
            counts[b] += (unsigned long long)pb::path_entry_closest(entries[i]) | ((unsigned long long)pb::path_entry_anyhit(entries[i]) << 32);
    for (uint32_t b = 0; b < blocks; ++b) offsets[b + 1] = offsets[b] + counts[b];
    const uint32_t total_c = (uint32_t)offsets[blocks], total_a = (uint32_t)(offsets[blocks] >> 32);
    for (uint32_t b = 0; b < blocks; ++b) {
        uint32_t c = (uint32_t)offsets[b], a = total_c + (uint32_t)(offsets[b] >> 32);
        for (uint32_t i = b * pb::kExpandTile; i < n && i < (b + 1) * pb::kExpandTile; ++i) {
            uint32_t tc[2], ta[2];
            pb::path_entry_tokens(entries[i], tc, ta);
            for (uint32_t k = 0; k < pb::path_entry_closest(entries[i]); ++k) tokens[c++] = tc[k];
            for (uint32_t k = 0; k < pb::path_entry_anyhit(entries[i]); ++k) tokens[a++] = ta[k];
        }
    }
    *n_closest = total_c;
    return total_c + total_a;
}

}  // extern "C"
