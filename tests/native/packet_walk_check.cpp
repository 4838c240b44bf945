// packet_walk_check.cpp — host model of the packet walk of pbrt-rs_amd/csrc/trace_wide_packet.h (test infrastructure, built by
// tests/test_packet_walk_host.py with g++; not part of the product library).
//
// Compiles the product's own builder (host_wide.cpp) and the product's own filter arithmetic (wide_bvh.h: wide_setup,
// wide_child_test, wide_ray_covered — the functions the kernels call) for the host and walks groups of up to 64 rays three ways:
//   R  the reference's loop over the binary tree (BVHAccel::intersect, src/accelerators/bvh.rs:828-879), one ray at a time;
//   W  the per-ray walk over the wide records (trace_wide.h without its scheduling): children ranked by the two dir_is_neg
//      levels, a stack of (reference, entry distance) per ray, the exact slab test at every candidate leaf;
//   P  the packet walk: once per negmask group of the 64 rays, one stack of references for the group, a child visited when ANY
//      lane passes wide_child_test with its own ray and t_max, the exact slab test and the triangle tests per lane at every leaf
//      the group reaches, lanes outside the group inert (t_max < 0).
// Every lane's (slot, t, b0, b1, b2) of P must equal R's and W's bit for bit. Rays the filter's bound does not cover, and rays
// whose t_max moves up by an ulp, leave W and P for the binary walk as they do in the kernels; they are counted, not compared.
// The slab and triangle tests are restated here in the operation order of csrc/trace.h (compiled with -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../pbrt-rs_amd/csrc/host_wide.cpp"

namespace {

constexpr float kMachEps = 5.9604644775390625e-08f;
inline float gamma_n(int n) { return (float)n * kMachEps / (1.0f - (float)n * kMachEps); }
const float kGamma2 = gamma_n(2), kGamma3 = gamma_n(3), kGamma5 = gamma_n(5);
const float kSlabScale = 1.0f + 2.0f * kGamma3;
constexpr int kTriDegenerate = 1 << 30;

struct Ray {
    float o[3], d[3], id[3], tmax;
    int neg[3];
    uint32_t negmask;
};
struct Hit {
    int32_t slot;
    float t, b0, b1, b2;
};

// Bounds3f::intersect_p (geometry.rs:709-751)
bool slab(const float lo[3], const float hi[3], const Ray& r, float tmax_ray) {
    const float* b[2] = {lo, hi};
    float t_min = (b[r.neg[0]][0] - r.o[0]) * r.id[0];
    float t_max = (b[1 - r.neg[0]][0] - r.o[0]) * r.id[0];
    float ty_min = (b[r.neg[1]][1] - r.o[1]) * r.id[1];
    float ty_max = (b[1 - r.neg[1]][1] - r.o[1]) * r.id[1];
    t_max *= kSlabScale;
    ty_max *= kSlabScale;
    if (t_min > ty_max || ty_min > t_max) return false;
    if (ty_min > t_min) t_min = ty_min;
    if (ty_max < t_max) t_max = ty_max;
    float tz_min = (b[r.neg[2]][2] - r.o[2]) * r.id[2];
    float tz_max = (b[1 - r.neg[2]][2] - r.o[2]) * r.id[2];
    tz_max *= kSlabScale;
    if (t_min > tz_max || tz_min > t_max) return false;
    if (tz_min > t_min) t_min = tz_min;
    if (tz_max < t_max) t_max = tz_max;
    return (t_min < tmax_ray) && (t_max > 0.0f);
}

inline float max3(float a, float b, float c) { return std::fmax(a, std::fmax(b, c)); }
// Triangle::intersect_test (triangle.rs:74-158), as csrc/trace.h: triangle_test with tri_ray_setup
bool triangle(const float* v, const Ray& r, float tmax, Hit* h) {
    const float ax = std::fabs(r.d[0]), ay = std::fabs(r.d[1]), az = std::fabs(r.d[2]);
    const int kz = (ax > ay && ax > az) ? 0 : (ay > az ? 1 : 2);
    const int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
    const float sx = -r.d[kx] / r.d[kz], sy = -r.d[ky] / r.d[kz], sz = r.id[kz];
    float p[3][3];
    for (int k = 0; k < 3; ++k) {
        const float t[3] = {v[3 * k] - r.o[0], v[3 * k + 1] - r.o[1], v[3 * k + 2] - r.o[2]};
        p[k][0] = t[kx];
        p[k][1] = t[ky];
        p[k][2] = t[kz];
        p[k][0] += sx * p[k][2];
        p[k][1] += sy * p[k][2];
    }
    const float e0 = (float)((double)p[1][0] * (double)p[2][1] - (double)p[1][1] * (double)p[2][0]);
    const float e1 = (float)((double)p[2][0] * (double)p[0][1] - (double)p[2][1] * (double)p[0][0]);
    const float e2 = (float)((double)p[0][0] * (double)p[1][1] - (double)p[0][1] * (double)p[1][0]);
    if ((e0 < 0.0f || e1 < 0.0f || e2 < 0.0f) && (e0 > 0.0f || e1 > 0.0f || e2 > 0.0f)) return false;
    const float det = e0 + e1 + e2;
    if (det == 0.0f) return false;
    p[0][2] *= sz;
    p[1][2] *= sz;
    p[2][2] *= sz;
    const float t_scaled = e0 * p[0][2] + e1 * p[1][2] + e2 * p[2][2];
    if (det < 0.0f && (t_scaled >= 0.0f || t_scaled < tmax * det)) return false;
    if (det > 0.0f && (t_scaled <= 0.0f || t_scaled > tmax * det)) return false;
    const float inv_det = 1.0f / det;
    const float t = t_scaled * inv_det;
    const float max_zt = max3(std::fabs(p[0][2]), std::fabs(p[1][2]), std::fabs(p[2][2]));
    const float delta_z = kGamma3 * max_zt;
    const float max_xt = max3(std::fabs(p[0][0]), std::fabs(p[1][0]), std::fabs(p[2][0]));
    const float max_yt = max3(std::fabs(p[0][1]), std::fabs(p[1][1]), std::fabs(p[2][1]));
    const float delta_x = kGamma5 * (max_xt + max_zt);
    const float delta_y = kGamma5 * (max_yt + max_zt);
    const float delta_e = 2.0f * (kGamma2 * max_xt * max_yt + delta_y * max_xt + delta_x * max_yt);
    const float max_e = max3(std::fabs(e0), std::fabs(e1), std::fabs(e2));
    const float delta_t = 3.0f * (kGamma3 * max_e * max_zt + delta_e * max_zt + delta_z * max_e) * std::fabs(inv_det);
    if (t <= delta_t) return false;
    h->t = t;
    h->b0 = e0 * inv_det;
    h->b1 = e1 * inv_det;
    h->b2 = e2 * inv_det;
    return true;
}

struct Model {
    const PbrtLinearBVHNode* nodes;
    const float* tris;  // 12 floats per leaf slot
    pb::WideTree wt;
    std::vector<int32_t> leaf_node;  // leaf slot of a leaf's first triangle -> its node

    // R: bvh.rs:828-879
    Hit reference(const Ray& r) const {
        Hit best{-1, 0.0f, 0.0f, 0.0f, 0.0f};
        float tmax = r.tmax;
        int32_t stack[64], sp = 0, cur = 0;
        for (;;) {
            const PbrtLinearBVHNode& nd = nodes[cur];
            if (slab(nd.bounds_min, nd.bounds_max, r, tmax)) {
                if (nd.n_primitives > 0) {
                    for (int i = 0; i < nd.n_primitives; ++i) {
                        const float* tv = tris + 12 * (size_t)(nd.offset + i);
                        Hit h;
                        int32_t flags;
                        std::memcpy(&flags, tv + 11, 4);
                        if (triangle(tv, r, tmax, &h) && !(flags & kTriDegenerate)) {
                            h.slot = nd.offset + i;
                            best = h;
                            tmax = h.t;
                        }
                    }
                    if (sp == 0) break;
                    cur = stack[--sp];
                } else if (r.neg[nd.axis]) {
                    stack[sp++] = cur + 1;
                    cur = nd.offset;
                } else {
                    stack[sp++] = nd.offset;
                    cur = cur + 1;
                }
            } else {
                if (sp == 0) break;
                cur = stack[--sp];
            }
        }
        return best;
    }

    // what both wide walks do at a leaf reference for one ray: the exact box, then the triangles; true: t_max moved UP
    bool leaf(int32_t ref, const Ray& r, float* tmax, Hit* best) const {
        const int v = ~ref, n = (v & 3) + 1, first = v >> 2;
        int32_t slot0;
        std::memcpy(&slot0, &wt.tris[12 * (size_t)first + 9], 4);
        const PbrtLinearBVHNode& lf = nodes[leaf_node[slot0]];
        if (!slab(lf.bounds_min, lf.bounds_max, r, *tmax)) return false;
        bool raised = false;
        for (int i = 0; i < n; ++i) {
            const float* tv = &wt.tris[12 * (size_t)(first + i)];
            Hit h;
            int32_t slot, flags;
            std::memcpy(&slot, tv + 9, 4);
            std::memcpy(&flags, tv + 10, 4);
            if (triangle(tv, r, *tmax, &h) && !(flags & kTriDegenerate)) {
                if (h.t > *tmax) raised = true;
                h.slot = slot;
                *best = h;
                *tmax = h.t;
            }
        }
        return raised;
    }

    struct Rec {
        uint32_t nq[3], fq[3], m[4], sel, child_base, ntb;
        const uint32_t* dw;
    };
    Rec record(int32_t idx, uint32_t negmask) const {
        Rec c;
        const uint32_t* rec = &wt.nodes[(size_t)idx * pb::kWideNodeDwords];
        c.dw = rec;
        for (int k = 0; k < 3; ++k) {
            const bool neg = (negmask >> k) & 1u;
            c.nq[k] = neg ? rec[5 + 2 * k] : rec[4 + 2 * k];
            c.fq[k] = neg ? rec[4 + 2 * k] : rec[5 + 2 * k];
        }
        const uint32_t dw3 = rec[3];
        c.m[0] = rec[0] & 0xffu, c.m[1] = rec[1] & 0xffu, c.m[2] = rec[2] & 0xffu, c.m[3] = dw3 >> 24;
        const uint32_t f_root = (negmask >> ((dw3 >> 18) & 3u)) & 1u, f_c0 = (negmask >> ((dw3 >> 20) & 3u)) & 1u,
                       f_c1 = (negmask >> ((dw3 >> 22) & 3u)) & 1u;
        c.sel = 0x03020100u ^ (f_c0 ? 0x00000101u : 0u) ^ (f_c1 ? 0x01010000u : 0u);
        if (f_root) c.sel = (c.sel >> 16) | (c.sel << 16);
        c.child_base = rec[10];
        c.ntb = rec[11];
        return c;
    }
    static int32_t child_ref(const Rec& c, int s) { return (c.m[s] & 0x80u) ? (int32_t)(c.child_base + (c.m[s] & 3u)) : (int32_t)(c.ntb - c.m[s]); }

    // W: one ray over the wide records. false: the ray leaves the wide walk (t_max moved up)
    bool per_ray(const Ray& r, Hit* out, int64_t* n_rec, int64_t* n_leaf) const {
        Hit best{-1, 0.0f, 0.0f, 0.0f, 0.0f};
        float tmax = r.tmax;
        std::vector<std::pair<int32_t, float>> st;
        int32_t cur = wt.root_ref;
        for (;;) {
            if (cur >= 0) {
                *n_rec += 1;
                const Rec c = record(cur, r.negmask);
                const pb::WideSetup ws = pb::wide_setup(c.dw[0], c.dw[1], c.dw[2], c.dw[3], r.o[0], r.o[1], r.o[2], r.id[0], r.id[1], r.id[2]);
                int32_t next = INT32_MIN;
                float next_e = 0.0f;
                for (int k = 3; k >= 0; --k) {
                    const int s = (c.sel >> (8 * k)) & 3u;
                    float e;
                    if (c.m[s] == 0xffu || !pb::wide_child_test(ws, c.nq[0], c.nq[1], c.nq[2], c.fq[0], c.fq[1], c.fq[2], s, tmax, &e)) continue;
                    if (next != INT32_MIN) st.push_back({next, next_e});
                    next = child_ref(c, s);
                    next_e = e;
                }
                cur = next;
            } else {
                *n_leaf += 1;
                if (leaf(cur, r, &tmax, &best)) return false;
                cur = INT32_MIN;
            }
            while (cur == INT32_MIN) {
                if (st.empty()) {
                    *out = best;
                    return true;
                }
                if (st.back().second < tmax) cur = st.back().first;
                st.pop_back();
            }
        }
    }

    // P: up to 64 rays, one walk per negmask group. special[i]: lane i left the walk. Returns the deepest stack.
    int packet(const Ray* rays, int n, Hit* out, bool* special, int64_t* n_rec, int64_t* n_leaf, int64_t* n_groups) const {
        float tmax[64];
        bool todo[64];
        int deepest = 0;
        for (int i = 0; i < n; ++i) {
            out[i] = Hit{-1, 0.0f, 0.0f, 0.0f, 0.0f};
            tmax[i] = rays[i].tmax;
            todo[i] = !special[i];
        }
        for (;;) {
            int leader = -1;
            for (int i = 0; i < n && leader < 0; ++i)
                if (todo[i]) leader = i;
            if (leader < 0) break;
            *n_groups += 1;
            const uint32_t g = rays[leader].negmask;
            float tm[64];
            for (int i = 0; i < n; ++i) {
                const bool in_group = todo[i] && rays[i].negmask == g;
                tm[i] = in_group ? tmax[i] : -1.0f;
                if (in_group) todo[i] = false;
            }
            std::vector<int32_t> st;
            int32_t cur = wt.root_ref;
            for (;;) {
                if (cur >= 0) {
                    *n_rec += 1;
                    const Rec c = record(cur, g);
                    bool any[4] = {false, false, false, false};
                    for (int i = 0; i < n; ++i) {
                        const Ray& r = rays[i];
                        const pb::WideSetup ws = pb::wide_setup(c.dw[0], c.dw[1], c.dw[2], c.dw[3], r.o[0], r.o[1], r.o[2], r.id[0], r.id[1], r.id[2]);
                        for (int s = 0; s < 4; ++s) {
                            float e;
                            if (pb::wide_child_test(ws, c.nq[0], c.nq[1], c.nq[2], c.fq[0], c.fq[1], c.fq[2], s, tm[i], &e)) any[s] = true;
                        }
                    }
                    int32_t next = INT32_MIN;
                    for (int k = 3; k >= 0; --k) {
                        const int s = (c.sel >> (8 * k)) & 3u;
                        if (c.m[s] == 0xffu || !any[s]) continue;
                        if (next != INT32_MIN) st.push_back(next);
                        next = child_ref(c, s);
                    }
                    if ((int)st.size() > deepest) deepest = (int)st.size();
                    cur = next;
                } else {
                    *n_leaf += 1;
                    for (int i = 0; i < n; ++i) {
                        if (!(tm[i] >= 0.0f)) continue;
                        if (leaf(cur, rays[i], &tm[i], &out[i])) {
                            special[i] = true;
                            tm[i] = -1.0f;
                        }
                    }
                    cur = INT32_MIN;
                }
                if (cur == INT32_MIN) {
                    if (st.empty()) break;
                    cur = st.back();
                    st.pop_back();
                }
            }
            for (int i = 0; i < n; ++i)
                if (rays[i].negmask == g && tm[i] >= 0.0f) tmax[i] = tm[i];
        }
        return deepest;
    }
};

bool same(const Hit& a, const Hit& b) {
    if (a.slot != b.slot) return false;
    if (a.slot < 0) return true;
    return std::memcmp(&a.t, &b.t, 16) == 0;
}

}  // namespace

// rays = n x {o.xyz, d.xyz, t_max}, walked in groups of `group` (<= 64) consecutive rays. Returns the number of lanes whose
// packet or per-ray result differs from the reference's (-100: the builder declined). counts: {lanes compared, lanes left to
// the binary walk, packet record steps, packet leaf visits, per-ray record steps (sum over the compared lanes), per-ray leaf
// visits, negmask groups walked, groups of rays, deepest packet stack, the builder's stack_need, lanes whose packet result differs,
// lanes whose per-ray result differs}.
extern "C" int64_t packet_walk_check(const PbrtLinearBVHNode* nodes, int32_t n_nodes, const float* tris, int32_t n_slots, const float* rays,
                                     int32_t n_rays, int32_t group, int64_t* counts) {
    if (group < 1 || group > 64) return -1;
    Model m;
    m.nodes = nodes;
    m.tris = tris;
    if (pb::build_wide_tree(nodes, n_nodes, tris, n_slots, &m.wt)) return -100;
    m.leaf_node.assign(n_slots, -1);
    for (int32_t i = 0; i < n_nodes; ++i)
        if (nodes[i].n_primitives > 0) m.leaf_node[nodes[i].offset] = i;
    int64_t bad = 0;
    counts[9] = m.wt.stack_need;
    for (int32_t g0 = 0; g0 < n_rays; g0 += group) {
        const int n = std::min(group, n_rays - g0);
        Ray r[64];
        Hit hp[64];
        bool special[64];
        for (int i = 0; i < n; ++i) {
            const float* ry = rays + 7 * (size_t)(g0 + i);
            r[i].negmask = 0;
            for (int k = 0; k < 3; ++k) {
                r[i].o[k] = ry[k];
                r[i].d[k] = ry[3 + k];
                r[i].id[k] = 1.0f / ry[3 + k];
                r[i].neg[k] = r[i].id[k] < 0.0f;
                r[i].negmask |= (uint32_t)r[i].neg[k] << k;
            }
            r[i].tmax = ry[6];
            // an uncovered ray, or the placeholder of a path outside pixel_bounds (t_max < 0): not walked
            special[i] = !pb::wide_ray_covered(r[i].o[0], r[i].o[1], r[i].o[2], r[i].id[0], r[i].id[1], r[i].id[2]) || r[i].tmax < 0.0f;
        }
        const int deepest = m.packet(r, n, hp, special, &counts[2], &counts[3], &counts[6]);
        if (deepest > counts[8]) counts[8] = deepest;
        counts[7] += 1;
        for (int i = 0; i < n; ++i) {
            if (special[i]) {
                counts[1] += 1;
                continue;
            }
            Hit hw;
            int64_t nr = 0, nl = 0;
            if (!m.per_ray(r[i], &hw, &nr, &nl)) {  // t_max moved up on the ray's own walk only: the packet result must still be the reference's
                hw = m.reference(r[i]);
            } else {
                counts[4] += nr;
                counts[5] += nl;
            }
            counts[0] += 1;
            const Hit hr = m.reference(r[i]);
            if (!same(hp[i], hr)) counts[10] += 1;
            if (!same(hw, hr)) counts[11] += 1;
            if (!same(hp[i], hr) || !same(hw, hr)) ++bad;
        }
    }
    return bad;
}
