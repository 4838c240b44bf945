// host_scene.cpp — scene creation on the host (host_scene.h): the checks of a scene description and the tables it puts
// on the device. No device call: tests/native/scene_plan_check.cpp runs all of it on a CPU.
#include "host_scene.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "host_envmap.h"
#include "host_lobes.h"
#include "host_motion.h"
#include "host_wide.h"

namespace pb {

bool mesh_indices_in_range(const int32_t* indices, int64_t n_tris, int32_t n_verts) {
    for (int64_t i = 0; i < 3 * n_tris; ++i)
        if (indices[i] < 0 || indices[i] >= n_verts) return false;
    return true;
}

float tri_area(const float* a, const float* b, const float* c) {
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

void make_distribution(const std::vector<float>& f, std::vector<float>* cdf, float* func_int) {
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

static int bits_for_count(int max_count) {
    int bits = 0;
    while ((1 << bits) < max_count) ++bits;
    return bits;
}

const char* tree_invalid(const PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t n_prims, int force_count_bits,
                         int64_t n_slots_total, int* depth_out) {
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
            ++n_interior;
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
        if (depth_out) *depth_out = max_depth;
    }
    if (n_interior != (n_nodes - 1) / 2 || (n_nodes & 1) == 0) return "node array is not a full binary tree";
    int count_bits = bits_for_count(max_count);
    if (force_count_bits >= 0) {
        if (force_count_bits < count_bits) return "leaf larger than the shared leaf-reference width";
        count_bits = force_count_bits;
    }
    if (((n_slots_total >= 0 ? n_slots_total : (int64_t)n_prims) << count_bits) >= (1ll << 31)) return "scene too large for 31-bit leaf references";
    return nullptr;
}

TreeLayout convert_tree(const PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t base, std::vector<float>* inodes,
                        int32_t slot_base, int force_count_bits) {
    std::vector<int32_t> interior_index(n_nodes, -1);
    int n_interior = 0, max_count = 1;
    for (int32_t i = 0; i < n_nodes; ++i) {
        if (nodes[i].n_primitives > 0) max_count = std::max<int>(max_count, nodes[i].n_primitives);
        else interior_index[i] = n_interior++;
    }
    const int count_bits = force_count_bits >= 0 ? force_count_bits : bits_for_count(max_count);
    auto child_ref = [&](int32_t node) -> int32_t {
        const PbrtLinearBVHNode& nd = nodes[node];
        if (nd.n_primitives > 0)
            return ~(int32_t)(((uint32_t)(nd.offset + slot_base) << count_bits) | (uint32_t)(nd.n_primitives - 1));
        return base + interior_index[node];
    };
    const size_t first = inodes->size();
    inodes->resize(first + (size_t)n_interior * 16, 0.0f);
    std::vector<int32_t> parent_record(n_nodes, -1);  // of interior nodes: the record holding them as a child (trace_stackless.h)
    for (int32_t i = 0; i < n_nodes; ++i) {
        if (interior_index[i] < 0) continue;
        parent_record[i + 1] = parent_record[nodes[i].offset] = base + interior_index[i];
    }
    for (int32_t i = 0; i < n_nodes; ++i) {
        if (interior_index[i] < 0) continue;
        const PbrtLinearBVHNode& c0 = nodes[i + 1];
        const PbrtLinearBVHNode& c1 = nodes[nodes[i].offset];
        float* r = &(*inodes)[first + (size_t)interior_index[i] * 16];
        r[0] = c0.bounds_min[0]; r[1] = c0.bounds_min[1]; r[2] = c0.bounds_min[2];
        r[3] = c0.bounds_max[0]; r[4] = c0.bounds_max[1]; r[5] = c0.bounds_max[2];
        r[6] = c1.bounds_min[0]; r[7] = c1.bounds_min[1]; r[8] = c1.bounds_min[2];
        r[9] = c1.bounds_max[0]; r[10] = c1.bounds_max[1]; r[11] = c1.bounds_max[2];
        int32_t refs[4] = {child_ref(i + 1), child_ref(nodes[i].offset), (int32_t)nodes[i].axis, parent_record[i]};
        std::memcpy(r + 12, refs, 16);
    }
    TreeLayout out;
    out.n_interior = n_interior;
    out.count_bits = count_bits;
    out.root_ref = child_ref(0);
    return out;
}

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
static DevShape shape_row(const PbrtShape& sh) {
    DevShape d;
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
    d.flags = sh.type | ((reverse != (det < 0.0f)) ? kShapeFlipNormal : 0);
    return d;
}

// ---- PbrtCurve (curve.rs:29-80: CurveCommon::new, Curve::new) ----
static const char* curve_invalid(const PbrtCurve& c, int32_t n_materials) {
    if (c.type < PBRT_CURVE_FLAT || c.type > PBRT_CURVE_RIBBON) return "unknown curve type";
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(c.cp[k / 3][k % 3])) return "curve control points must be finite";
    if (!(c.width0 >= 0.0f) || !(c.width1 >= 0.0f) || !std::isfinite(c.width0) || !std::isfinite(c.width1))
        return "curve widths must be finite and not negative";
    if (c.width0 == 0.0f && c.width1 == 0.0f) return "curve widths must not both be zero";
    if (!(c.u_min >= 0.0f && c.u_max <= 1.0f && c.u_min < c.u_max)) return "curve u range must satisfy 0 <= u_min < u_max <= 1";
    if (c.type == PBRT_CURVE_RIBBON) {
        double l0 = 0.0, l1 = 0.0, d = 0.0, cr[3];
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(c.n0[k]) || !std::isfinite(c.n1[k])) return "ribbon normals must be finite";
            l0 += (double)c.n0[k] * c.n0[k];
            l1 += (double)c.n1[k] * c.n1[k];
            d += (double)c.n0[k] * c.n1[k];
        }
        if (l0 == 0.0 || l1 == 0.0) return "ribbon normals must not be zero";
        for (int k = 0; k < 3; ++k) cr[k] = (double)c.n0[(k + 1) % 3] * c.n1[(k + 2) % 3] - (double)c.n0[(k + 2) % 3] * c.n1[(k + 1) % 3];
        if (d < 0.0 && cr[0] == 0.0 && cr[1] == 0.0 && cr[2] == 0.0) return "ribbon normals must not be opposite (n0 == -n1)";
    }
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(c.to_world[k]) || !std::isfinite(c.to_object[k])) return "curve transforms must be finite";
    if (c.to_world[12] != 0.0f || c.to_world[13] != 0.0f || c.to_world[14] != 0.0f || c.to_world[15] != 1.0f ||
        c.to_object[12] != 0.0f || c.to_object[13] != 0.0f || c.to_object[14] != 0.0f || c.to_object[15] != 1.0f)
        return "curve transforms must be affine (last row 0 0 0 1)";
    if (c.material < 0 || c.material >= n_materials) return "curve material out of range";
    return nullptr;
}
static DevCurve curve_row(const PbrtCurve& c) {
    DevCurve d;
    std::memcpy(d.w2o, c.to_object, 48);
    std::memcpy(d.o2w, c.to_world, 48);
    std::memcpy(d.cp, c.cp, 48);
    d.width0 = c.width0;
    d.width1 = c.width1;
    d.u_min = c.u_min;
    d.u_max = c.u_max;
    for (int k = 0; k < 3; ++k) d.n0[k] = d.n1[k] = 0.0f;
    d.normal_angle = d.inv_sin_normal_angle = 0.0f;
    if (c.type == PBRT_CURVE_RIBBON) {
        // CurveCommon::new after pbrt-v3: the normals normalised, normal_angle = acos(clamp(n0 . n1, 0, 1)) (D103)
        double l0 = 0.0, l1 = 0.0, dt = 0.0;
        for (int k = 0; k < 3; ++k) {
            l0 += (double)c.n0[k] * c.n0[k];
            l1 += (double)c.n1[k] * c.n1[k];
        }
        for (int k = 0; k < 3; ++k) {
            d.n0[k] = (float)(c.n0[k] / std::sqrt(l0));
            d.n1[k] = (float)(c.n1[k] / std::sqrt(l1));
            dt += (double)d.n0[k] * d.n1[k];
        }
        const double angle = std::acos(dt < 0.0 ? 0.0 : (dt > 1.0 ? 1.0 : dt));
        const bool same = d.n0[0] == d.n1[0] && d.n0[1] == d.n1[1] && d.n0[2] == d.n1[2];
        if (!same && (float)angle != 0.0f) {
            d.normal_angle = (float)angle;
            d.inv_sin_normal_angle = (float)(1.0 / std::sin(angle));
        }
    }
    const float* m = c.to_world;
    const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    d.flags = c.type | (((c.reverse_orientation != 0) != (det < 0.0f)) ? kCurveFlipNormal : 0);
    return d;
}

static bool is_permutation(const int32_t* order, int32_t n) {  // of entries already known to lie in [0, n)
    std::vector<char> seen(n, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (seen[order[i]]) return false;
        seen[order[i]] = 1;
    }
    return true;
}

// the leaf-reference width the object trees of a two-level scene share
static int shared_count_bits(const InstancingArgs& ia) {
    int max_count = 1;
    for (int32_t k = 0; k < ia.n_objects; ++k)
        for (int32_t i = 0; i < ia.objects[k].n_nodes; ++i) max_count = std::max<int>(max_count, ia.objects[k].nodes[i].n_primitives);
    return bits_for_count(max_count);
}

// The checks of a two-level scene's instances, motions and trees; *depth: the two levels' depths together.
static std::string instancing_invalid(const SceneDesc& desc, int* depth) {
    const InstancingArgs& ia = desc.ia;
    const int32_t n_top = desc.n_top();
    for (int32_t i = 0; i < n_top; ++i)
        if (ia.tlas_order[i] < 0 || ia.tlas_order[i] >= n_top) return "tlas_order entry out of range";
    for (int32_t i = 0; i < ia.n_instances; ++i) {
        const float* m = ia.instances[i].to_world;
        const float* mi = ia.instances[i].to_object;
        if (m[12] != 0.0f || m[13] != 0.0f || m[14] != 0.0f || m[15] != 1.0f || mi[12] != 0.0f || mi[13] != 0.0f ||
            mi[14] != 0.0f || mi[15] != 1.0f)
            return "instance transforms must be affine (last row 0 0 0 1)";
        if (ia.instances[i].material >= desc.n_materials) return "instance material out of range";
    }
    int top_depth = 0, deepest = 0;
    if (const char* e = tree_invalid(ia.tlas_nodes, ia.n_tlas_nodes, n_top, -1, -1, &top_depth)) return e;
    if (ia.motions) {
        // moving instances (host_motion.cpp); the limits of their one general shading build per integrator family: DESIGN.md D96
        for (int32_t i = 0; i < desc.n_lights; ++i)
            if (desc.lights[i].type == PBRT_LIGHT_PROJECTION || desc.lights[i].type == PBRT_LIGHT_GONIOMETRIC)
                return "scenes with moving instances take no projection or goniometric light";
        for (int32_t i = 0; i < ia.n_instances; ++i) {
            DevMotion row;
            if (const char* why = motion_row(ia.instances[i], ia.motions[i], &row)) return "moving instance " + std::to_string(i) + ": " + why;
        }
        // The caller built the top-level tree; one built over the static bounds would silently drop hits: every
        // instance's motion bound must lie inside the leaf box that holds it.
        for (int32_t nd = 0; nd < ia.n_tlas_nodes; ++nd) {
            const PbrtLinearBVHNode& leaf = ia.tlas_nodes[nd];
            for (int32_t k = 0; k < (int32_t)leaf.n_primitives; ++k) {
                const int32_t slot = leaf.offset + k;
                if (slot < 0 || slot >= n_top) return "top-level leaf slot out of range";
                const int32_t id = ia.tlas_order[slot];
                if (id >= ia.n_instances) continue;
                const PbrtLinearBVHNode& root = ia.objects[ia.instance_object ? ia.instance_object[id] : 0].nodes[0];
                float lo[3], hi[3];
                if (pbrt_hip_instance_motion_bounds(root.bounds_min, root.bounds_max, ia.instances + id, ia.motions + id, 1, lo, hi) != PBRT_HIP_OK)
                    return "moving instance: no motion bound";
                for (int c = 0; c < 3; ++c)
                    if (!(lo[c] >= leaf.bounds_min[c] && hi[c] <= leaf.bounds_max[c]))
                        return "instance " + std::to_string(id) + ": its motion bound (pbrt_hip_instance_motion_bounds) leaves the top-level "
                               "leaf box that holds it; build the top-level tree over the motion bounds";
            }
        }
    }
    // the object-level trees: one leaf-reference width for all of them
    const int bits = shared_count_bits(ia);
    for (int32_t k = 0; k < ia.n_objects; ++k) {
        const PbrtObject& o = ia.objects[k];
        int d = 0;
        if (const char* e = tree_invalid(o.nodes, o.n_nodes, o.n_tris, bits, desc.n_tris, &d)) return e;
        deepest = std::max(deepest, d);
    }
    *depth = top_depth + deepest;
    return std::string();
}

const char* combine_two_level(const TwoLevelArgs& a, CombinedMesh* out) {
    const int32_t n_objects = a.n_objects, n_world_tris = a.n_world_tris, n_world_verts = a.n_world_verts;
    if (!a.objects || n_objects <= 0 || !a.instances || a.n_instances <= 0 || !a.tlas_nodes || a.n_tlas_nodes <= 0 || !a.tlas_order)
        return "two-level scene needs objects, instances and a top-level node array";
    if (n_world_tris < 0 || n_world_verts < 0 || (n_world_tris > 0 && (!a.world_positions || !a.world_indices || n_world_verts <= 0)))
        return "bad world-space triangle arguments";
    // ---- the combined mesh: object after object, then the world-space triangles ----
    InstancingArgs& ia = out->ia;
    ia = InstancingArgs{a.instances, a.n_instances, a.tlas_nodes, a.n_tlas_nodes, a.tlas_order, a.objects, n_objects, a.instance_object, a.motions,
                        std::vector<int32_t>(n_objects + 1, 0), n_world_tris, 0};
    int64_t n_verts = 0, n_tris = 0, n_nodes = 0;
    for (int32_t k = 0; k < n_objects; ++k) {
        const PbrtObject& o = a.objects[k];
        if (!o.positions || !o.indices || !o.nodes || !o.prim_order || o.n_verts <= 0 || o.n_tris <= 0 || o.n_nodes <= 0)
            return "object aggregate with a null pointer or an empty mesh / tree";
        if (!mesh_indices_in_range(o.indices, o.n_tris, o.n_verts)) return "object vertex index out of range";
        for (int32_t i = 0; i < o.n_tris; ++i)
            if (o.prim_order[i] < 0 || o.prim_order[i] >= o.n_tris) return "object prim_order entry out of range";
        n_verts += o.n_verts;
        n_tris += o.n_tris;
        n_nodes += o.n_nodes;
        ia.obj_tri_offset[k + 1] = (int32_t)n_tris;
    }
    ia.world_tri_offset = (int32_t)n_tris;
    if (!mesh_indices_in_range(a.world_indices, n_world_tris, n_world_verts)) return "world triangle vertex index out of range";
    n_verts += n_world_verts;
    n_tris += n_world_tris;
    if (n_tris >= (1ll << 30) || n_verts >= (1ll << 31)) return "two-level scene too large";
    for (int32_t i = 0; i < a.n_instances; ++i)
        if (a.instance_object && (a.instance_object[i] < 0 || a.instance_object[i] >= n_objects)) return "instance_object out of range";
    for (int32_t i = 0; i < a.n_lights; ++i)
        if (a.lights[i].type == PBRT_LIGHT_DIFFUSE_AREA && (a.lights[i].prim < 0 || a.lights[i].prim >= n_world_tris))
            return "area lights sit on world-space triangles (instanced primitives cannot be area lights): prim out of range";
    out->n_nodes = (int32_t)n_nodes;
    std::vector<float>& pos = out->pos;
    std::vector<int32_t>&idx = out->idx, &mat = out->mat, &lgt = out->lgt, &order = out->order;
    pos.assign((size_t)n_verts * 3, 0.0f);
    idx.assign((size_t)n_tris * 3, 0);
    mat.assign((size_t)n_tris, 0);
    lgt.assign((size_t)n_tris, -1);
    order.assign((size_t)n_tris, 0);
    // the world-space triangles are one more mesh, in caller order, and the only one whose triangles can be lights
    const PbrtObject world{a.world_positions, n_world_verts, a.world_indices, n_world_tris, a.world_tri_material, nullptr, 0, nullptr};
    int64_t v0 = 0, t0 = 0;
    for (int32_t k = 0; k <= n_objects; ++k) {
        const PbrtObject& o = k < n_objects ? a.objects[k] : world;
        if (o.n_tris <= 0) continue;
        std::memcpy(&pos[(size_t)v0 * 3], o.positions, (size_t)o.n_verts * 12);
        for (int64_t i = 0; i < 3 * (int64_t)o.n_tris; ++i) idx[(size_t)t0 * 3 + i] = o.indices[i] + (int32_t)v0;
        for (int32_t i = 0; i < o.n_tris; ++i) {
            mat[(size_t)t0 + i] = o.tri_material ? o.tri_material[i] : 0;
            if (k == n_objects && a.world_tri_light) lgt[(size_t)t0 + i] = a.world_tri_light[i];
            order[(size_t)t0 + i] = (o.prim_order ? o.prim_order[i] : i) + (int32_t)t0;
        }
        v0 += o.n_verts;
        t0 += o.n_tris;
    }
    return nullptr;
}

std::string scene_invalid(const SceneDesc& desc) {
    const SphereArgs& sa = desc.sa;
    const InstancingArgs& ia = desc.ia;
    const int32_t n_tris = desc.n_tris, n_verts = desc.n_verts, n_materials = desc.n_materials, n_lights = desc.n_lights;
    const PbrtLight* lights = desc.lights;
    const bool dt = desc.device_tree;  // nodes / prim_order are then unused, and the device builder makes a tree of any mesh
    if (n_tris <= 0 || n_verts <= 0 || (!dt && desc.n_nodes <= 0)) return "empty scene: n_tris, n_verts and n_nodes must be > 0";
    if (!desc.positions || !desc.indices || (!dt && ((!desc.nodes && ia.n_instances == 0) || !desc.prim_order))) return "null geometry / BVH pointer";
    if (n_materials <= 0 || !desc.materials) return "at least one material is required";
    if (n_lights < 0 || (n_lights > 0 && !lights)) return "bad light table";
    if (!mesh_indices_in_range(desc.indices, n_tris, n_verts)) return "vertex index out of range";
    const int32_t n_prims = desc.n_prims();
    if (sa.n < 0 || (sa.n > 0 && (!sa.spheres || dt || ia.n_instances > 0))) return "bad sphere arguments";
    for (int32_t i = 0; i < sa.n; ++i) {
        if (!(sa.spheres[4 * i + 3] > 0.0f)) return "sphere radius must be positive";
        if (sa.material && (sa.material[i] < 0 || sa.material[i] >= n_materials)) return "sphere material out of range";
        if (sa.light && (sa.light[i] < -1 || sa.light[i] >= n_lights)) return "sphere light out of range";
    }
    if (sa.n_shapes < 0 || (sa.n_shapes > 0 && (!sa.shapes || sa.n > 0 || dt || ia.n_instances > 0))) return "bad shape arguments";
    for (int32_t i = 0; i < sa.n_shapes; ++i) {
        if (const char* why = shape_invalid(sa.shapes[i], n_materials, n_lights)) return why;
    }
    if (desc.n_curves < 0 || (desc.n_curves > 0 && (!desc.curves || sa.n > 0 || dt || ia.n_instances > 0))) return "bad curve arguments";
    for (int32_t i = 0; i < desc.n_curves; ++i) {
        if (const char* why = curve_invalid(desc.curves[i], n_materials)) return why;
    }
    for (int32_t i = 0; i < n_prims && !dt; ++i)
        if (desc.prim_order[i] < 0 || desc.prim_order[i] >= n_prims) return "prim_order entry out of range";
    for (int32_t i = 0; i < n_tris; ++i) {
        if (desc.tri_material && (desc.tri_material[i] < 0 || desc.tri_material[i] >= n_materials)) return "tri_material out of range";
        if (desc.tri_light && (desc.tri_light[i] < -1 || desc.tri_light[i] >= n_lights)) return "tri_light out of range";
    }
    for (int32_t i = 0; i < n_materials; ++i) {
        if (const char* why = material_invalid(desc.materials[i])) return why;
    }
    for (int32_t i = 0; i < n_lights; ++i) {
        if (lights[i].type < PBRT_LIGHT_DIFFUSE_AREA || lights[i].type > PBRT_LIGHT_GONIOMETRIC) return "unknown light type";
        if (lights[i].type == PBRT_LIGHT_PROJECTION || lights[i].type == PBRT_LIGHT_GONIOMETRIC) {
            const PbrtLight& l = lights[i];
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(l.pos[k]) || !std::isfinite(l.L[k])) return "projection / goniometric light: pos and L must be finite";
            for (int k = 0; k < 9; ++k)
                if (!std::isfinite(l.world_to_light[k])) return "projection / goniometric light: world_to_light must be finite";
            if (l.type == PBRT_LIGHT_PROJECTION && !(std::isfinite(l.fov) && l.fov > 0.0f && l.fov < 180.0f))
                return "projection light: fov must be finite and in (0, 180)";
        }
        if (lights[i].type == PBRT_LIGHT_DIFFUSE_AREA &&
            (lights[i].prim < 0 || lights[i].prim >= (ia.n_instances > 0 ? ia.n_world_tris : n_prims)))
            return "area light primitive out of range";
        if (lights[i].type == PBRT_LIGHT_DIFFUSE_AREA && desc.n_curves > 0 && lights[i].prim >= n_prims - desc.n_curves)
            return "a curve cannot carry an area light (Curve::sample is unimplemented)";
    }
    // ---- the tree(s): single level, one tree over the primitives; two levels (instancing), the top-level tree over the
    // instances and the world-space triangles, then the object-level trees over the triangles ----
    int depth = 0;
    if (desc.instanced()) {
        std::string why = instancing_invalid(desc, &depth);
        if (!why.empty()) return why;
    } else if (!dt) {
        if (const char* e = tree_invalid(desc.nodes, desc.n_nodes, n_prims, -1, -1, &depth)) return e;
    }
    if (depth > 64) return "BVH deeper than the 64-entry traversal stack (bvh.rs:839)";
    if (!dt && !is_permutation(desc.prim_order, n_prims)) return "prim_order is not a permutation";
    if (desc.instanced() && !is_permutation(ia.tlas_order, desc.n_top())) return "tlas_order is not a permutation";
    return std::string();
}

// ---- triangles, spheres and shapes in leaf order (48 B) ----
static void plan_prim_records(const SceneDesc& desc, ScenePlan* plan) {
    const SphereArgs& sa = desc.sa;
    const int32_t n_prims = desc.n_prims(), n_tris = desc.n_tris;
    std::vector<float>& tris = plan->tris;
    tris.resize((size_t)n_prims * 12);
    plan->prim_slot.assign(n_prims, -1);
    for (int32_t slot = 0; slot < n_prims; ++slot) {
        int32_t prim = desc.prim_order[slot];
        plan->prim_slot[prim] = slot;
        if (prim >= n_tris + sa.n_shapes && desc.n_curves > 0) {  // curve record: - | - | (~row of DevSceneData::curves, prim, material, kPrimSphere)
            const int32_t row = prim - n_tris - sa.n_shapes;
            float* t = &tris[(size_t)slot * 12];
            for (int k = 0; k < 8; ++k) t[k] = 0.0f;
            int32_t meta[4] = {~row, prim, desc.curves[row].material, kPrimSphere};
            std::memcpy(t + 8, meta, 16);
            continue;
        }
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
        const float* a = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim];
        const float* b = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim + 1];
        const float* c = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim + 2];
        float* t = &tris[(size_t)slot * 12];
        t[0] = a[0]; t[1] = a[1]; t[2] = a[2];
        t[3] = b[0]; t[4] = b[1]; t[5] = b[2];
        t[6] = c[0]; t[7] = c[1]; t[8] = c[2];
        int32_t meta[3];
        meta[0] = prim;
        meta[1] = desc.tri_material ? desc.tri_material[prim] : 0;
        meta[2] = (desc.tri_light ? desc.tri_light[prim] + 1 : 0) | (triangle_rejected_by_intersect(a, b, c) ? kTriDegenerate : 0);
        std::memcpy(t + 9, meta, 12);
    }
}

// ---- the light rows with area, scale and power, the infinite lights' list, the map lights' host rows ----
static void plan_lights(const SceneDesc& desc, ScenePlan* plan) {
    const SphereArgs& sa = desc.sa;
    const int32_t n_lights = desc.n_lights, n_tris = desc.n_tris;
    const PbrtLight* lights = desc.lights;
    const float world_radius = plan->d.world_radius;
    plan->lights.resize(std::max(1, n_lights));
    plan->power_func.resize(n_lights);
    for (int32_t i = 0; i < n_lights; ++i) {
        DevLight& l = plan->lights[i];
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
            int32_t prim = lights[i].prim + (desc.instanced() ? desc.ia.world_tri_offset : 0);  // two-level: prim counts the world-space triangles
            l.slot = desc.dt ? desc.dt->light_slot[i] : plan->prim_slot[prim];
            if (prim >= n_tris && sa.n_shapes > 0) {
                l.area = shape_area(sa.shapes[prim - n_tris]);
            } else if (prim >= n_tris) {
                float r = sa.spheres[4 * (size_t)(prim - n_tris) + 3];
                l.area = (360.0f * (kPi / 180.0f)) * r * (r - (-r));  // Sphere::area (sphere.rs:99-101)
            } else {
                const float* a = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim];
                const float* b = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim + 1];
                const float* c = desc.positions + 3 * (size_t)desc.indices[3 * (size_t)prim + 2];
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
            plan->light_maps = true;
            if (plan->light_map_rows.empty()) {
                plan->light_map_rows.assign(n_lights, DevLightMap{});
                plan->light_fov.assign(n_lights, 0.0f);
            }
            plan->light_fov[i] = lights[i].fov;
            DevLightMap& m = plan->light_map_rows[i];
            const double cos_total_width = light_map_geometry(l.type, lights[i].fov, 0, 0, m.screen_bounds, &m.inv_tan);
            l.cos_total_width = (float)cos_total_width;
            scale = l.type == PBRT_LIGHT_GONIOMETRIC ? 4.0f * kPi : (float)(2.0 * 3.14159265358979323846 * (1.0 - cos_total_width));
        } else {
            plan->infinite_ids.push_back(i);
            scale = kPi * world_radius * world_radius;  // infinite.rs:131-133
        }
        float p[3] = {l.L[0] * scale, l.L[1] * scale, l.L[2] * scale};
        l.power_y = 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2];  // spectrum.rs:679-682
        plan->power_func[i] = l.power_y;
    }
    plan->light_samples.resize(n_lights);
    for (int32_t i = 0; i < n_lights; ++i) {
        const bool map_light = lights[i].type == PBRT_LIGHT_PROJECTION || lights[i].type == PBRT_LIGHT_GONIOMETRIC;
        plan->light_samples[i] = map_light ? 1 : std::max(1, lights[i].n_samples);
    }
}

// ---- the environment's 2x2 table and the two light sampling distributions ----
static void plan_distributions(const SceneDesc& desc, ScenePlan* plan) {
    DevSceneData& d = plan->d;
    // InfiniteAreaLight's Distribution2D over a 2x2 sin-weighted image of the constant map
    // (infinite.rs:59-73); all infinite lights here are constant so one table per light would be
    // identical up to the luminance scale -- built for the first infinite light, rescaled per use.
    for (int v = 0; v < 2; ++v) {
        float vp = ((float)v + 0.5f) / 2.0f;
        float sin_theta = host_det_sin(kPi * vp);
        std::vector<float> row(2);
        for (int u = 0; u < 2; ++u) {
            float y = 1.0f;
            if (!plan->infinite_ids.empty()) {
                const float* L = plan->lights[plan->infinite_ids[0]].L;
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
    // light sampling distributions (lightdistrib.rs:21-69, integrator.rs:268-277)
    if (desc.n_lights > 0) {
        plan->uniform_func.assign(desc.n_lights, 1.0f);
        make_distribution(plan->uniform_func, &plan->uniform_cdf, &d.light_distrib_uniform.func_int);
        d.light_distrib_uniform.n = desc.n_lights;
        make_distribution(plan->power_func, &plan->power_cdf, &d.light_distrib_power.func_int);
        d.light_distrib_power.n = desc.n_lights;
    }
}

// ---- two-level scenes: the object table, the top-level leaf slots' records, the motion rows, the local slot_prim ----
static void plan_instancing(const SceneDesc& desc, ScenePlan* plan) {
    const InstancingArgs& ia = desc.ia;
    const int32_t n_top = desc.n_top(), n_prims = desc.n_prims();
    DevBVH& bvh = plan->d.bvh;
    bvh.general_top = (ia.n_objects > 1 || ia.n_world_tris > 0) ? 1 : 0;
    bvh.blas_root_ref = plan->obj_root_ref[0];
    std::memcpy(bvh.blas_root_min, ia.objects[0].nodes[0].bounds_min, 12);
    std::memcpy(bvh.blas_root_max, ia.objects[0].nodes[0].bounds_max, 12);
    // object table: (root box min, root reference) (root box max, -)
    plan->objects.assign((size_t)ia.n_objects * 8, 0.0f);
    for (int32_t k = 0; k < ia.n_objects; ++k) {
        const PbrtLinearBVHNode& root = ia.objects[k].nodes[0];
        float* r = &plan->objects[(size_t)k * 8];
        std::memcpy(r, root.bounds_min, 12);
        std::memcpy(r + 3, &plan->obj_root_ref[k], 4);
        std::memcpy(r + 4, root.bounds_max, 12);
    }
    // records of the top-level leaf slots: to_object rows 0-2, to_world rows 0-2, (material, instance id, object, kind);
    // a world-space triangle beside the instances: kind 1, its leaf slot in the third field
    plan->top_slot_records.assign((size_t)n_top * 28, 0.0f);
    plan->slot_inst.resize(n_top);
    for (int32_t slot = 0; slot < n_top; ++slot) {
        int32_t id = ia.tlas_order[slot];
        float* r = &plan->top_slot_records[(size_t)slot * 28];
        if (id < ia.n_instances) {
            plan->slot_inst[slot] = id;
            std::memcpy(r, ia.instances[id].to_object, 48);
            std::memcpy(r + 12, ia.instances[id].to_world, 48);
            int32_t meta[4] = {ia.instances[id].material, id, ia.instance_object ? ia.instance_object[id] : 0, 0};
            std::memcpy(r + 24, meta, 16);
        } else {
            plan->slot_inst[slot] = -1;
            int32_t meta[4] = {-1, -1, plan->prim_slot[ia.world_tri_offset + (id - ia.n_instances)], 1};
            std::memcpy(r + 24, meta, 16);
        }
    }
    if (ia.motions) {  // moving instances: one row per top-level slot on the device
        plan->motions.assign(n_top, DevMotion{});
        for (int32_t slot = 0; slot < n_top; ++slot)
            if (plan->slot_inst[slot] >= 0) motion_row(ia.instances[plan->slot_inst[slot]], ia.motions[plan->slot_inst[slot]], &plan->motions[slot]);
    }
    // hit records name a triangle by its index inside its own object (world triangles: their own list)
    plan->slot_prim.resize(n_prims);
    int32_t k = 0;
    for (int32_t slot = 0; slot < n_prims; ++slot) {
        while (k < ia.n_objects && slot >= ia.obj_tri_offset[k + 1]) ++k;
        plan->slot_prim[slot] = desc.prim_order[slot] - (k < ia.n_objects ? ia.obj_tri_offset[k] : ia.world_tri_offset);
    }
}

void plan_scene(const SceneDesc& desc, ScenePlan* plan) {
    const InstancingArgs& ia = desc.ia;
    const DeviceTree* dt = desc.dt;
    DevSceneData& d = plan->d;
    std::memset(&d, 0, sizeof(d));
    // ---- interior records: both children's boxes + references + axis (64 B) ----
    TreeLayout top;
    if (desc.instanced()) {
        top = convert_tree(ia.tlas_nodes, ia.n_tlas_nodes, 0, &plan->inodes);
        // the object-level trees behind it in one record array; one leaf-reference width for all of them
        const int bits = shared_count_bits(ia);
        int base = top.n_interior;
        plan->obj_root_ref.resize(ia.n_objects);
        for (int32_t k = 0; k < ia.n_objects; ++k) {
            TreeLayout o = convert_tree(ia.objects[k].nodes, ia.objects[k].n_nodes, base, &plan->inodes, ia.obj_tri_offset[k], bits);
            base += o.n_interior;
            plan->obj_root_ref[k] = o.root_ref;
        }
        plan->n_interior = base;
        d.bvh.blas_count_bits = bits;
    } else if (dt) {
        top.n_interior = dt->n_interior;
        top.root_ref = dt->root_ref;
        top.count_bits = dt->count_bits;
        plan->n_interior = dt->n_interior;
    } else {
        top = convert_tree(desc.nodes, desc.n_nodes, 0, &plan->inodes);
        plan->n_interior = top.n_interior;
    }
    if (plan->inodes.empty()) plan->inodes.assign(16, 0.0f);
    if (!dt) plan_prim_records(desc, plan);

    // Bounds3::bounding_sphere of the root bounds (infinite.rs:135-139)
    const float* mn = dt ? dt->root_min : (desc.instanced() ? ia.tlas_nodes[0] : desc.nodes[0]).bounds_min;
    const float* mx = dt ? dt->root_max : (desc.instanced() ? ia.tlas_nodes[0] : desc.nodes[0]).bounds_max;
    {
        float dx[3];
        for (int k = 0; k < 3; ++k) {
            d.world_center[k] = (mn[k] + mx[k]) / 2.0f;
            dx[k] = d.world_center[k] - mx[k];
        }
        bool inside = true;
        for (int k = 0; k < 3; ++k) inside = inside && d.world_center[k] >= mn[k] && d.world_center[k] <= mx[k];
        d.world_radius = inside ? std::sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]) : 0.0f;
    }
    plan_lights(desc, plan);
    plan->materials.resize(desc.n_materials);
    for (int32_t i = 0; i < desc.n_materials; ++i) {
        plan->materials[i] = row_of_material(desc.materials[i]);
        plan->glossy = plan->glossy || desc.materials[i].type == PBRT_MAT_PLASTIC || desc.materials[i].type == PBRT_MAT_METAL;
    }
    std::memcpy(d.bvh.root_min, mn, 12);
    std::memcpy(d.bvh.root_max, mx, 12);
    d.bvh.root_ref = top.root_ref;
    d.bvh.count_bits = top.count_bits;
    d.bvh.n_slots = desc.n_prims();
    // (a scene with curves is a scene with shapes, whether it holds a quadric or not: its builds are theirs with the curve added)
    d.bvh.has_spheres = (desc.sa.n_shapes > 0 || desc.n_curves > 0) ? 2 : (desc.sa.n > 0 ? 1 : 0);
    plan->curves.resize(desc.n_curves);
    for (int32_t i = 0; i < desc.n_curves; ++i) plan->curves[i] = curve_row(desc.curves[i]);
    d.n_curves = desc.n_curves;
    if (desc.n_curves > 0) {  // the rows a hair material may not take: those a triangle or a quadric shape names
        plan->row_off_curve.assign(desc.n_materials, 0);
        for (int32_t i = 0; i < desc.n_tris; ++i) plan->row_off_curve[desc.tri_material ? desc.tri_material[i] : 0] = 1;
        for (int32_t i = 0; i < desc.sa.n_shapes; ++i) plan->row_off_curve[desc.sa.shapes[i].material] = 1;
    }
    plan->shapes.resize(desc.sa.n_shapes);
    for (int32_t i = 0; i < desc.sa.n_shapes; ++i) plan->shapes[i] = shape_row(desc.sa.shapes[i]);
    d.bvh.instanced = desc.instanced() ? 1 : 0;
    if (desc.instanced()) plan_instancing(desc, plan);
    d.n_lights = desc.n_lights;
    d.n_materials = desc.n_materials;
    d.n_infinite = (int)plan->infinite_ids.size();
    plan_distributions(desc, plan);
}

const char* plan_two_level_wide(const SceneDesc& desc, const ScenePlan& plan, TwoLevelWide* out) {
    const InstancingArgs& ia = desc.ia;
    const int32_t n_top = desc.n_top(), n_prims = desc.n_prims();
    WideTree top;
    if (const char* why = build_wide_tree(ia.tlas_nodes, ia.n_tlas_nodes, nullptr, n_top, &top)) return why;
    std::vector<WideTree> wobj(ia.n_objects);
    int record_base = top.n_records, deepest = 0;
    for (int32_t k = 0; k < ia.n_objects; ++k) {
        WideBase b;
        b.record = record_base;
        b.tri = b.slot = ia.obj_tri_offset[k];
        if (const char* why = build_wide_tree(ia.objects[k].nodes, ia.objects[k].n_nodes, plan.tris.data() + 12 * (size_t)ia.obj_tri_offset[k],
                                              ia.objects[k].n_tris, &wobj[k], b))
            return why;
        record_base += wobj[k].n_records;
        deepest = std::max(deepest, wobj[k].stack_need);
    }
    std::vector<uint32_t>& wn = out->nodes;
    wn.insert(wn.end(), top.nodes.begin(), top.nodes.begin() + (size_t)top.n_records * kWideNodeDwords);
    out->tris.assign((size_t)n_prims * 12, 0.0f);
    out->leaf_boxes.assign((size_t)n_prims * 8, 0.0f);
    out->objects.assign((size_t)ia.n_objects * 8, 0.0f);
    for (int32_t k = 0; k < ia.n_objects; ++k) {
        wn.insert(wn.end(), wobj[k].nodes.begin(), wobj[k].nodes.begin() + (size_t)wobj[k].n_records * kWideNodeDwords);
        std::memcpy(&out->tris[12 * (size_t)ia.obj_tri_offset[k]], wobj[k].tris.data(), wobj[k].tris.size() * 4);
        std::memcpy(&out->leaf_boxes[8 * (size_t)ia.obj_tri_offset[k]], wobj[k].leaf_boxes.data(), wobj[k].leaf_boxes.size() * 4);
        const PbrtLinearBVHNode& root = ia.objects[k].nodes[0];
        float* r = &out->objects[(size_t)k * 8];
        std::memcpy(r, root.bounds_min, 12);
        std::memcpy(r + 3, &wobj[k].root_ref, 4);
        std::memcpy(r + 4, root.bounds_max, 12);
    }
    if (wn.empty()) wn.assign(kWideNodeDwords, 0u);
    // the top-level entries as the wide kernel reads them, in wide order, 20 floats each: the exact box of the leaf
    // the entry belongs to with two words in the w fields — the binary-layout top slot (hit records name it) and
    // the object index (an instance) or 0x40000000 | leaf slot (a world-space triangle) — then the three
    // world-to-object rows
    out->top_slots.resize((size_t)n_top * 20);
    for (int32_t pos = 0; pos < n_top; ++pos) {
        const int32_t slot = top.order[pos];
        const float* src = &plan.top_slot_records[(size_t)slot * 28];
        float* dst = &out->top_slots[(size_t)pos * 20];
        int32_t meta[4];
        std::memcpy(meta, src + 24, 16);  // (material, id, object | leaf slot, kind)
        const int32_t word = meta[3] == 1 ? (0x40000000 | meta[2]) : meta[2];
        std::memcpy(dst, &top.leaf_boxes[(size_t)pos * 8], 12);
        std::memcpy(dst + 3, &slot, 4);
        std::memcpy(dst + 4, &top.leaf_boxes[(size_t)pos * 8 + 4], 12);
        std::memcpy(dst + 7, &word, 4);
        std::memcpy(dst + 8, src, 48);
    }
    out->top_boxes = std::move(top.leaf_boxes);
    out->root_ref = top.root_ref;
    out->obj0_root = wobj[0].root_ref;
    out->n_records = record_base;
    out->stack_need = top.stack_need + deepest + 1;
    return nullptr;
}

}  // namespace pb
