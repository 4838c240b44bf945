// scene_plan_check.cpp — host-side check of scene creation's first two phases (test infrastructure, built and run by
// tests/test_scene_plan_host.py under AddressSanitizer and UBSan; not part of the product library).
//
// Links the product's own pbrt-rs_amd/csrc/host_scene.cpp (scene_invalid, plan_scene, plan_two_level_wide) with the host files
// it calls, builds tiny scenes with pbrt_hip_bvh_build and checks
//   - invariants of the plan that do not restate the code: prim_slot inverts prim_order, triangle records hold the mesh's
//     vertices, an area light's slot holds a record that names the light, every cdf runs from 0 to 1 without falling, the
//     uniform distribution integrates to 1, one interior record per interior node, the two-level wide entries name every
//     top-level slot exactly once;
//   - the message scene_invalid gives for each bad input the GPU tests feed the C ABI, and a few only a CPU can afford to
//     feed under a sanitizer (duplicated order entries, a motion bound outside its leaf, a non-affine instance).
// The code under test turns caller-supplied indices into array subscripts: the sanitizers watch every one of them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../pbrt-rs_amd/csrc/host_scene.h"

namespace pb {
void set_thread_error(const std::string&) {}  // pbrt_hip.hip's, for host_motion.cpp's context-free entry points
}

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++g_failures;                                  \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

struct Tree {
    std::vector<PbrtLinearBVHNode> nodes;
    std::vector<int32_t> order;
};
Tree take(PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t* order, int32_t n) {
    Tree t;
    t.nodes.assign(nodes, nodes + n_nodes);
    t.order.assign(order, order + n);
    pbrt_hip_free(nodes);
    pbrt_hip_free(order);
    return t;
}
Tree tree_over_mesh(const std::vector<float>& pos, const std::vector<int32_t>& idx, int max_prims, int split = 0) {
    PbrtLinearBVHNode* nodes = nullptr;
    int32_t n_nodes = 0, *order = nullptr;
    int rc = pbrt_hip_bvh_build(pos.data(), (int32_t)pos.size() / 3, idx.data(), (int32_t)idx.size() / 3, max_prims, split, &nodes, &n_nodes, &order);
    CHECK(rc == PBRT_HIP_OK, "pbrt_hip_bvh_build %d", rc);
    return take(nodes, n_nodes, order, (int32_t)idx.size() / 3);
}
Tree tree_over_boxes(const std::vector<float>& lo, const std::vector<float>& hi, int max_prims) {
    PbrtLinearBVHNode* nodes = nullptr;
    int32_t n_nodes = 0, *order = nullptr;
    int rc = pbrt_hip_bvh_build_boxes(lo.data(), hi.data(), (int32_t)lo.size() / 3, max_prims, 0, &nodes, &n_nodes, &order);
    CHECK(rc == PBRT_HIP_OK, "pbrt_hip_bvh_build_boxes %d", rc);
    return take(nodes, n_nodes, order, (int32_t)lo.size() / 3);
}

// a 12-triangle box of half-width h around c
struct Mesh {
    std::vector<float> pos;
    std::vector<int32_t> idx;
};
Mesh box(float cx, float cy, float cz, float h) {
    Mesh m;
    for (int v = 0; v < 8; ++v) {
        m.pos.push_back(cx + ((v & 1) ? h : -h));
        m.pos.push_back(cy + ((v & 2) ? h : -h));
        m.pos.push_back(cz + ((v & 4) ? h : -h));
    }
    const int q[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
    for (auto& f : q) {
        const int a[6] = {f[0], f[1], f[2], f[0], f[2], f[3]};
        m.idx.insert(m.idx.end(), a, a + 6);
    }
    return m;
}
void tri_bounds(const Mesh& m, std::vector<float>* lo, std::vector<float>* hi) {
    for (size_t t = 0; t < m.idx.size() / 3; ++t)
        for (int c = 0; c < 3; ++c) {
            float a = INFINITY, b = -INFINITY;
            for (int v = 0; v < 3; ++v) {
                const float x = m.pos[3 * (size_t)m.idx[3 * t + v] + c];
                a = std::fmin(a, x);
                b = std::fmax(b, x);
            }
            lo->push_back(a);
            hi->push_back(b);
        }
}
PbrtMaterial matte() {
    PbrtMaterial m;
    std::memset(&m, 0, sizeof(m));
    m.type = PBRT_MAT_MATTE;
    m.kd[0] = m.kd[1] = m.kd[2] = 0.5f;
    m.eta = 1.0f;
    return m;
}
PbrtLight area_light(int32_t prim) {
    PbrtLight l;
    std::memset(&l, 0, sizeof(l));
    l.type = PBRT_LIGHT_DIFFUSE_AREA;
    l.L[0] = l.L[1] = l.L[2] = 5.0f;
    l.prim = prim;
    l.n_samples = 1;
    return l;
}
PbrtLight point_light() {
    PbrtLight l = area_light(0);
    l.type = PBRT_LIGHT_POINT;
    l.pos[1] = 3.0f;
    return l;
}
void identity(float m[16]) {
    std::memset(m, 0, 64);
    m[0] = m[5] = m[10] = m[15] = 1.0f;
}
PbrtInstance instance_at(float x, float y, float z) {
    PbrtInstance in;
    std::memset(&in, 0, sizeof(in));
    identity(in.to_world);
    identity(in.to_object);
    in.to_world[3] = x; in.to_world[7] = y; in.to_world[11] = z;
    in.to_object[3] = -x; in.to_object[7] = -y; in.to_object[11] = -z;
    in.material = -1;
    return in;
}

// A scene with everything it points at. desc is filled by the makers below.
struct Scene {
    Mesh mesh;
    std::vector<int32_t> tri_material, tri_light;
    std::vector<PbrtMaterial> materials;
    std::vector<PbrtLight> lights;
    Tree tree;
    std::vector<float> spheres;
    std::vector<int32_t> sphere_material, sphere_light;
    std::vector<PbrtShape> shapes;
    // two levels
    std::vector<Mesh> obj_mesh;
    std::vector<Tree> obj_tree;
    std::vector<PbrtObject> objects;
    std::vector<PbrtInstance> instances;
    std::vector<PbrtInstanceMotion> motions;
    std::vector<int32_t> instance_object;
    Tree top;
    int64_t n_tree_nodes = 0;  // of every tree of the scene
    pb::SceneDesc desc;

    void point_desc_at_mesh() {
        desc.positions = mesh.pos.data();
        desc.n_verts = (int32_t)mesh.pos.size() / 3;
        desc.indices = mesh.idx.data();
        desc.n_tris = (int32_t)mesh.idx.size() / 3;
        desc.tri_material = tri_material.data();
        desc.tri_light = tri_light.data();
        desc.materials = materials.data();
        desc.n_materials = (int32_t)materials.size();
        desc.lights = lights.data();
        desc.n_lights = (int32_t)lights.size();
    }
    void point_desc_at_tree() {
        desc.nodes = tree.nodes.data();
        desc.n_nodes = (int32_t)tree.nodes.size();
        desc.prim_order = tree.order.data();
        n_tree_nodes = desc.n_nodes;
    }
};

// the box with an area light on triangle 5 and a point light
void make_box(Scene* s, int max_prims) {
    s->mesh = box(0, 0, 0, 1);
    s->tri_material.assign(12, 0);
    s->tri_light.assign(12, -1);
    s->tri_light[5] = 0;
    s->materials = {matte(), matte()};
    s->lights = {area_light(5), point_light()};
    s->tree = tree_over_mesh(s->mesh.pos, s->mesh.idx, max_prims);
    s->point_desc_at_mesh();
    s->point_desc_at_tree();
}
void make_box_with_spheres(Scene* s) {
    make_box(s, 4);
    s->spheres = {3, 0, 0, 0.5f, 0, 3, 0, 0.25f};
    s->sphere_material = {1, 0};
    s->sphere_light = {-1, -1};
    std::vector<float> lo, hi;
    tri_bounds(s->mesh, &lo, &hi);
    for (int i = 0; i < 2; ++i)
        for (int c = 0; c < 3; ++c) {
            lo.push_back(s->spheres[4 * i + c] - s->spheres[4 * i + 3]);
            hi.push_back(s->spheres[4 * i + c] + s->spheres[4 * i + 3]);
        }
    s->tree = tree_over_boxes(lo, hi, 2);
    s->point_desc_at_tree();
    s->desc.sa.spheres = s->spheres.data();
    s->desc.sa.material = s->sphere_material.data();
    s->desc.sa.light = s->sphere_light.data();
    s->desc.sa.n = 2;
}
PbrtShape shape(int type, float x) {
    PbrtShape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.type = type;
    sh.material = 0;
    sh.light = -1;
    sh.radius = 0.5f;
    sh.z_min = type == PBRT_SHAPE_DISK ? 0.0f : -0.5f;
    sh.z_max = 0.5f;
    sh.phi_max = 360.0f;
    identity(sh.to_world);
    identity(sh.to_object);
    sh.to_world[3] = x;
    sh.to_object[3] = -x;
    return sh;
}
// the box, a sphere that carries area light 2, a disk and a cylinder
void make_box_with_shapes(Scene* s) {
    make_box(s, 4);
    s->shapes = {shape(PBRT_SHAPE_SPHERE, 3), shape(PBRT_SHAPE_DISK, 5), shape(PBRT_SHAPE_CYLINDER, 7)};
    s->shapes[0].light = 2;
    s->lights.push_back(area_light(12));  // primitive n_tris + 0
    std::vector<float> lo, hi, b(6 * 3);
    tri_bounds(s->mesh, &lo, &hi);
    CHECK(pbrt_hip_shape_world_bounds(s->shapes.data(), 3, b.data()) == PBRT_HIP_OK, "shape bounds");
    for (int i = 0; i < 3; ++i) {
        lo.insert(lo.end(), &b[6 * i], &b[6 * i] + 3);
        hi.insert(hi.end(), &b[6 * i + 3], &b[6 * i + 3] + 3);
    }
    s->tree = tree_over_boxes(lo, hi, 2);
    s->point_desc_at_mesh();
    s->point_desc_at_tree();
    s->desc.sa.shapes = s->shapes.data();
    s->desc.sa.n_shapes = 3;
}
// 2 objects x 3 instances + 2 world triangles, the second of them an area light; `moving`: instance 1 travels along x and
// the top-level tree is built over the motion bounds
void make_two_level(Scene* s, bool moving) {
    s->obj_mesh = {box(0, 0, 0, 0.5f), box(0, 0, 0, 0.25f)};
    s->objects.resize(2);
    for (int k = 0; k < 2; ++k) {
        s->obj_tree.push_back(tree_over_mesh(s->obj_mesh[k].pos, s->obj_mesh[k].idx, k == 0 ? 1 : 4));
        PbrtObject& o = s->objects[k];
        o.positions = s->obj_mesh[k].pos.data();
        o.n_verts = 8;
        o.indices = s->obj_mesh[k].idx.data();
        o.n_tris = 12;
        o.tri_material = nullptr;
        o.nodes = s->obj_tree[k].nodes.data();
        o.n_nodes = (int32_t)s->obj_tree[k].nodes.size();
        o.prim_order = s->obj_tree[k].order.data();
        s->n_tree_nodes += o.n_nodes;
    }
    s->instances = {instance_at(-3, 0, 0), instance_at(0, 0, 0), instance_at(3, 0, 0)};
    s->instance_object = {0, 1, 0};
    s->motions.resize(3);
    std::memset(s->motions.data(), 0, sizeof(PbrtInstanceMotion) * 3);
    if (moving) {
        PbrtInstanceMotion& mo = s->motions[1];
        PbrtInstance end = instance_at(0.75f, 0, 0);
        std::memcpy(mo.end_to_world, end.to_world, 64);
        mo.start_time = 0.0f;
        mo.end_time = 1.0f;
        mo.animated = 1;
    }
    // the combined mesh, as combine_two_level lays it out (scene_edit_check.cpp holds it to that): object after object, then the world triangles
    const float wpos[12] = {-1, 2, -1, 1, 2, -1, 1, 2, 1, -1, 2, 1};
    const int32_t widx[6] = {0, 1, 2, 0, 2, 3};
    pb::InstancingArgs& ia = s->desc.ia;
    ia.obj_tri_offset = {0, 12, 24};
    ia.world_tri_offset = 24;
    ia.n_world_tris = 2;
    std::vector<int32_t> order;
    for (int k = 0; k < 2; ++k) {
        for (int32_t i : s->obj_mesh[k].idx) s->mesh.idx.push_back(i + 8 * k);
        s->mesh.pos.insert(s->mesh.pos.end(), s->obj_mesh[k].pos.begin(), s->obj_mesh[k].pos.end());
        for (int32_t o : s->obj_tree[k].order) order.push_back(o + 12 * k);
    }
    s->mesh.pos.insert(s->mesh.pos.end(), wpos, wpos + 12);
    for (int32_t i : widx) s->mesh.idx.push_back(i + 16);
    order.push_back(24);
    order.push_back(25);
    s->tree.order = order;
    s->tri_material.assign(26, 0);
    s->tri_light.assign(26, -1);
    s->tri_light[25] = 0;
    s->materials = {matte()};
    s->lights = {area_light(1), point_light()};  // prim counts the world triangles
    // the top-level tree over the instances' (motion) bounds, then the world triangles' bounds
    std::vector<float> lo(15), hi(15);
    for (int i = 0; i < 3; ++i) {
        const PbrtLinearBVHNode& root = s->obj_tree[s->instance_object[i]].nodes[0];
        CHECK(pbrt_hip_instance_motion_bounds(root.bounds_min, root.bounds_max, &s->instances[i], &s->motions[i], 1, &lo[3 * i], &hi[3 * i]) == PBRT_HIP_OK,
              "motion bounds of instance %d", i);
    }
    Mesh world;
    world.pos.assign(wpos, wpos + 12);
    world.idx.assign(widx, widx + 6);
    std::vector<float> wlo, whi;
    tri_bounds(world, &wlo, &whi);
    std::copy(wlo.begin(), wlo.end(), lo.begin() + 9);
    std::copy(whi.begin(), whi.end(), hi.begin() + 9);
    s->top = tree_over_boxes(lo, hi, 1);
    s->n_tree_nodes += (int64_t)s->top.nodes.size();
    s->point_desc_at_mesh();
    s->desc.nodes = nullptr;
    s->desc.n_nodes = (int32_t)(s->obj_tree[0].nodes.size() + s->obj_tree[1].nodes.size());
    s->desc.prim_order = s->tree.order.data();
    ia.instances = s->instances.data();
    ia.n_instances = 3;
    ia.tlas_nodes = s->top.nodes.data();
    ia.n_tlas_nodes = (int32_t)s->top.nodes.size();
    ia.tlas_order = s->top.order.data();
    ia.objects = s->objects.data();
    ia.n_objects = 2;
    ia.instance_object = s->instance_object.data();
    ia.motions = moving ? s->motions.data() : nullptr;
}

void check_cdf(const float* cdf, int n, const char* scene, const char* what) {
    CHECK(cdf[0] == 0.0f && cdf[n] == 1.0f, "%s: %s cdf runs from %g to %g", scene, what, cdf[0], cdf[n]);
    for (int i = 0; i < n; ++i) CHECK(cdf[i + 1] >= cdf[i], "%s: %s cdf falls at %d", scene, what, i);
}

// the plan of a good scene
void check_plan(const Scene& s, const char* name) {
    const pb::SceneDesc& d = s.desc;
    const std::string why = pb::scene_invalid(d);
    CHECK(why.empty(), "%s: refused: %s", name, why.c_str());
    if (!why.empty()) return;
    pb::ScenePlan plan;
    pb::plan_scene(d, &plan);
    const int32_t n_prims = d.n_prims();
    CHECK((int32_t)plan.prim_slot.size() == n_prims && plan.tris.size() == (size_t)n_prims * 12, "%s: record counts", name);
    for (int32_t slot = 0; slot < n_prims; ++slot) {
        const int32_t prim = d.prim_order[slot];
        CHECK(plan.prim_slot[prim] == slot, "%s: prim_slot[%d] = %d, slot %d", name, prim, plan.prim_slot[prim], slot);
        if (prim >= d.n_tris) continue;
        for (int v = 0; v < 3; ++v)
            CHECK(std::memcmp(&plan.tris[(size_t)slot * 12 + 3 * v], d.positions + 3 * (size_t)d.indices[3 * (size_t)prim + v], 12) == 0,
                  "%s: slot %d vertex %d", name, slot, v);
    }
    for (int32_t i = 0; i < d.n_lights; ++i) {
        if (d.lights[i].type != PBRT_LIGHT_DIFFUSE_AREA) continue;
        const int32_t slot = plan.lights[i].slot;
        CHECK(slot >= 0 && slot < n_prims, "%s: light %d slot %d", name, i, slot);
        if (slot < 0 || slot >= n_prims) continue;
        int32_t w;
        std::memcpy(&w, &plan.tris[(size_t)slot * 12 + 11], 4);
        CHECK((w & ~(pb::kTriDegenerate | pb::kPrimSphere)) - 1 == i, "%s: light %d sits on a record of light %d", name, i,
              (w & ~(pb::kTriDegenerate | pb::kPrimSphere)) - 1);
        CHECK(plan.lights[i].area > 0.0f && plan.lights[i].power_y > 0.0f, "%s: light %d area %g power %g", name, i, plan.lights[i].area, plan.lights[i].power_y);
    }
    if (d.n_lights > 0) {
        check_cdf(plan.uniform_cdf.data(), d.n_lights, name, "uniform");
        check_cdf(plan.power_cdf.data(), d.n_lights, name, "power");
        CHECK(plan.d.light_distrib_uniform.func_int == 1.0f, "%s: uniform func_int %g", name, plan.d.light_distrib_uniform.func_int);
    }
    check_cdf(plan.d.env_cond_cdf[0], 2, name, "env row 0");
    check_cdf(plan.d.env_cond_cdf[1], 2, name, "env row 1");
    check_cdf(plan.d.env_marg_cdf, 2, name, "env marginal");
    CHECK(plan.d.light_distrib_uniform.n == d.n_lights && plan.d.light_distrib_power.n == d.n_lights, "%s: distribution sizes", name);
    int64_t n_trees = d.instanced() ? 1 + d.ia.n_objects : 1;
    CHECK(plan.n_interior == (s.n_tree_nodes - n_trees) / 2, "%s: %d interior records for %lld nodes in %lld trees", name, plan.n_interior,
          (long long)s.n_tree_nodes, (long long)n_trees);
    CHECK(plan.inodes.size() == (size_t)std::max(plan.n_interior, 1) * 16, "%s: interior record floats", name);
    CHECK((int32_t)plan.shapes.size() == d.sa.n_shapes, "%s: shape rows", name);
    if (!d.instanced()) return;
    const int32_t n_top = d.n_top();
    CHECK((int32_t)plan.slot_inst.size() == n_top && plan.top_slot_records.size() == (size_t)n_top * 28, "%s: top-level records", name);
    CHECK(plan.motions.size() == (d.ia.motions ? (size_t)n_top : 0), "%s: motion rows", name);
    for (int32_t slot = 0; slot < n_top; ++slot) {
        const int32_t id = d.ia.tlas_order[slot];
        CHECK(plan.slot_inst[slot] == (id < d.ia.n_instances ? id : -1), "%s: slot_inst[%d]", name, slot);
        if (d.ia.motions) CHECK(plan.motions[slot].animated == (id < d.ia.n_instances ? d.ia.motions[id].animated : 0), "%s: motion row of slot %d", name, slot);
    }
    for (int32_t slot = 0; slot < n_prims; ++slot) CHECK(plan.slot_prim[slot] >= 0 && plan.slot_prim[slot] < 12, "%s: local slot_prim[%d]", name, slot);
    pb::TwoLevelWide tw;
    const char* no_wide = pb::plan_two_level_wide(d, plan, &tw);
    CHECK(no_wide == nullptr, "%s: no wide records: %s", name, no_wide);
    if (no_wide) return;
    std::vector<int> named(n_top, 0);
    CHECK(tw.top_slots.size() == (size_t)n_top * 20, "%s: wide top-level entries", name);
    for (int32_t pos = 0; pos < n_top; ++pos) {
        int32_t slot;
        std::memcpy(&slot, &tw.top_slots[(size_t)pos * 20 + 3], 4);
        CHECK(slot >= 0 && slot < n_top, "%s: wide entry %d names slot %d", name, pos, slot);
        if (slot >= 0 && slot < n_top) ++named[slot];
    }
    for (int32_t slot = 0; slot < n_top; ++slot) CHECK(named[slot] == 1, "%s: top-level slot %d named %d times", name, slot, named[slot]);
    CHECK(tw.nodes.size() == (size_t)std::max(tw.n_records, 1) * pb::kWideNodeDwords && tw.tris.size() == (size_t)n_prims * 12, "%s: wide array sizes", name);
}

void expect(const pb::SceneDesc& d, const char* want, const char* what) {
    const std::string why = pb::scene_invalid(d);
    CHECK(why.find(want) != std::string::npos, "%s: expected \"%s\", got \"%s\"", what, want, why.c_str());
}

// every bad input of tests/test_gpu_intersect.py::test_error_behaviour_of_the_c_abi, on the box
void check_refusals_of_the_box() {
    Scene s;
    make_box(&s, 4);
    {
        Scene b = s;
        b.mesh.idx[3 * 3 + 1] = 10000;
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "vertex index out of range", "vertex index");
    }
    {
        Scene b = s;
        b.tree.order[0] = b.tree.order[1];
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "prim_order is not a permutation", "duplicated prim_order entry");
        b.tree.order[0] = 12;
        expect(b.desc, "prim_order entry out of range", "prim_order entry past the end");
    }
    {
        Scene b = s;
        b.tree.nodes[0].offset = 1;  // second child must come after the first subtree
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "second-child offset out of range", "root offset");
    }
    {
        Scene b = s;
        b.tree.nodes.resize(b.tree.nodes.size() - 2);
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        const std::string why = pb::scene_invalid(b.desc);
        CHECK(why.find("full binary tree") != std::string::npos || why.find("leaves do not cover") != std::string::npos ||
                  why.find("offset out of range") != std::string::npos,
              "truncated node array: got \"%s\"", why.c_str());
    }
    {
        Scene b = s;
        b.tri_material[0] = 99;
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "tri_material out of range", "tri_material");
    }
    {
        Scene b = s;
        b.materials[0].type = 17;
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "material type", "material type");
    }
    {
        Scene b = s;
        b.lights[0].prim = 10000;
        b.point_desc_at_mesh();
        b.point_desc_at_tree();
        expect(b.desc, "area light primitive out of range", "area light prim");
        b.lights[0].prim = 5;
        b.lights[0].type = 42;
        expect(b.desc, "unknown light type", "light type");
    }
    {
        // the description pbrt_hip_scene_create_hlbvh checks before its device build: no tree, same wording
        Scene b = s;
        b.point_desc_at_mesh();
        b.desc.device_tree = true;
        CHECK(pb::scene_invalid(b.desc).empty(), "device-tree description refused");
        b.lights[0].prim = 12;
        expect(b.desc, "area light primitive out of range", "device-tree description, area light");
        b.mesh.idx[0] = -1;
        expect(b.desc, "vertex index out of range", "device-tree description, vertex index");
        b.desc.n_tris = 0;
        expect(b.desc, "empty scene", "device-tree description, no triangles");
    }
}

// tests/test_gpu_shapes.py: the material and light cases of test_creation_refusals_leave_the_context_usable
void check_refusals_of_shapes() {
    Scene s;
    make_box_with_shapes(&s);
    const PbrtShape good = s.shapes[1];
    s.shapes[1].material = 2;
    expect(s.desc, "shape material out of range", "shape material past the table");
    s.shapes[1].material = -1;
    expect(s.desc, "shape material out of range", "negative shape material");
    s.shapes[1] = good;
    s.shapes[1].light = 3;
    expect(s.desc, "shape light out of range", "shape light past the table");
    s.shapes[1] = good;
    s.shapes[1].type = 3;
    expect(s.desc, "unknown shape type", "shape type");
    s.shapes[1] = good;
    s.desc.sa.spheres = s.shapes[0].to_world;  // spheres and shapes in one scene
    s.desc.sa.n = 1;
    expect(s.desc, "bad shape arguments", "spheres beside shapes");
}

// tests/test_gpu_intersect.py::test_too_deep_tree_is_refused: 80 triangles the midpoint split peels off one per level
void check_too_deep_tree() {
    Scene s;
    const int n = 80;
    float x = 1.0f;
    for (int i = 0; i < n; ++i, x *= 3.0f) {
        const float p[9] = {x, 0, 0, x, 1e-3f, 0, x, 0, 1e-3f};
        s.mesh.pos.insert(s.mesh.pos.end(), p, p + 9);
        for (int v = 0; v < 3; ++v) s.mesh.idx.push_back(3 * i + v);
    }
    s.tri_material.assign(n, 0);
    s.tri_light.assign(n, -1);
    s.materials = {matte()};
    s.tree = tree_over_mesh(s.mesh.pos, s.mesh.idx, 1, 2 /* Middle */);
    s.point_desc_at_mesh();
    s.point_desc_at_tree();
    expect(s.desc, "deeper than the 64-entry", "80 levels");
    s.tree = tree_over_mesh(s.mesh.pos, s.mesh.idx, 1, 0 /* SAH: balanced */);
    s.point_desc_at_tree();
    check_plan(s, "80 triangles under a balanced tree");
}

void check_refusals_of_two_levels() {
    {
        Scene s;
        make_two_level(&s, false);
        s.top.order[0] = s.top.order[1];
        expect(s.desc, "tlas_order is not a permutation", "duplicated tlas_order entry");
        s.top.order[0] = 5;
        expect(s.desc, "tlas_order entry out of range", "tlas_order entry past the end");
    }
    {
        Scene s;
        make_two_level(&s, false);
        s.instances[2].to_world[12] = 0.5f;
        expect(s.desc, "instance transforms must be affine", "non-affine instance");
        s.instances[2].to_world[12] = 0.0f;
        s.instances[0].material = 1;
        expect(s.desc, "instance material out of range", "instance material");
    }
    {
        // the moving instance under a top-level tree built over the STATIC bounds: the motion bound leaves its leaf
        Scene moving, still;
        make_two_level(&moving, true);
        make_two_level(&still, false);
        moving.top = still.top;
        moving.desc.ia.tlas_nodes = moving.top.nodes.data();
        moving.desc.ia.n_tlas_nodes = (int32_t)moving.top.nodes.size();
        moving.desc.ia.tlas_order = moving.top.order.data();
        expect(moving.desc, "instance 1: its motion bound", "motion bound outside its leaf");
    }
    {
        Scene s;
        make_two_level(&s, true);
        s.motions[1].end_time = s.motions[1].start_time;
        expect(s.desc, "moving instance 1: ", "empty time range");
    }
}

}  // namespace

int main() {
    for (int max_prims : {1, 4}) {
        Scene s;
        make_box(&s, max_prims);
        check_plan(s, max_prims == 1 ? "box, one triangle per leaf" : "box, up to four per leaf");
    }
    {
        Scene s;
        make_box_with_spheres(&s);
        check_plan(s, "box and spheres");
    }
    {
        Scene s;
        make_box_with_shapes(&s);
        check_plan(s, "box and shapes");
    }
    for (bool moving : {false, true}) {
        Scene s;
        make_two_level(&s, moving);
        check_plan(s, moving ? "two levels, one instance moving" : "two levels");
    }
    check_refusals_of_the_box();
    check_refusals_of_shapes();
    check_too_deep_tree();
    check_refusals_of_two_levels();
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
