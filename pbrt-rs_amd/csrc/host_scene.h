// host_scene.h — scene creation on the host: one description of the call (SceneDesc), every check that needs no device
// (scene_invalid) and every table the scene uploads (plan_scene, plan_two_level_wide). Implemented in host_scene.cpp, which
// makes no device call; pbrt_hip.hip's upload_scene puts a plan on the device. Scene::new (src/core/scene.rs:18-34).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "motion.h"
#include "scene.h"

namespace pb {

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
// Two-level scenes: the mesh of the SceneDesc is then the COMBINED mesh (every object's triangles, object after object,
// then the world-space triangles) and prim_order the combined leaf order (object k's leaf order at obj_tri_offset[k],
// world triangles in caller order at world_tri_offset).
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

// What every pbrt_hip_scene_create* entry point asks for. An aggregate: the entry points list the fields in this order.
struct SceneDesc {
    const float* positions = nullptr;
    int32_t n_verts = 0;
    const int32_t* indices = nullptr;
    int32_t n_tris = 0;
    const int32_t* tri_material = nullptr;
    const PbrtMaterial* materials = nullptr;
    int32_t n_materials = 0;
    const int32_t* tri_light = nullptr;
    const PbrtLight* lights = nullptr;
    int32_t n_lights = 0;
    // the tree over the primitives in reference order; two-level scenes: nodes == nullptr, n_nodes the objects' total
    const PbrtLinearBVHNode* nodes = nullptr;
    int32_t n_nodes = 0;
    const int32_t* prim_order = nullptr;
    SphereArgs sa;
    InstancingArgs ia;
    // pbrt_hip_scene_create_hlbvh: the tree, the triangle records and the leaf order are made on the device and nodes /
    // prim_order are unused. dt is null while the checks run before the build and names the built tree afterwards.
    bool device_tree = false;
    DeviceTree* dt = nullptr;
    // curve segments behind the shapes (pbrt_hip_scene_create_with_curves): primitive ids n_tris + n_shapes .. + n_curves - 1
    const PbrtCurve* curves = nullptr;
    int32_t n_curves = 0;

    int32_t n_prims() const { return n_tris + sa.n + sa.n_shapes + n_curves; }
    bool instanced() const { return ia.n_instances > 0; }
    int32_t n_top() const { return ia.n_instances + ia.n_world_tris; }  // primitives of the top-level aggregate
};

// Every check of scene creation that needs no device, in the order scene creation has always met them; the message for
// pbrt_hip_last_error, empty when the description is fine.
std::string scene_invalid(const SceneDesc& desc);

// What pbrt_hip_scene_create_two_level_moving is called with, in its order (the other two-level entry points leave out a part)
struct TwoLevelArgs {
    const PbrtObject* objects;
    int32_t n_objects;
    const PbrtInstance* instances;
    const PbrtInstanceMotion* motions;
    const int32_t* instance_object;
    int32_t n_instances;
    const float* world_positions;
    int32_t n_world_verts;
    const int32_t* world_indices;
    int32_t n_world_tris;
    const int32_t *world_tri_material, *world_tri_light;
    const PbrtMaterial* materials;
    int32_t n_materials;
    const PbrtLight* lights;
    int32_t n_lights;
    const PbrtLinearBVHNode* tlas_nodes;
    int32_t n_tlas_nodes;
    const int32_t* tlas_order;
};
// The combined mesh of a two-level scene (InstancingArgs above), owned: what the SceneDesc of such a scene points at
struct CombinedMesh {
    std::vector<float> pos;
    std::vector<int32_t> idx, mat, lgt, order;  // lgt: -1 on object triangles; order: the combined leaf order
    int32_t n_nodes = 0;                        // the objects' total
    InstancingArgs ia;
};
// Checks the arguments that become subscripts here and concatenates the meshes; nullptr, or the refusal (*out unspecified then)
const char* combine_two_level(const TwoLevelArgs& a, CombinedMesh* out);

// Validates one reference-order LinearBVHNode array (nullptr, or the refusal) ...
// force_count_bits >= 0: the width of (n_primitives - 1) in the leaf references (several object trees share one width);
// n_slots_total >= 0: the leaf slots of the whole scene, where the tree is one of several.
const char* tree_invalid(const PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t n_prims, int force_count_bits = -1,
                         int64_t n_slots_total = -1, int* depth = nullptr);
// ... and converts a valid one to the device records (trace.h), appended to *inodes (16 floats each): interior nodes get
// indices base + 0.. in DFS order, leaves are encoded with count_bits. slot_base: leaf slot of the tree's first primitive
// in the scene's slot numbering.
struct TreeLayout {
    int n_interior = 0, count_bits = 0;
    int32_t root_ref = 0;
};
TreeLayout convert_tree(const PbrtLinearBVHNode* nodes, int32_t n_nodes, int32_t base, std::vector<float>* inodes,
                        int32_t slot_base = 0, int force_count_bits = -1);

float tri_area(const float* a, const float* b, const float* c);  // triangle.rs:323-328
// Distribution1D::new (sampling.rs:69-93), intended (D40)
void make_distribution(const std::vector<float>& f, std::vector<float>* cdf, float* func_int);

// Everything a valid description puts on the device, as host arrays. With desc.dt the plan leaves out what the device
// builder already made (interior and triangle records, prim_slot; area lights take their slot from dt->light_slot).
struct ScenePlan {
    DevSceneData d;  // every field that is no device pointer; upload_scene fills the pointers in
    int n_interior = 0;
    std::vector<float> inodes;       // 64-B interior records: the top-level tree's, then the objects'
    std::vector<float> tris;         // 48-B triangle / sphere / shape records in leaf order
    std::vector<int32_t> prim_slot;  // primitive -> leaf slot
    std::vector<DevShape> shapes;    // theta_min / theta_max are k_shape_angles'
    std::vector<DevCurve> curves;    // one row per curve record
    std::vector<uint8_t> row_off_curve;  // scenes with curves, per material row: a triangle or a quadric shape names it
    std::vector<DevLight> lights;    // max(1, n_lights) rows
    std::vector<int> infinite_ids;
    std::vector<DevMaterial> materials;
    bool glossy = false;
    bool light_maps = false;
    std::vector<DevLightMap> light_map_rows;  // [n_lights] when light_maps
    std::vector<float> light_fov;
    std::vector<int> light_samples;
    std::vector<float> uniform_func, uniform_cdf, power_func, power_cdf;  // light sampling distributions (n_lights > 0)
    // two-level scenes
    std::vector<float> objects;           // per object: (root box min, root reference) (root box max, -)
    std::vector<int32_t> obj_root_ref;
    std::vector<float> top_slot_records;  // 28 floats per top-level leaf slot
    std::vector<int32_t> slot_inst;       // top-level leaf slot -> instance, -1 for a world-space triangle
    std::vector<DevMotion> motions;       // by top-level leaf slot; empty when nothing moves
    std::vector<int32_t> slot_prim;       // leaf slot -> triangle index inside its own object (world triangles: their own list)
};
void plan_scene(const SceneDesc& desc, ScenePlan* plan);

// The 4-wide records of a two-level scene (host_wide.cpp) in the device arrays' form: the top-level tree's records first
// (its leaves keep their exact boxes and name top-level primitives in wide order), then every object aggregate's; one
// triangle / leaf-box array for all objects.
struct TwoLevelWide {
    std::vector<uint32_t> nodes;
    std::vector<float> tris, leaf_boxes, objects, top_slots, top_boxes;
    int32_t root_ref = 0, obj0_root = 0;
    int n_records = 0;
    int stack_need = 0;  // entries a ray can have on the stack below the top-level tree's root, both levels together
};
// nullptr, or the reason the scene keeps the binary records only
const char* plan_two_level_wide(const SceneDesc& desc, const ScenePlan& plan, TwoLevelWide* out);

}  // namespace pb
