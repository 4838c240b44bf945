// host_edit.h — scene edits on the host: what each pbrt_hip_scene_set_* entry point checks and computes before it touches the
// device, and the one rule by which an edit's writes reach the device tables (apply_writes). Implemented in host_edit.cpp, which
// makes no device call; pbrt_hip.hip's setters enter, call the function of their edit, list the writes, apply them and commit
// the host copies. tests/native/scene_edit_check.cpp runs all of it on a CPU.
#pragma once
#include <string>
#include <vector>

#include "host_envmap.h"
#include "host_lobes.h"

namespace pb {

// pbrt_hip_scene_set_material_roughness: row `m` with TrowbridgeReitzDistribution's alphas of (u, v), or why not
const char* roughness_row(const DevMaterial& m, float u, float v, bool remap, DevMaterial* out);

// pbrt-v3's DisneyMaterial without subsurface: the lobes' constants, computed in double and rounded once per
// field, and the kMatDisney row that names them. The refusal, or an empty string.
std::string disney_of_desc(const PbrtDisneyDesc& p, DevDisney* block, DevMaterial* row);

// pbrt-v3's HairMaterial: the absorption of the chosen parametrisation and the lobes' constants, computed in
// double and rounded once per field, and the kMatHair row that names them. The refusal, or an empty string. (What depends on the
// scene — it holds curves, and only curves name the row — is the setter's to check.)
std::string hair_of_desc(const PbrtHairDesc& p, DevHair* block, DevMaterial* row);

// The material tables' host copies as pbrt_hip_scene_set_lobe_material reads them: a mix copies its operands' lists as they are now
struct LobeTables {
    const std::vector<DevMaterial>& materials;
    const std::vector<DevLobeRow>& lobe_rows;
    const std::vector<int>& lobe_origin;
    bool general_shapes, light_maps, moving;  // scenes whose shading builds take no lobe rows
};
std::string lobe_row_of_desc(const PbrtLobeMaterialDesc& d, const LobeTables& t, DevLobeRow* lobe_row, DevMaterial* row);

// DevEnvMap::l2w / w2l of an affine light_to_world (row-major 4x4): the upper 3x3 and its inverse, in double; or why not
const char* envmap_transform(const float light_to_world[16], DevEnvMap* e);
// Light::power().y_value() of a light with a map: InfiniteAreaLight::power (infinite.rs:131-133) and D89
float envmap_power_y(const EnvTables& t, float world_radius);
float light_map_power_y(const LightMapTables& t, const float L[3]);
// rgb triples as the device's texels
std::vector<float4> texels_of_rgb(const std::vector<float>& rgb);

// What giving light `light` the power `power_y` does to the power distribution over lights[0, n): the arrays of
// DevSceneData::light_distrib_power after the edit and, for putting them back, as they are now
struct PowerEdit {
    std::vector<float> func, cdf, old_func, old_cdf;
    float func_int = 0.0f, old_func_int = 0.0f;
};
PowerEdit power_edit(const std::vector<DevLight>& lights, int n, int light, float power_y);

// One write of an edit: `bytes` at dst become `now`; `before` is what they hold (nullptr: a block nothing names until a later
// write of the same edit, with nothing to put back).
struct DeviceWrite {
    void* dst;
    const void* now;
    const void* before;
    size_t bytes;
};
enum class Applied {
    kDone,        // every write arrived
    kRolledBack,  // one failed and the previous values are back: the device names none of the edit's fresh arrays
    kTorn         // putting them back failed as well: the device may still name the fresh arrays, which must outlive the edit
};
// All of `writes` in order through copy(dst, src, bytes), which returns false and leaves its reason in *error on failure. After a
// failure every `before` is written, again in order and up to the first failure; *error keeps the FIRST failure's reason.
template <class Copy>
Applied apply_writes(const std::vector<DeviceWrite>& writes, Copy&& copy, std::string* error) {
    bool ok = true;
    for (size_t k = 0; ok && k < writes.size(); ++k) ok = copy(writes[k].dst, writes[k].now, writes[k].bytes);
    if (ok) return Applied::kDone;
    const std::string first = *error;
    ok = true;
    for (size_t k = 0; ok && k < writes.size(); ++k)
        if (writes[k].before) ok = copy(writes[k].dst, writes[k].before, writes[k].bytes);
    *error = first;
    return ok ? Applied::kRolledBack : Applied::kTorn;
}

}  // namespace pb
