// host_lobes.h — the lobe list (the reference's BSDF, reflection.rs:207-449) of any material row description, on the host.
// One function per description, all ending in the same LobeList; host_edit.cpp's lobe_row_of_desc (the host half of
// pbrt_hip_scene_set_lobe_material) and the context-free pbrt_hip_material_lobes (include/pbrt_hip.h) call them. The rules that turn a PbrtMaterial / PbrtMaterialDesc into a
// DevMaterial row live here as well, so that the scene and the listing cannot disagree. No device code.
#pragma once
#include <algorithm>
#include <cmath>

#include "scene.h"

namespace pb {

// TrowbridgeReitzDistribution::roughness_to_alpha (microfacet.rs:160-169), in double, rounded once
inline float roughness_to_alpha(float roughness) {
    double x = std::log(std::max((double)roughness, 1e-3));
    return (float)(1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x * x * x + 0.000640711 * x * x * x * x);
}
// Roughness of a plastic / metal material: finite, >= 0, and > 0 when it is taken as alpha unchanged (remap off)
inline const char* roughness_invalid(float u, float v, bool remap) {
    if (!std::isfinite(u) || !std::isfinite(v) || u < 0.0f || v < 0.0f) return "roughness must be finite and >= 0";
    if (!remap && (u == 0.0f || v == 0.0f)) return "roughness 0 without remapping (alpha 0)";
    return nullptr;
}
// The one place materials are checked (scene creation); nullptr when the material is usable
const char* material_invalid(const PbrtMaterial& m);
// the DevMaterial row of a PbrtMaterial (scene creation) and of a PbrtMaterialDesc (pbrt_hip_scene_set_material); the second
// returns why the descriptor is refused, or nullptr
DevMaterial row_of_material(const PbrtMaterial& m);
const char* row_of_desc(const PbrtMaterialDesc& d, DevMaterial* out);

struct LobeList {
    PbrtLobe lobes[kMaxLobes];
    int n = 0;
    float eta = 1.0f;  // BSDF::eta
};
// The list of a row of levels 0-2 (matte, mirror, plastic, metal, Oren-Nayar, rough glass, substrate; PBRT_MAT_NONE: no lobe).
// Refused (the reason is returned): smooth glass, whose lobes depend on the integrator, and Disney / lobe rows.
const char* lobes_of_row(const DevMaterial& m, LobeList* out);
// UberMaterial / TranslucentMaterial / MixMaterial (uber.cpp, translucent.cpp, mixmat.cpp). a, b: the operands' lists of a mix.
const char* lobes_of_lobe_desc(const PbrtLobeMaterialDesc& d, const LobeList* a, const LobeList* b, LobeList* out);
// the device form of a list
DevLobeRow lobe_row_of(const LobeList& l);

}  // namespace pb
