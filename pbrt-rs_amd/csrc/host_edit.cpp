// host_edit.cpp — scene edits on the host (host_edit.h). No device call: every function here maps a descriptor and the scene's
// host copies to the bytes an edit writes, or to the reason it is refused.
#include "host_edit.h"

#include <cstring>

#include "abi_guard.h"
#include "host_scene.h"

namespace pb {

const char* roughness_row(const DevMaterial& m, float u, float v, bool remap, DevMaterial* out) {
    if (m.type == kMatHair) return "a hair row has no roughness: pbrt_hip_scene_set_hair_material sets beta_m and beta_n";
    if (m.type != PBRT_MAT_PLASTIC && m.type != PBRT_MAT_METAL) return "material is not PBRT_MAT_PLASTIC or PBRT_MAT_METAL";
    if (const char* why = roughness_invalid(u, v, remap)) return why;
    if (m.type == PBRT_MAT_PLASTIC && u != v) return "plastic is isotropic: u_roughness must equal v_roughness";
    *out = m;
    out->alpha_u = remap ? roughness_to_alpha(u) : u;
    out->alpha_v = remap ? roughness_to_alpha(v) : v;
    return nullptr;
}

std::string disney_of_desc(const PbrtDisneyDesc& p, DevDisney* block, DevMaterial* row) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p.color[k]) || p.color[k] < 0.0f) return "color must be finite and >= 0";
    const struct {
        const char* name;
        float v, max;
    } scalars[] = {{"metallic", p.metallic, 1.0f}, {"eta", p.eta, INFINITY}, {"roughness", p.roughness, 1.0f},
                   {"specular_tint", p.specular_tint, 1.0f}, {"anisotropic", p.anisotropic, 1.0f}, {"sheen", p.sheen, INFINITY},
                   {"sheen_tint", p.sheen_tint, 1.0f}, {"clearcoat", p.clearcoat, INFINITY}, {"clearcoat_gloss", p.clearcoat_gloss, 1.0f},
                   {"spec_trans", p.spec_trans, 1.0f}, {"flatness", p.flatness, 1.0f}, {"diff_trans", p.diff_trans, 2.0f}};
    for (const auto& sv : scalars) {
        if (!std::isfinite(sv.v) || sv.v < 0.0f) return std::string(sv.name) + " must be finite and >= 0";
        if (sv.v > sv.max) return std::string(sv.name) + (sv.max == 2.0f ? " must be <= 2" : " must be <= 1");
    }
    if (!(p.eta > 0.0f)) return "eta must be > 0";

    const bool thin = p.thin != 0;
    const double c[3] = {p.color[0], p.color[1], p.color[2]};
    const double lum = 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2];
    const double metallic = p.metallic, eta = p.eta, rough = p.roughness, strans = p.spec_trans, flat = p.flatness;
    const double dw = (1.0 - metallic) * (1.0 - strans), dt = p.diff_trans / 2.0;
    const double aspect = std::sqrt(1.0 - 0.9 * p.anisotropic);
    const double r0 = ((eta - 1.0) / (eta + 1.0)) * ((eta - 1.0) / (eta + 1.0));
    auto lerp = [](double t, double a, double b) { return (1.0 - t) * a + t * b; };
    DevDisney z{};
    z.metallic = p.metallic;
    z.eta = p.eta;
    z.roughness = p.roughness;
    z.ax = (float)std::max(1e-3, rough * rough / aspect);
    z.ay = (float)std::max(1e-3, rough * rough * aspect);
    z.tax = z.ax;
    z.tay = z.ay;
    z.sep_trans = thin ? 0 : 1;
    z.lobes = kDzMicro;
    if (dw > 0.0) z.lobes |= kDzDiffuse | kDzRetro | (thin ? kDzFakeSS : 0) | (p.sheen > 0.0f ? kDzSheen : 0);
    if (p.clearcoat > 0.0f) z.lobes |= kDzClearcoat;
    if (p.spec_trans > 0.0f) z.lobes |= kDzTrans;
    if (thin) z.lobes |= kDzLambertT;
    for (int k = 0; k < 3; ++k) {
        const double tint = lum > 0.0 ? c[k] / lum : 1.0;
        z.cspec0[k] = (float)lerp(metallic, r0 * lerp(p.specular_tint, 1.0, tint), c[k]);
        if (z.lobes & kDzDiffuse) z.diffuse[k] = (float)(thin ? dw * (1.0 - flat) * (1.0 - dt) * c[k] : dw * c[k]);
        if (z.lobes & kDzFakeSS) z.fakess[k] = (float)(dw * flat * (1.0 - dt) * c[k]);
        if (z.lobes & kDzRetro) z.retro[k] = (float)(dw * c[k]);
        if (z.lobes & kDzSheen) z.sheen[k] = (float)(dw * p.sheen * lerp(p.sheen_tint, 1.0, tint));
        if (z.lobes & kDzTrans) z.trans[k] = (float)(strans * std::sqrt(c[k]));
        if (z.lobes & kDzLambertT) z.lambert_t[k] = (float)(dt * c[k]);
    }
    {
        const double g = lerp(p.clearcoat_gloss, 0.1, 0.001), a2 = g * g;
        z.clearcoat = p.clearcoat;
        z.cc_a2 = (float)a2;
        z.cc_ln_a2 = (float)std::log(a2);
        z.cc_norm = (float)((a2 - 1.0) / (3.14159265358979323846 * std::log(a2)));
    }
    if ((z.lobes & kDzTrans) && thin) {
        const double rs = (0.65 * eta - 0.35) * rough;
        z.tax = (float)std::max(1e-3, rs * rs / aspect);
        z.tay = (float)std::max(1e-3, rs * rs * aspect);
    }
    z.n = __builtin_popcount((unsigned)z.lobes);
    DevMaterial m{};
    m.type = kMatDisney;
    std::memcpy(m.kd, p.color, 12);
    m.eta = p.eta;
    *block = z;
    *row = m;
    return "";
}

std::string hair_of_desc(const PbrtHairDesc& p, DevHair* block, DevMaterial* row) {
    const float fields[] = {p.sigma_a[0], p.sigma_a[1], p.sigma_a[2], p.color[0], p.color[1], p.color[2], p.eumelanin, p.pheomelanin,
                            p.eta, p.beta_m, p.beta_n, p.alpha};
    for (float f : fields)
        if (!std::isfinite(f)) return "every field must be finite";
    if (p.beta_m < 0.0f || p.beta_m > 1.0f) return "beta_m must be in [0, 1]";
    if (p.beta_n < 0.0f || p.beta_n > 1.0f) return "beta_n must be in [0, 1]";
    if (!(p.eta > 0.0f)) return "eta must be > 0";
    const double bm = p.beta_m, bn = p.beta_n, pi = 3.14159265358979323846;
    double sigma_a[3];
    if (p.absorption == PBRT_HAIR_SIGMA_A) {
        for (int k = 0; k < 3; ++k) {
            if (p.sigma_a[k] < 0.0f) return "sigma_a must be >= 0";
            sigma_a[k] = p.sigma_a[k];
        }
    } else if (p.absorption == PBRT_HAIR_COLOR) {
        const double d = 5.969 - 0.215 * bn + 2.532 * std::pow(bn, 2) - 10.73 * std::pow(bn, 3) + 5.574 * std::pow(bn, 4) + 0.245 * std::pow(bn, 5);
        for (int k = 0; k < 3; ++k) {
            if (!(p.color[k] > 0.0f && p.color[k] <= 1.0f)) return "color must be in (0, 1]";
            const double q = std::log((double)p.color[k]) / d;
            sigma_a[k] = q * q;
        }
    } else if (p.absorption == PBRT_HAIR_MELANIN) {
        if (p.eumelanin < 0.0f || p.pheomelanin < 0.0f) return "eumelanin and pheomelanin must be >= 0";
        const double eu[3] = {0.419, 0.697, 1.37}, ph[3] = {0.187, 0.4, 1.05};
        for (int k = 0; k < 3; ++k) sigma_a[k] = (double)p.eumelanin * eu[k] + (double)p.pheomelanin * ph[k];
    } else {
        return "unknown absorption (PBRT_HAIR_SIGMA_A, PBRT_HAIR_COLOR or PBRT_HAIR_MELANIN)";
    }
    DevHair z{};
    for (int k = 0; k < 3; ++k) z.sigma_a[k] = (float)sigma_a[k];
    z.eta = p.eta;
    const double q = 0.726 * bm + 0.812 * bm * bm + 3.7 * std::pow(bm, 20);
    const double v0 = q * q;
    z.v[0] = (float)v0;
    z.v[1] = (float)(0.25 * v0);
    z.v[2] = (float)(4.0 * v0);
    z.v[3] = z.v[2];
    const double s = std::sqrt(pi / 8.0) * (0.265 * bn + 1.194 * bn * bn + 5.372 * std::pow(bn, 22));
    z.s = (float)s;
    double sk[3], ck[3];
    sk[0] = std::sin((double)p.alpha * (pi / 180.0));
    ck[0] = std::sqrt(std::max(0.0, 1.0 - sk[0] * sk[0]));
    for (int i = 1; i < 3; ++i) {
        sk[i] = 2.0 * ck[i - 1] * sk[i - 1];
        ck[i] = ck[i - 1] * ck[i - 1] - sk[i - 1] * sk[i - 1];
    }
    for (int i = 0; i < 3; ++i) {
        z.sin2k[i] = (float)sk[i];
        z.cos2k[i] = (float)ck[i];
    }
    // the trimmed logistic over [-pi, pi]: at s == 0 (beta_n == 0) the cdfs are 0 and 1
    const double lo = s > 0.0 ? 1.0 / (1.0 + std::exp(pi / s)) : 0.0, hi = s > 0.0 ? 1.0 / (1.0 + std::exp(-pi / s)) : 1.0;
    z.cdf_lo = (float)lo;
    z.trim_k = (float)(hi - lo);
    DevMaterial m{};
    m.type = kMatHair;
    m.eta = p.eta;
    *block = z;
    *row = m;
    return "";
}

std::string lobe_row_of_desc(const PbrtLobeMaterialDesc& d, const LobeTables& t, DevLobeRow* lobe_row, DevMaterial* row) {
    if (t.general_shapes) return "scenes with general quadric shapes take no lobe rows (their shading builds stay at level 3)";
    if (t.light_maps) return "scenes with a projection or goniometric light take no lobe rows (their shading builds stay at level 3)";
    if (t.moving) return "scenes with moving instances take no lobe rows";
    LobeList la, lb, L;
    if (d.type == PBRT_LOBEMAT_MIX) {
        const int32_t ops[2] = {d.material_a, d.material_b};
        LobeList* lists[2] = {&la, &lb};
        for (int k = 0; k < 2; ++k) {
            const std::string name = k ? "material_b" : "material_a";
            if (ops[k] < 0 || ops[k] >= (int32_t)t.materials.size()) return name + " out of range";
            const DevMaterial& om = t.materials[ops[k]];
            if (om.type == kMatLobes) {
                if (t.lobe_origin[ops[k]] == PBRT_LOBEMAT_MIX) return name + " is a mix row";
                const DevLobeRow& r = t.lobe_rows[ops[k]];
                lists[k]->n = r.n;
                lists[k]->eta = r.eta;
                for (int i = 0; i < r.n; ++i) lists[k]->lobes[i] = r.lobes[i];
            } else if (const char* why = lobes_of_row(om, lists[k])) {
                return name + ": " + why;
            }
        }
    }
    if (const char* why = lobes_of_lobe_desc(d, &la, &lb, &L)) return why;
    *lobe_row = lobe_row_of(L);
    *row = DevMaterial{};
    row->type = kMatLobes;
    row->eta = L.eta;
    return "";
}

const char* envmap_transform(const float m[16], DevEnvMap* e) {
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return "light_to_world is not finite";
    if (m[12] != 0.0f || m[13] != 0.0f || m[14] != 0.0f || m[15] != 1.0f) return "light_to_world's last row is not (0, 0, 0, 1)";
    // world_to_light's directions: the inverse of the upper 3x3, in double
    double a[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[3 * r + c] = m[4 * r + c];
    double inv[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                     a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                     a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    double det = a[0] * inv[0] + a[1] * inv[3] + a[2] * inv[6];
    for (int k = 0; k < 9; ++k) {
        e->l2w[k] = (float)a[k];
        e->w2l[k] = det != 0.0 ? (float)(inv[k] / det) : 0.0f;
        if (det == 0.0 || !std::isfinite(e->w2l[k])) return "light_to_world is singular";
    }
    return nullptr;
}

static float y_value(const float p[3]) { return 0.212671f * p[0] + 0.715160f * p[1] + 0.072169f * p[2]; }
float envmap_power_y(const EnvTables& t, float world_radius) {
    const float scale = kPi * world_radius * world_radius;
    const float p[3] = {t.power_rgb[0] * scale, t.power_rgb[1] * scale, t.power_rgb[2] * scale};
    return y_value(p);
}
float light_map_power_y(const LightMapTables& t, const float L[3]) {
    const float p[3] = {L[0] * t.power_rgb[0], L[1] * t.power_rgb[1], L[2] * t.power_rgb[2]};
    return y_value(p);
}

std::vector<float4> texels_of_rgb(const std::vector<float>& rgb) {
    std::vector<float4> texels(rgb.size() / 3);
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    return texels;
}

PowerEdit power_edit(const std::vector<DevLight>& lights, int n, int light, float power_y) {
    PowerEdit e;
    e.func.resize(n);
    e.old_func.resize(n);
    for (int i = 0; i < n; ++i) {
        e.old_func[i] = lights[i].power_y;
        e.func[i] = i == light ? power_y : e.old_func[i];
    }
    make_distribution(e.func, &e.cdf, &e.func_int);
    make_distribution(e.old_func, &e.old_cdf, &e.old_func_int);
    return e;
}

}  // namespace pb

// the constants of a hair row without a scene (include/pbrt_hip.h)
extern "C" int pbrt_hip_hair_tables(const PbrtHairDesc* desc, PbrtHairTables* out, const char** reason) try {
    static thread_local std::string why;
    if (reason) *reason = nullptr;
    pb::DevHair z;
    pb::DevMaterial m;
    why = (desc && out) ? pb::hair_of_desc(*desc, &z, &m) : std::string("null pointer");
    if (!why.empty()) {
        if (reason) *reason = why.c_str();
        return PBRT_HIP_ERR_INVALID;
    }
    std::memcpy(out->sigma_a, z.sigma_a, 12);
    out->eta = z.eta;
    std::memcpy(out->v, z.v, 16);
    out->s = z.s;
    std::memcpy(out->sin2k, z.sin2k, 12);
    std::memcpy(out->cos2k, z.cos2k, 12);
    return PBRT_HIP_OK;
}
PB_ABI_CATCH
