// scene_edit_check.cpp — host-side check of the scene setters' host half (test infrastructure, built and run by
// tests/test_scene_edit_host.py under AddressSanitizer and UBSan; not part of the product library).
//
// Links the product's own pbrt-rs_amd/csrc/host_edit.cpp and host_scene.cpp with the host files they call and checks
//   - the message each function gives for the refusal inputs the GPU tests feed the pbrt_hip_scene_set_* entry points and the
//     two-level creation calls (the messages are written out here as the entry points have always given them; what the entry
//     points check themselves — a null scene or descriptor, a row or light index, a light's type — needs a scene);
//   - properties of what the functions compute that do not restate them: the Disney block's lobe mask and colours, the power
//     distribution before and after a light's edit, the environment map's transform, the combined mesh of a two-level scene;
//   - apply_writes over memcpy, with a writer that fails at the k-th call.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../pbrt-rs_amd/csrc/host_edit.h"
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

void expect(const std::string& got, const std::string& want, const char* what) {
    CHECK(got == want, "%s: expected \"%s\", got \"%s\"", what, want.c_str(), got.c_str());
}
void expect(const char* got, const std::string& want, const char* what) { expect(std::string(got ? got : ""), want, what); }

void rgb(float* c, float r, float g, float b) { c[0] = r, c[1] = g, c[2] = b; }
void grey(float* c, float v) { rgb(c, v, v, v); }

// ---- Disney: tests/disney_cases.py ----
PbrtDisneyDesc disney() {  // scenes.disney((0.8, 0.5, 0.3)): pbrt-v3's defaults
    PbrtDisneyDesc d{};
    rgb(d.color, 0.8f, 0.5f, 0.3f);
    d.eta = 1.5f;
    d.roughness = 0.5f;
    d.sheen_tint = 0.5f;
    d.clearcoat_gloss = 1.0f;
    d.diff_trans = 1.0f;
    return d;
}
std::string disney_refusal(const PbrtDisneyDesc& d) {
    pb::DevDisney z;
    pb::DevMaterial m;
    return pb::disney_of_desc(d, &z, &m);
}
void check_disney_refusals() {
    const float nan = NAN, inf = INFINITY;
    for (float bad : {-0.1f, nan, inf}) {
        PbrtDisneyDesc d = disney();
        d.color[bad == inf ? 0 : 1] = bad;
        expect(disney_refusal(d), "color must be finite and >= 0", "colour");
    }
    struct Scalar {
        const char* name;
        float PbrtDisneyDesc::*field;
        bool unit;  // bounded by 1
    };
    const Scalar scalars[] = {{"metallic", &PbrtDisneyDesc::metallic, true}, {"eta", &PbrtDisneyDesc::eta, false},
                              {"roughness", &PbrtDisneyDesc::roughness, true}, {"specular_tint", &PbrtDisneyDesc::specular_tint, true},
                              {"anisotropic", &PbrtDisneyDesc::anisotropic, true}, {"sheen", &PbrtDisneyDesc::sheen, false},
                              {"sheen_tint", &PbrtDisneyDesc::sheen_tint, true}, {"clearcoat", &PbrtDisneyDesc::clearcoat, false},
                              {"clearcoat_gloss", &PbrtDisneyDesc::clearcoat_gloss, true}, {"spec_trans", &PbrtDisneyDesc::spec_trans, true},
                              {"flatness", &PbrtDisneyDesc::flatness, true}, {"diff_trans", &PbrtDisneyDesc::diff_trans, false}};
    for (const Scalar& s : scalars) {
        for (float bad : {-0.25f, -1.5f, nan}) {
            PbrtDisneyDesc d = disney();
            d.*s.field = bad;
            expect(disney_refusal(d), std::string(s.name) + " must be finite and >= 0", s.name);
        }
        PbrtDisneyDesc d = disney();
        d.*s.field = s.unit ? 1.5f : inf;
        expect(disney_refusal(d), std::string(s.name) + (s.unit ? " must be <= 1" : " must be finite and >= 0"), s.name);
    }
    PbrtDisneyDesc d = disney();
    d.eta = 0.0f;
    expect(disney_refusal(d), "eta must be > 0", "eta 0");
    d = disney();
    d.diff_trans = 2.5f;
    expect(disney_refusal(d), "diff_trans must be <= 2", "diff_trans 2.5");
    // accepted where a neighbour is refused (ACCEPTED)
    for (int k = 0; k < 8; ++k) {
        d = disney();
        if (k == 0) d.sheen = 3.0f;
        if (k == 1) d.clearcoat = 2.5f;
        if (k == 2) d.diff_trans = 2.0f;
        if (k == 3) d.eta = 0.8f;
        if (k == 4) d.roughness = 0.0f;
        if (k == 5) d.metallic = d.spec_trans = 1.0f;
        if (k == 6) grey(d.color, 0.0f);
        if (k == 7) rgb(d.color, 2.0f, 1.5f, 1.0f);
        expect(disney_refusal(d), "", "accepted Disney descriptor");
    }
}

bool zero3(const float* c) { return c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f; }
void check_disney_block(const PbrtDisneyDesc& d, int want_lobes, const char* name) {
    pb::DevDisney z;
    pb::DevMaterial m;
    const std::string why = pb::disney_of_desc(d, &z, &m);
    CHECK(why.empty(), "%s: refused: %s", name, why.c_str());
    if (!why.empty()) return;
    CHECK(z.lobes == want_lobes, "%s: lobes %d, expected %d", name, z.lobes, want_lobes);
    CHECK(z.n == __builtin_popcount((unsigned)z.lobes), "%s: n %d", name, z.n);
    CHECK(m.type == pb::kMatDisney && std::memcmp(m.kd, d.color, 12) == 0 && m.eta == d.eta, "%s: the row", name);
    if (!d.thin) CHECK(z.tax == z.ax && z.tay == z.ay && z.sep_trans == 1, "%s: transmission alphas %g %g vs %g %g", name, z.tax, z.tay, z.ax, z.ay);
    const struct {
        int bit;
        const float* colour;
        const char* lobe;
    } colours[] = {{pb::kDzDiffuse, z.diffuse, "diffuse"}, {pb::kDzFakeSS, z.fakess, "fakess"}, {pb::kDzRetro, z.retro, "retro"},
                   {pb::kDzSheen, z.sheen, "sheen"}, {pb::kDzTrans, z.trans, "trans"}, {pb::kDzLambertT, z.lambert_t, "lambert_t"}};
    for (const auto& c : colours)
        if (!(z.lobes & c.bit)) CHECK(zero3(c.colour), "%s: colour of the unset lobe %s", name, c.lobe);
    for (int k = 0; k < 3; ++k) CHECK(std::isfinite(z.cspec0[k]), "%s: cspec0[%d] = %g", name, k, z.cspec0[k]);
    CHECK(std::isfinite(z.cc_norm) && z.cc_a2 > 0.0f && z.ax >= 1e-3f && z.ay >= 1e-3f, "%s: clearcoat / alphas", name);
}
void check_disney_blocks() {
    using namespace pb;
    PbrtDisneyDesc d = disney();
    check_disney_block(d, kDzDiffuse | kDzRetro | kDzMicro, "default");
    d.thin = 1;
    check_disney_block(d, kDzDiffuse | kDzFakeSS | kDzRetro | kDzMicro | kDzLambertT, "thin");
    d.spec_trans = 0.5f;
    check_disney_block(d, kDzDiffuse | kDzFakeSS | kDzRetro | kDzMicro | kDzTrans | kDzLambertT, "thin, spec_trans 0.5");
    {
        DevDisney z;
        DevMaterial m;
        disney_of_desc(d, &z, &m);  // thin: the transmission lobe's roughness is scaled by 0.65 eta - 0.35 = 0.625
        CHECK(std::fabs(z.tax / z.ax - 0.625f * 0.625f) < 1e-6f, "thin transmission alpha %g against %g", z.tax, z.ax);
    }
    d = disney();
    d.spec_trans = 0.5f;
    d.sheen = 1.0f;
    d.clearcoat = 1.0f;
    check_disney_block(d, kDzDiffuse | kDzRetro | kDzSheen | kDzMicro | kDzClearcoat | kDzTrans, "spec_trans 0.5, sheen, clearcoat");
    d.spec_trans = 1.0f;  // dw = 0: no diffuse side
    check_disney_block(d, kDzMicro | kDzClearcoat | kDzTrans, "spec_trans 1");
    d = disney();
    d.anisotropic = 1.0f;
    check_disney_block(d, kDzDiffuse | kDzRetro | kDzMicro, "anisotropic 1");
    {
        DevDisney z;
        DevMaterial m;
        disney_of_desc(d, &z, &m);  // aspect^2 = 1 - 0.9
        CHECK(std::fabs(z.ay / z.ax - 0.1f) < 1e-6f, "anisotropic alphas %g %g", z.ax, z.ay);
    }
    d = disney();
    grey(d.color, 0.0f);  // luminance 0: the tint is white, nothing divides by it
    check_disney_block(d, kDzDiffuse | kDzRetro | kDzMicro, "black");
}

// ---- roughness: tests/test_gpu_glossy.py::test_roughness_refusals_leave_the_scene_unchanged ----
PbrtMaterial material(int type, float kd, float kt, float eta) {
    PbrtMaterial m{};
    m.type = type;
    grey(m.kd, kd);
    grey(m.kt, kt);
    m.eta = eta;
    return m;
}
void check_roughness() {
    const pb::DevMaterial rows[3] = {pb::row_of_material(material(PBRT_MAT_PLASTIC, 0.3f, 0.5f, 0.2f)), pb::row_of_material(material(PBRT_MAT_METAL, 0.2f, 3.0f, 0.1f)),
                                     pb::row_of_material(material(PBRT_MAT_MATTE, 0.5f, 0.0f, 1.0f))};
    const struct {
        int row;
        float u, v;
        bool remap;
        const char* why;
    } cases[] = {{2, 0.1f, 0.1f, true, "material is not PBRT_MAT_PLASTIC or PBRT_MAT_METAL"},
                 {0, 0.1f, 0.2f, true, "plastic is isotropic: u_roughness must equal v_roughness"},
                 {1, -0.1f, 0.1f, true, "roughness must be finite and >= 0"},
                 {1, 0.1f, NAN, true, "roughness must be finite and >= 0"},
                 {0, INFINITY, INFINITY, false, "roughness must be finite and >= 0"},
                 {1, 0.0f, 0.1f, false, "roughness 0 without remapping (alpha 0)"},
                 {0, 0.0f, 0.0f, false, "roughness 0 without remapping (alpha 0)"}};
    for (const auto& c : cases) {
        pb::DevMaterial out = rows[c.row];
        expect(pb::roughness_row(rows[c.row], c.u, c.v, c.remap, &out), c.why, "roughness");
        CHECK(std::memcmp(&out, &rows[c.row], sizeof out) == 0, "a refused roughness wrote the row");
    }
    pb::DevMaterial out{};
    expect(pb::roughness_row(rows[1], 0.1f, 0.3f, true, &out), "", "anisotropic metal");
    CHECK(out.alpha_u == pb::roughness_to_alpha(0.1f) && out.alpha_v == pb::roughness_to_alpha(0.3f) && out.type == PBRT_MAT_METAL &&
              std::memcmp(out.kd, rows[1].kd, 28) == 0, "remapped alphas %g %g", out.alpha_u, out.alpha_v);
    expect(pb::roughness_row(rows[0], 0.25f, 0.25f, false, &out), "", "plastic, alpha as given");
    CHECK(out.alpha_u == 0.25f && out.alpha_v == 0.25f, "alphas as given %g %g", out.alpha_u, out.alpha_v);
}

// ---- pbrt_hip_scene_set_material's descriptors: tests/test_gpu_bxdfs.py::test_refusals_leave_the_scene_unchanged ----
PbrtMaterialDesc matte_sigma(float g, float sigma) {
    PbrtMaterialDesc d{};
    d.type = PBRT_MATDESC_MATTE;
    grey(d.kd, g);
    d.sigma = sigma;
    return d;
}
PbrtMaterialDesc rough_glass(float eta, float u, float v, bool remap = true) {
    PbrtMaterialDesc d{};
    d.type = PBRT_MATDESC_GLASS;
    grey(d.kr, 0.9f);
    grey(d.kt, 0.8f);
    d.eta = eta;
    d.u_roughness = u;
    d.v_roughness = v;
    d.remap_roughness = remap;
    return d;
}
PbrtMaterialDesc substrate(float u, float v, bool remap = true) {
    PbrtMaterialDesc d{};
    d.type = PBRT_MATDESC_SUBSTRATE;
    grey(d.kd, 0.5f);
    grey(d.ks, 0.5f);
    d.u_roughness = u;
    d.v_roughness = v;
    d.remap_roughness = remap;
    return d;
}
void check_material_descs() {
    pb::DevMaterial m;
    auto refused = [&](PbrtMaterialDesc d, const char* why) { expect(pb::row_of_desc(d, &m), why, why); };
    PbrtMaterialDesc d = matte_sigma(0.5f, 20.0f);
    d.type = 2;
    refused(d, "unknown material descriptor type");
    d.type = 7;
    refused(d, "unknown material descriptor type");
    d = matte_sigma(0.5f, 20.0f);
    d.kd[1] = -0.1f;
    refused(d, "Kd must be finite and >= 0");
    d.kd[1] = NAN;
    refused(d, "Kd must be finite and >= 0");
    refused(matte_sigma(0.5f, -1.0f), "sigma must be finite and >= 0");
    refused(matte_sigma(0.5f, INFINITY), "sigma must be finite and >= 0");
    d = rough_glass(1.5f, 0.2f, 0.2f);
    d.kr[0] = INFINITY;
    refused(d, "Kr must be finite and >= 0");
    d = rough_glass(1.5f, 0.2f, 0.2f);
    d.kt[2] = -1.0f;
    refused(d, "Kt must be finite and >= 0");
    for (float eta : {0.0f, -1.5f, NAN}) refused(rough_glass(eta, 0.2f, 0.2f), "glass needs a finite eta > 0");
    refused(rough_glass(1.5f, -0.2f, -0.2f), "roughness must be finite and >= 0");
    refused(rough_glass(1.5f, 0.2f, NAN), "roughness must be finite and >= 0");
    refused(rough_glass(1.5f, 0.0f, 0.2f, false), "roughness 0 without remapping (alpha 0)");
    d = substrate(0.2f, 0.2f);
    d.ks[0] = NAN;
    refused(d, "Ks must be finite and >= 0");
    d = substrate(0.2f, 0.2f);
    d.kd[0] = -0.5f;
    refused(d, "Kd must be finite and >= 0");
    refused(substrate(INFINITY, INFINITY), "roughness must be finite and >= 0");
    refused(substrate(0.0f, 0.0f, false), "roughness 0 without remapping (alpha 0)");
    refused(substrate(0.2f, 0.0f, false), "roughness 0 without remapping (alpha 0)");
    expect(pb::row_of_desc(matte_sigma(0.5f, 20.0f), &m), "", "Oren-Nayar");
    CHECK(m.type == pb::kMatOrenNayar, "sigma 20 is row type %d", m.type);
}

// ---- lobe rows: tests/lobe_cases.py's REFUSAL_ROWS, REFUSED and ACCEPTED ----
PbrtLobeMaterialDesc uber(float kd = 0.25f, float ks = 0.25f, float kr = 0.0f, float kt = 0.0f, float opacity = 1.0f) {
    PbrtLobeMaterialDesc d{};
    d.type = PBRT_LOBEMAT_UBER;
    grey(d.kd, kd);
    grey(d.ks, ks);
    grey(d.kr, kr);
    grey(d.kt, kt);
    grey(d.opacity, opacity);
    d.eta = 1.5f;
    d.u_roughness = d.v_roughness = 0.1f;
    d.remap_roughness = 1;
    return d;
}
PbrtLobeMaterialDesc translucent(float kd = 0.25f, float ks = 0.25f) {
    PbrtLobeMaterialDesc d{};
    d.type = PBRT_LOBEMAT_TRANSLUCENT;
    grey(d.kd, kd);
    grey(d.ks, ks);
    grey(d.reflect, 0.5f);
    grey(d.transmit, 0.5f);
    d.u_roughness = d.v_roughness = 0.1f;
    d.remap_roughness = 1;
    return d;
}
PbrtLobeMaterialDesc mix(int a, int b, float amount) {
    PbrtLobeMaterialDesc d{};
    d.type = PBRT_LOBEMAT_MIX;
    d.material_a = a;
    d.material_b = b;
    grey(d.amount, amount);
    return d;
}
struct Tables {
    std::vector<pb::DevMaterial> materials;
    std::vector<pb::DevLobeRow> lobe_rows;
    std::vector<int> origin;
    pb::LobeTables view(bool shapes = false, bool maps = false, bool moving = false) const { return {materials, lobe_rows, origin, shapes, maps, moving}; }
    std::string set(int row, const PbrtLobeMaterialDesc& d) {  // as pbrt_hip_scene_set_lobe_material commits an accepted row
        pb::DevLobeRow r;
        pb::DevMaterial m;
        const std::string why = pb::lobe_row_of_desc(d, view(), &r, &m);
        if (why.empty()) materials[row] = m, lobe_rows[row] = r, origin[row] = d.type;
        return why;
    }
};
void check_lobe_rows() {
    // 0 matte, 1 metal, 2 smooth glass, 3 Disney, 4 a mix of 0 and 1, 5 uber with 5 lobes, 6 matte
    Tables t;
    const pb::DevMaterial matte = pb::row_of_material(material(PBRT_MAT_MATTE, 0.5f, 0.0f, 1.0f));
    t.materials.assign(7, matte);
    t.materials[1] = pb::row_of_material(material(PBRT_MAT_METAL, 0.2f, 3.0f, 0.1f));
    t.materials[2] = pb::row_of_material(material(PBRT_MAT_GLASS, 1.0f, 1.0f, 1.5f));
    pb::DevDisney z;
    expect(pb::disney_of_desc(disney(), &z, &t.materials[3]), "", "row 3");
    t.lobe_rows.assign(7, pb::DevLobeRow{});
    t.origin.assign(7, 0);
    expect(t.set(4, mix(0, 1, 0.5f)), "", "row 4");
    expect(t.set(5, uber(0.25f, 0.3f, 0.2f, 0.3f, 0.5f)), "", "row 5");
    CHECK(t.lobe_rows[4].n == 2 && t.lobe_rows[5].n == 5 && t.materials[5].type == pb::kMatLobes, "operand rows: %d and %d lobes", t.lobe_rows[4].n, t.lobe_rows[5].n);
    const Tables before = t;
    pb::DevLobeRow r;
    pb::DevMaterial m;
    auto refused = [&](PbrtLobeMaterialDesc d, const char* why) { expect(pb::lobe_row_of_desc(d, t.view(), &r, &m), why, why); };
    PbrtLobeMaterialDesc d = uber();
    d.type = 7;
    refused(d, "unknown lobe material type");
    d = uber();
    d.kd[1] = -0.1f;
    refused(d, "Kd must be finite and >= 0");
    d = uber();
    d.ks[0] = NAN;
    refused(d, "Ks must be finite and >= 0");
    d = uber();
    d.kr[0] = INFINITY;
    refused(d, "Kr must be finite and >= 0");
    refused(uber(0.25f, 0.25f, 0.0f, -1.0f), "Kt must be finite and >= 0");
    refused(uber(0.25f, 0.25f, 0.0f, 0.0f, -0.5f), "opacity must be finite and >= 0");
    for (float eta : {0.0f, NAN}) {
        d = uber();
        d.eta = eta;
        refused(d, "eta must be finite and > 0");
    }
    d = uber();
    d.u_roughness = -0.1f;
    refused(d, "roughness must be finite and >= 0");
    d = uber();
    d.v_roughness = INFINITY;
    refused(d, "roughness must be finite and >= 0");
    d = uber();
    d.u_roughness = 0.0f;
    d.remap_roughness = 0;
    refused(d, "roughness 0 without remapping (alpha 0)");
    d = translucent();
    grey(d.reflect, -0.1f);
    refused(d, "reflect must be finite and >= 0");
    d = translucent();
    grey(d.transmit, NAN);
    refused(d, "transmit must be finite and >= 0");
    refused(translucent(-1.0f), "Kd must be finite and >= 0");
    d = translucent();
    d.u_roughness = d.v_roughness = 0.0f;
    d.remap_roughness = 0;
    refused(d, "roughness 0 without remapping (alpha 0)");
    refused(mix(0, 1, -0.5f), "amount must be finite and >= 0");
    refused(mix(0, 1, NAN), "amount must be finite and >= 0");
    refused(mix(0, 7, 0.5f), "material_b out of range");
    refused(mix(-1, 0, 0.5f), "material_a out of range");
    refused(mix(3, 0, 0.5f), "material_a: a Disney row has no lobe list");
    refused(mix(0, 4, 0.5f), "material_b is a mix row");
    refused(mix(2, 0, 0.5f), "material_a: smooth glass has no one lobe list: FresnelSpecular under the path integrator, two specular lobes elsewhere; "
                             "an uber row with Kr, Kt gives smooth specular lobes");
    refused(mix(5, 5, 0.5f), "a mix of more than 8 lobes");
    // the scenes that take no lobe rows, in the order the entry point has always met them
    expect(pb::lobe_row_of_desc(uber(), t.view(true, true, true), &r, &m), "scenes with general quadric shapes take no lobe rows (their shading builds stay at level 3)", "shapes");
    expect(pb::lobe_row_of_desc(uber(), t.view(false, true, true), &r, &m),
           "scenes with a projection or goniometric light take no lobe rows (their shading builds stay at level 3)", "map lights");
    expect(pb::lobe_row_of_desc(uber(), t.view(false, false, true), &r, &m), "scenes with moving instances take no lobe rows", "moving");
    CHECK(std::memcmp(t.materials.data(), before.materials.data(), 7 * sizeof(pb::DevMaterial)) == 0, "a refusal wrote the tables");
    // accepted where a neighbour is refused: no microfacet lobe carries the zero alpha
    d = uber(0.25f, 0.0f);
    d.u_roughness = 0.0f;
    d.remap_roughness = 0;
    expect(t.set(6, d), "", "uber without Ks at roughness 0");
    d = translucent(0.25f, 0.0f);
    d.u_roughness = d.v_roughness = 0.0f;
    d.remap_roughness = 0;
    expect(t.set(6, d), "", "translucent without Ks at roughness 0");
    expect(t.set(6, mix(5, 0, 0.5f)), "", "a mix of 5 + 1 lobes");
    CHECK(t.lobe_rows[6].n == 6 && t.materials[6].eta == t.lobe_rows[5].eta && t.origin[6] == PBRT_LOBEMAT_MIX, "mix of rows 5 and 0: %d lobes", t.lobe_rows[6].n);
    for (int i = 0; i < 5; ++i) CHECK(t.lobe_rows[6].lobes[i].kind == t.lobe_rows[5].lobes[i].kind && t.lobe_rows[6].lobes[i].scale[0] == 0.5f, "mix lobe %d", i);
}

// ---- maps: tests/test_gpu_envmap.py::test_refusals_leave_the_scene_usable, test_gpu_light_maps.py's refusals ----
void check_maps() {
    float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    pb::DevEnvMap e{};
    expect(pb::envmap_transform(m, &e), "", "identity");
    float sing[16];
    std::memcpy(sing, m, 64);
    std::memcpy(sing + 8, sing, 12);  // row 2 = row 0
    expect(pb::envmap_transform(sing, &e), "light_to_world is singular", "singular");
    float bad[16];
    std::memcpy(bad, m, 64);
    bad[14] = 0.5f;
    expect(pb::envmap_transform(bad, &e), "light_to_world's last row is not (0, 0, 0, 1)", "last row");
    for (float& v : bad) v = NAN;
    expect(pb::envmap_transform(bad, &e), "light_to_world is not finite", "NaN matrix");
    std::memcpy(bad, m, 64);
    bad[5] = INFINITY;
    expect(pb::envmap_transform(bad, &e), "light_to_world is not finite", "infinite entry");
    // a rotation about (1, 2, 3) with a translation, which the map ignores
    const double ax[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)}, c = std::cos(0.7), s = std::sin(0.7);
    float rot[16] = {0, 0, 0, 5, 0, 0, 0, -6, 0, 0, 0, 7, 0, 0, 0, 1};
    const double cross[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) rot[4 * r + k] = (float)((r == k ? c : 0.0) + s * cross[3 * r + k] + (1 - c) * ax[r] * ax[k]);
    expect(pb::envmap_transform(rot, &e), "", "rotation");
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            double sum = 0;
            for (int j = 0; j < 3; ++j) sum += (double)e.w2l[3 * r + j] * e.l2w[3 * j + k];
            CHECK(std::fabs(sum - (r == k)) < 4e-7, "w2l l2w [%d][%d] = %.9g", r, k, sum);
            CHECK(e.l2w[3 * r + k] == rot[4 * r + k], "l2w[%d][%d]", r, k);
        }
    // the texels
    const float L[3] = {1, 1, 1};
    std::vector<float> ok(4 * 4 * 3, 1.0f), nan = ok, neg = ok;
    nan[(1 * 4 + 2) * 3] = NAN;
    neg[(3 * 4 + 3) * 3 + 2] = -1.0f;
    pb::EnvTables et;
    pb::LightMapTables lt;
    expect(pb::envmap_build(nan.data(), 4, 4, L, &et), "texels must be finite and >= 0", "NaN texel");
    expect(pb::envmap_build(neg.data(), 4, 4, L, &et), "texels must be finite and >= 0", "negative texel");
    for (int type : {PBRT_LIGHT_PROJECTION, PBRT_LIGHT_GONIOMETRIC}) {
        expect(pb::light_map_build(type, 60.0f, nan.data(), 4, 4, &lt), "texels must be finite and >= 0", "NaN texel");
        expect(pb::light_map_build(type, 60.0f, neg.data(), 4, 4, &lt), "texels must be finite and >= 0", "negative texel");
        expect(pb::light_map_build(type, 60.0f, ok.data(), 0, 4, &lt), "width and height must be >= 1", "width 0");
        expect(pb::light_map_build(type, 60.0f, ok.data(), 4, -2, &lt), "width and height must be >= 1", "height -2");
        expect(pb::light_map_build(type, 60.0f, ok.data(), 1 << 14, 1 << 14, &lt), "the map's sampling table would pass 2^28 texels", "2^14 x 2^14");
    }
    // a 4 x 2 map of distinct texels: the texels as the device reads them, and each light's power
    std::vector<float> map(4 * 2 * 3);
    for (size_t i = 0; i < map.size(); ++i) map[i] = 0.25f + 0.125f * (float)i;
    expect(pb::envmap_build(map.data(), 4, 2, L, &et), "", "4 x 2 environment map");
    const std::vector<float4> texels = pb::texels_of_rgb(et.level0);
    CHECK(texels.size() == (size_t)et.w * et.h && et.w == 4 && et.h == 2, "%zu texels of a %d x %d map", texels.size(), et.w, et.h);
    for (size_t i = 0; i < texels.size(); ++i)
        CHECK(texels[i].x == et.level0[3 * i] && texels[i].y == et.level0[3 * i + 1] && texels[i].z == et.level0[3 * i + 2] && texels[i].w == 0.0f, "texel %zu", i);
    const float y1 = pb::envmap_power_y(et, 1.0f), y2 = pb::envmap_power_y(et, 2.0f);
    CHECK(y1 > 0.0f && std::fabs(y2 / y1 - 4.0f) < 1e-6f, "environment power %g at r = 1, %g at r = 2", y1, y2);
    expect(pb::light_map_build(PBRT_LIGHT_GONIOMETRIC, 0.0f, map.data(), 4, 2, &lt), "", "4 x 2 light map");
    const float I1[3] = {1, 1, 1}, I3[3] = {3, 3, 3};
    CHECK(pb::light_map_power_y(lt, I1) > 0.0f && std::fabs(pb::light_map_power_y(lt, I3) / pb::light_map_power_y(lt, I1) - 3.0f) < 1e-6f, "light map power");
}

// ---- the power distribution under an edit ----
void check_power_edit(const std::vector<float>& power, int light, float now) {
    const int n = (int)power.size();
    std::vector<pb::DevLight> lights(n + 1, pb::DevLight{});  // the scene keeps max(1, n) rows: one more than n is read by nobody
    for (int i = 0; i < n; ++i) lights[i].power_y = power[i];
    lights[n].power_y = NAN;
    const pb::PowerEdit e = pb::power_edit(lights, n, light, now);
    std::vector<float> old_cdf;
    float old_int;
    pb::make_distribution(power, &old_cdf, &old_int);
    CHECK(e.old_func == power && e.old_cdf == old_cdf && e.old_func_int == old_int, "the old arrays are not the input's");
    CHECK((int)e.func.size() == n && (int)e.cdf.size() == n + 1, "sizes %zu %zu", e.func.size(), e.cdf.size());
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(std::memcmp(&e.func[i], i == light ? &now : &power[i], 4) == 0, "func[%d] = %g", i, e.func[i]);
        CHECK(e.cdf[i + 1] >= e.cdf[i], "cdf falls at %d", i);
        sum += e.func[i];
    }
    CHECK(e.cdf[0] == 0.0f && e.cdf[n] == 1.0f, "cdf runs from %g to %g", e.cdf[0], e.cdf[n]);
    CHECK(std::fabs(e.func_int - sum / n) <= 1e-6 * (sum / n), "func_int %g, mean %g", e.func_int, sum / n);
    if (sum == 0.0)  // Distribution1D::new's all-zero case: the uniform cdf
        for (int i = 0; i <= n; ++i) CHECK(e.cdf[i] == (float)i / (float)n, "all-zero cdf[%d] = %g", i, e.cdf[i]);
}

// ---- apply_writes over memcpy ----
struct Writer {
    int calls = 0, fail_at = -1, fail_again_at = -1;
    std::string error;
    bool operator()(void* dst, const void* src, size_t bytes) {
        const int k = calls++;
        if (k == fail_at || k == fail_again_at) {
            error = "write " + std::to_string(k) + " failed";
            return false;
        }
        std::memcpy(dst, src, bytes);
        return true;
    }
};
void check_apply_writes() {
    const int32_t before[4][3] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}, {10, 11, 12}}, now[4][3] = {{-1, -2, -3}, {-4, -5, -6}, {-7, -8, -9}, {-10, -11, -12}};
    const size_t bytes[4] = {12, 4, 8, 12};
    auto expected = [&](const int32_t dev[4][3], bool changed, const char* what) {
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < 3; ++i)
                CHECK(dev[w][i] == ((changed && (size_t)i * 4 < bytes[w]) ? now[w][i] : before[w][i]), "%s: write %d word %d = %d", what, w, i, dev[w][i]);
    };
    for (int fail_at = -1; fail_at < 4; ++fail_at)
        for (int again = -1; again < (fail_at < 0 ? 0 : 4); ++again) {
            int32_t dev[4][3];
            std::memcpy(dev, before, sizeof dev);
            std::vector<pb::DeviceWrite> writes;
            for (int w = 0; w < 4; ++w) writes.push_back({dev[w], now[w], before[w], bytes[w]});
            Writer writer;
            writer.fail_at = fail_at;
            writer.fail_again_at = again < 0 ? -1 : fail_at + 1 + again;  // the `again`-th write of the rollback
            const pb::Applied a = pb::apply_writes(writes, [&](void* d, const void* s, size_t n) { return writer(d, s, n); }, &writer.error);
            if (fail_at < 0) {
                CHECK(a == pb::Applied::kDone && writer.calls == 4 && writer.error.empty(), "no failure: %d calls", writer.calls);
                expected(dev, true, "no failure");
                continue;
            }
            expect(writer.error, "write " + std::to_string(fail_at) + " failed", "the first failure's text");
            if (again < 0) {
                CHECK(a == pb::Applied::kRolledBack && writer.calls == fail_at + 1 + 4, "failure at %d: %d calls", fail_at, writer.calls);
                expected(dev, false, "rolled back");
            } else {
                CHECK(a == pb::Applied::kTorn && writer.calls == fail_at + 1 + again + 1, "failures at %d and in the rollback at %d: %d calls", fail_at, again, writer.calls);
            }
        }
    // a block without a previous value is left as the failed edit wrote it; an empty list is done
    int32_t block[3] = {1, 2, 3}, row[3] = {4, 5, 6};
    Writer writer;
    writer.fail_at = 1;
    const pb::Applied a = pb::apply_writes(std::vector<pb::DeviceWrite>{{block, now[0], nullptr, 12}, {row, now[1], before[1], 12}},
                                           [&](void* d, const void* s, size_t n) { return writer(d, s, n); }, &writer.error);
    CHECK(a == pb::Applied::kRolledBack && writer.calls == 3 && block[0] == -1 && row[0] == 4, "block %d row %d after %d calls", block[0], row[0], writer.calls);
    CHECK(pb::apply_writes(std::vector<pb::DeviceWrite>{}, [&](void* d, const void* s, size_t n) { return writer(d, s, n); }, &writer.error) == pb::Applied::kDone, "empty list");
}

// ---- the combined mesh of a two-level scene ----
struct TwoLevel {
    // object 0: 2 triangles over 4 vertices; object 1: 1 triangle over 3; the world: 2 triangles over 4, the second a light
    std::vector<float> pos0 = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0}, pos1 = {0, 0, 1, 1, 0, 1, 0, 1, 1}, wpos = {-1, 2, -1, 1, 2, -1, 1, 2, 1, -1, 2, 1};
    std::vector<int32_t> idx0 = {0, 1, 2, 0, 2, 3}, idx1 = {2, 1, 0}, widx = {0, 1, 2, 0, 2, 3}, order0 = {1, 0}, order1 = {0}, mat0 = {1, 0}, wmat = {0, 1}, wlgt = {-1, 0};
    std::vector<int32_t> instance_object = {0, 1, 0}, tlas_order = {0, 1, 2, 3, 4};
    PbrtLinearBVHNode node{};  // the trees are not read here: scene_invalid checks them
    PbrtObject objects[2];
    PbrtInstance instances[3] = {};
    PbrtMaterial materials[2] = {material(PBRT_MAT_MATTE, 0.5f, 0.0f, 1.0f), material(PBRT_MAT_MATTE, 0.25f, 0.0f, 1.0f)};
    PbrtLight light{};
    pb::TwoLevelArgs a;
    TwoLevel() {
        objects[0] = {pos0.data(), 4, idx0.data(), 2, mat0.data(), &node, 1, order0.data()};
        objects[1] = {pos1.data(), 3, idx1.data(), 1, nullptr, &node, 1, order1.data()};
        light.type = PBRT_LIGHT_DIFFUSE_AREA;
        light.prim = 1;
        a = {objects, 2, instances, nullptr, instance_object.data(), 3, wpos.data(), 4, widx.data(), 2, wmat.data(), wlgt.data(), materials, 2, &light, 1, &node, 1,
             tlas_order.data()};
    }
};
void check_two_level_combine() {
    {
        TwoLevel t;
        pb::CombinedMesh m;
        expect(pb::combine_two_level(t.a, &m), "", "two objects and world triangles");
        CHECK(m.ia.obj_tri_offset == (std::vector<int32_t>{0, 2, 3}) && m.ia.world_tri_offset == 3 && m.ia.n_world_tris == 2 && m.n_nodes == 2, "offsets");
        CHECK(m.ia.n_objects == 2 && m.ia.n_instances == 3 && m.ia.instance_object == t.instance_object.data() && m.ia.motions == nullptr, "instancing arguments");
        CHECK(m.pos.size() == 11 * 3 && std::memcmp(&m.pos[0], t.pos0.data(), 48) == 0 && std::memcmp(&m.pos[12], t.pos1.data(), 36) == 0 &&
                  std::memcmp(&m.pos[21], t.wpos.data(), 48) == 0, "positions");
        CHECK(m.idx == (std::vector<int32_t>{0, 1, 2, 0, 2, 3, 6, 5, 4, 7, 8, 9, 7, 9, 10}), "rebased indices");
        CHECK(m.order == (std::vector<int32_t>{1, 0, 2, 3, 4}), "prim_order");
        CHECK(m.mat == (std::vector<int32_t>{1, 0, 0, 0, 1}), "materials");
        CHECK(m.lgt == (std::vector<int32_t>{-1, -1, -1, -1, 0}), "lights: -1 on object triangles");
    }
    {
        TwoLevel t;  // one object, no instance_object, no world triangles' material / light arrays
        t.a.n_objects = 1;
        t.a.instance_object = nullptr;
        t.a.world_tri_material = t.a.world_tri_light = nullptr;
        t.a.n_lights = 0;
        pb::CombinedMesh m;
        expect(pb::combine_two_level(t.a, &m), "", "one object and world triangles");
        CHECK(m.ia.obj_tri_offset == (std::vector<int32_t>{0, 2}) && m.ia.world_tri_offset == 2 && m.ia.instance_object == nullptr, "offsets");
        CHECK(m.idx == (std::vector<int32_t>{0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7}) && m.order == (std::vector<int32_t>{1, 0, 2, 3}), "indices and order");
        CHECK(m.mat == (std::vector<int32_t>{1, 0, 0, 0}) && m.lgt == (std::vector<int32_t>{-1, -1, -1, -1}), "materials and lights");
        t.a.n_world_tris = t.a.n_world_verts = 0;  // pbrt_hip_scene_create_instanced
        t.a.world_positions = nullptr;
        t.a.world_indices = nullptr;
        expect(pb::combine_two_level(t.a, &m), "", "one object alone");
        CHECK(m.idx.size() == 6 && m.pos.size() == 12 && m.ia.world_tri_offset == 2 && m.order == (std::vector<int32_t>{1, 0}), "one object alone");
    }
    pb::CombinedMesh m;
    auto refused = [&](const TwoLevel& t, const char* why) { expect(pb::combine_two_level(t.a, &m), why, why); };
    const char* needs = "two-level scene needs objects, instances and a top-level node array";
    for (int k = 0; k < 7; ++k) {
        TwoLevel t;
        if (k == 0) t.a.objects = nullptr;
        if (k == 1) t.a.n_objects = 0;
        if (k == 2) t.a.instances = nullptr;
        if (k == 3) t.a.n_instances = 0;
        if (k == 4) t.a.tlas_nodes = nullptr;
        if (k == 5) t.a.n_tlas_nodes = 0;
        if (k == 6) t.a.tlas_order = nullptr;
        refused(t, needs);
    }
    for (int k = 0; k < 5; ++k) {
        TwoLevel t;
        if (k == 0) t.a.n_world_tris = -1;
        if (k == 1) t.a.n_world_verts = -1;
        if (k == 2) t.a.world_positions = nullptr;
        if (k == 3) t.a.world_indices = nullptr;
        if (k == 4) t.a.n_world_verts = 0;
        refused(t, "bad world-space triangle arguments");
    }
    for (int k = 0; k < 7; ++k) {
        TwoLevel t;
        PbrtObject& o = t.objects[1];
        if (k == 0) o.positions = nullptr;
        if (k == 1) o.indices = nullptr;
        if (k == 2) o.nodes = nullptr;
        if (k == 3) o.prim_order = nullptr;
        if (k == 4) o.n_verts = 0;
        if (k == 5) o.n_tris = 0;
        if (k == 6) o.n_nodes = 0;
        refused(t, "object aggregate with a null pointer or an empty mesh / tree");
    }
    for (int32_t bad : {-1, 3, 10000}) {
        TwoLevel t;
        t.idx1[1] = bad;
        refused(t, "object vertex index out of range");
    }
    for (int32_t bad : {-1, 2}) {
        TwoLevel t;
        t.order0[1] = bad;
        refused(t, "object prim_order entry out of range");
    }
    for (int32_t bad : {-1, 4}) {
        TwoLevel t;
        t.widx[5] = bad;
        refused(t, "world triangle vertex index out of range");
    }
    for (int32_t bad : {-1, 2}) {
        TwoLevel t;
        t.instance_object[2] = bad;
        refused(t, "instance_object out of range");
    }
    for (int32_t bad : {-1, 2}) {
        TwoLevel t;
        t.light.prim = bad;
        refused(t, "area lights sit on world-space triangles (instanced primitives cannot be area lights): prim out of range");
    }
    {
        TwoLevel t;  // the counts alone decide: no array of that size is read before the refusal
        t.objects[0].n_verts = 0x7fffffff;
        t.objects[1].n_verts = 0x7fffffff;
        t.idx1 = {0x7ffffffe, 1, 0};
        t.objects[1].indices = t.idx1.data();
        refused(t, "two-level scene too large");
    }
}

}  // namespace

int main() {
    check_disney_refusals();
    check_disney_blocks();
    check_roughness();
    check_material_descs();
    check_lobe_rows();
    check_maps();
    check_power_edit({3.0f}, 0, 5.0f);
    check_power_edit({0.0f, 3.0f}, 0, 2.0f);
    check_power_edit({0.0f, 3.0f}, 1, 0.0f);  // every light dark
    check_power_edit({1.5f, 0.25f, 4.0f}, 1, 0.0f);
    check_apply_writes();
    check_two_level_combine();
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
