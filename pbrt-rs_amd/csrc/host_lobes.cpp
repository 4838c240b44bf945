// host_lobes.cpp — lobe lists of material rows (host_lobes.h): pbrt-v3's material rules written out as lists of the reference's
// BxDFs. Host only; pbrt_hip_material_lobes needs no context and no GPU.
#include "host_lobes.h"

#include <cstring>

#include "abi_guard.h"

namespace pb {

const char* material_invalid(const PbrtMaterial& m) {
    if (m.type < PBRT_MAT_NONE || m.type > PBRT_MAT_METAL) return "unknown material type";
    if (m.type == PBRT_MAT_GLASS && !(m.eta > 0.0f)) return "glass needs eta > 0";
    if (m.type == PBRT_MAT_PLASTIC || m.type == PBRT_MAT_METAL)
        if (const char* why = roughness_invalid(m.eta, m.eta, true)) return why;
    if (m.type == PBRT_MAT_METAL)
        for (int c = 0; c < 3; ++c) {
            if (!(std::isfinite(m.kd[c]) && m.kd[c] > 0.0f)) return "metal eta must be finite and > 0";
            if (!(std::isfinite(m.kt[c]) && m.kt[c] >= 0.0f)) return "metal k must be finite and >= 0";
        }
    return nullptr;
}

DevMaterial row_of_material(const PbrtMaterial& m) {
    DevMaterial r{};
    r.type = m.type;
    std::memcpy(r.kd, m.kd, 12);
    std::memcpy(r.kt, m.kt, 12);
    r.eta = m.eta;
    const bool glossy = m.type == PBRT_MAT_PLASTIC || m.type == PBRT_MAT_METAL;
    r.alpha_u = r.alpha_v = glossy ? roughness_to_alpha(m.eta) : 0.0f;
    return r;
}

static bool bad_colour(const float* c) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(c[k]) || c[k] < 0.0f) return true;
    return false;
}
static bool black(const float* c) { return c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f; }

const char* row_of_desc(const PbrtMaterialDesc& d, DevMaterial* out) {
    if (d.type != PBRT_MATDESC_MATTE && d.type != PBRT_MATDESC_GLASS && d.type != PBRT_MATDESC_SUBSTRATE)
        return "unknown material descriptor type";
    DevMaterial m{};
    if (d.type == PBRT_MATDESC_MATTE) {
        if (bad_colour(d.kd)) return "Kd must be finite and >= 0";
        if (!std::isfinite(d.sigma) || d.sigma < 0.0f) return "sigma must be finite and >= 0";
        std::memcpy(m.kd, d.kd, 12);
        const double sigma = std::min((double)d.sigma, 90.0) * (3.14159265358979323846 / 180.0);  // MatteMaterial's clamp, then radians
        if (sigma == 0.0) {
            m.type = PBRT_MAT_MATTE;
            m.eta = 1.0f;
        } else {  // OrenNayar::new (reflection.rs:925-936), in double, rounded once
            const double sigma2 = sigma * sigma;
            m.type = kMatOrenNayar;
            m.alpha_u = (float)(1.0 - sigma2 / (2.0 * (sigma2 + 0.33)));
            m.alpha_v = (float)(0.45 * sigma2 / (sigma2 + 0.09));
        }
    } else {
        const bool glass = d.type == PBRT_MATDESC_GLASS;
        const float* c0 = glass ? d.kr : d.kd;
        const float* c1 = glass ? d.kt : d.ks;
        if (bad_colour(c0)) return glass ? "Kr must be finite and >= 0" : "Kd must be finite and >= 0";
        if (bad_colour(c1)) return glass ? "Kt must be finite and >= 0" : "Ks must be finite and >= 0";
        if (glass && !(std::isfinite(d.eta) && d.eta > 0.0f)) return "glass needs a finite eta > 0";
        const bool remap = d.remap_roughness != 0;
        if (const char* why = roughness_invalid(d.u_roughness, d.v_roughness, true)) return why;
        std::memcpy(m.kd, c0, 12);
        std::memcpy(m.kt, c1, 12);
        m.eta = glass ? d.eta : 1.0f;
        if (glass && d.u_roughness == 0.0f && d.v_roughness == 0.0f) {
            m.type = PBRT_MAT_GLASS;  // GlassMaterial's isSpecular: FresnelSpecular / the specular lobes
        } else {
            // alpha 0 is refused only where a microfacet lobe would carry it
            if (!(black(c0) && black(c1)))
                if (const char* why = roughness_invalid(d.u_roughness, d.v_roughness, remap)) return why;
            m.type = glass ? kMatRoughGlass : kMatSubstrate;
            m.alpha_u = remap ? roughness_to_alpha(d.u_roughness) : d.u_roughness;
            m.alpha_v = remap ? roughness_to_alpha(d.v_roughness) : d.v_roughness;
        }
    }
    *out = m;
    return nullptr;
}

// ---- lobes ----
constexpr int kR = 1, kT = 2, kDiffuse = 4, kGlossy = 8, kSpecular = 16;  // BxDFType

static PbrtLobe make_lobe(int kind, int type, const float* r) {
    PbrtLobe l{};
    l.kind = kind;
    l.type = type;
    l.fresnel = PBRT_FRESNEL_NOOP;
    for (int k = 0; k < 3; ++k) {
        l.scale[k] = 1.0f;
        l.r[k] = r[k];
    }
    l.eta_i = l.eta_t = 1.0f;
    return l;
}
static PbrtLobe lambertian_reflection(const float* r) { return make_lobe(PBRT_LOBE_LAMBERTIAN_REFLECTION, kR | kDiffuse, r); }
static PbrtLobe lambertian_transmission(const float* t) { return make_lobe(PBRT_LOBE_LAMBERTIAN_TRANSMISSION, kT | kDiffuse, t); }
static PbrtLobe specular_reflection(const float* r, int fresnel, float eta_i, float eta_t) {
    PbrtLobe l = make_lobe(PBRT_LOBE_SPECULAR_REFLECTION, kR | kSpecular, r);
    l.fresnel = fresnel;
    l.eta_i = eta_i;
    l.eta_t = eta_t;
    return l;
}
static PbrtLobe specular_transmission(const float* t, float eta_a, float eta_b) {
    PbrtLobe l = make_lobe(PBRT_LOBE_SPECULAR_TRANSMISSION, kT | kSpecular, t);
    l.fresnel = PBRT_FRESNEL_DIELECTRIC;
    l.eta_i = eta_a;
    l.eta_t = eta_b;
    return l;
}
static PbrtLobe microfacet_reflection(const float* r, float ax, float ay, float eta_i, float eta_t) {
    PbrtLobe l = make_lobe(PBRT_LOBE_MICROFACET_REFLECTION, kR | kGlossy, r);
    l.fresnel = PBRT_FRESNEL_DIELECTRIC;
    l.ax = ax;
    l.ay = ay;
    l.eta_i = eta_i;
    l.eta_t = eta_t;
    return l;
}
static PbrtLobe microfacet_transmission(const float* t, float ax, float ay, float eta_a, float eta_b) {
    PbrtLobe l = make_lobe(PBRT_LOBE_MICROFACET_TRANSMISSION, kT | kGlossy, t);
    l.fresnel = PBRT_FRESNEL_DIELECTRIC;
    l.ax = ax;
    l.ay = ay;
    l.eta_i = eta_a;
    l.eta_t = eta_b;
    return l;
}

const char* lobes_of_row(const DevMaterial& m, LobeList* out) {
    LobeList L;
    auto add = [&](const PbrtLobe& l) { L.lobes[L.n++] = l; };
    switch (m.type) {
        case PBRT_MAT_NONE: break;
        case PBRT_MAT_MATTE:
            if (!black(m.kd)) add(lambertian_reflection(m.kd));
            break;
        case PBRT_MAT_MIRROR:
            if (!black(m.kd)) add(specular_reflection(m.kd, PBRT_FRESNEL_NOOP, 1.0f, 1.0f));
            break;
        case PBRT_MAT_GLASS:
            return "smooth glass has no one lobe list: FresnelSpecular under the path integrator, two specular lobes elsewhere; "
                   "an uber row with Kr, Kt gives smooth specular lobes";
        case PBRT_MAT_PLASTIC:  // pbrt-v3's PlasticMaterial passes FresnelDielectric(1.5, 1)
            if (!black(m.kd)) add(lambertian_reflection(m.kd));
            if (!black(m.kt)) add(microfacet_reflection(m.kt, m.alpha_u, m.alpha_v, 1.5f, 1.0f));
            break;
        case PBRT_MAT_METAL: {
            const float one[3] = {1.0f, 1.0f, 1.0f};
            PbrtLobe l = microfacet_reflection(one, m.alpha_u, m.alpha_v, 1.0f, 1.0f);
            l.fresnel = PBRT_FRESNEL_CONDUCTOR;
            std::memcpy(l.eta, m.kd, 12);
            std::memcpy(l.k, m.kt, 12);
            add(l);
            break;
        }
        case kMatOrenNayar:
            if (!black(m.kd)) {
                PbrtLobe l = make_lobe(PBRT_LOBE_OREN_NAYAR, kR | kDiffuse, m.kd);
                l.A = m.alpha_u;
                l.B = m.alpha_v;
                add(l);
            }
            break;
        case kMatRoughGlass:
            if (!black(m.kd)) add(microfacet_reflection(m.kd, m.alpha_u, m.alpha_v, 1.0f, m.eta));
            if (!black(m.kt)) add(microfacet_transmission(m.kt, m.alpha_u, m.alpha_v, 1.0f, m.eta));
            L.eta = m.eta;
            break;
        case kMatSubstrate:
            if (!(black(m.kd) && black(m.kt))) {
                PbrtLobe l = make_lobe(PBRT_LOBE_FRESNEL_BLEND, kR | kGlossy, m.kd);
                std::memcpy(l.s, m.kt, 12);
                l.ax = m.alpha_u;
                l.ay = m.alpha_v;
                add(l);
            }
            break;
        case kMatDisney: return "a Disney row has no lobe list";
        case kMatHair: return "a hair row has no lobe list";
        default: return "a lobe row is not an operand";
    }
    *out = L;
    return nullptr;
}

static float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
static void clamp3(const float* c, float* out) {
    for (int k = 0; k < 3; ++k) out[k] = clamp01(c[k]);
}
static void mul3(const float* a, const float* b, float* out) {
    for (int k = 0; k < 3; ++k) out[k] = a[k] * b[k];
}

const char* lobes_of_lobe_desc(const PbrtLobeMaterialDesc& d, const LobeList* a, const LobeList* b, LobeList* out) {
    LobeList L;
    auto add = [&](const PbrtLobe& l) { L.lobes[L.n++] = l; };
    const bool remap = d.remap_roughness != 0;
    if (d.type == PBRT_LOBEMAT_UBER) {
        if (bad_colour(d.kd)) return "Kd must be finite and >= 0";
        if (bad_colour(d.ks)) return "Ks must be finite and >= 0";
        if (bad_colour(d.kr)) return "Kr must be finite and >= 0";
        if (bad_colour(d.kt)) return "Kt must be finite and >= 0";
        if (bad_colour(d.opacity)) return "opacity must be finite and >= 0";
        if (!(std::isfinite(d.eta) && d.eta > 0.0f)) return "eta must be finite and > 0";
        if (const char* why = roughness_invalid(d.u_roughness, d.v_roughness, true)) return why;
        float op[3], t[3], c[3], kd[3], ks[3], kr[3], kt[3];
        clamp3(d.opacity, op);
        for (int k = 0; k < 3; ++k) t[k] = clamp01(-op[k] + 1.0f);
        if (!black(t)) {
            add(specular_transmission(t, 1.0f, 1.0f));
            L.eta = 1.0f;
        } else {
            L.eta = d.eta;
        }
        clamp3(d.kd, c);
        mul3(op, c, kd);
        if (!black(kd)) add(lambertian_reflection(kd));
        clamp3(d.ks, c);
        mul3(op, c, ks);
        if (!black(ks)) {
            if (const char* why = roughness_invalid(d.u_roughness, d.v_roughness, remap)) return why;
            add(microfacet_reflection(ks, remap ? roughness_to_alpha(d.u_roughness) : d.u_roughness,
                                      remap ? roughness_to_alpha(d.v_roughness) : d.v_roughness, 1.0f, d.eta));
        }
        clamp3(d.kr, c);
        mul3(op, c, kr);
        if (!black(kr)) add(specular_reflection(kr, PBRT_FRESNEL_DIELECTRIC, 1.0f, d.eta));
        clamp3(d.kt, c);
        mul3(op, c, kt);
        if (!black(kt)) add(specular_transmission(kt, 1.0f, d.eta));
    } else if (d.type == PBRT_LOBEMAT_TRANSLUCENT) {
        if (bad_colour(d.kd)) return "Kd must be finite and >= 0";
        if (bad_colour(d.ks)) return "Ks must be finite and >= 0";
        if (bad_colour(d.reflect)) return "reflect must be finite and >= 0";
        if (bad_colour(d.transmit)) return "transmit must be finite and >= 0";
        if (const char* why = roughness_invalid(d.u_roughness, d.u_roughness, true)) return why;
        L.eta = 1.5f;
        float r[3], t[3], kd[3], ks[3], c[3];
        clamp3(d.reflect, r);
        clamp3(d.transmit, t);
        clamp3(d.kd, kd);
        clamp3(d.ks, ks);
        if (!(black(r) && black(t))) {
            if (!black(kd)) {
                if (!black(r)) {
                    mul3(r, kd, c);
                    add(lambertian_reflection(c));
                }
                if (!black(t)) {
                    mul3(t, kd, c);
                    add(lambertian_transmission(c));
                }
            }
            if (!black(ks)) {
                if (const char* why = roughness_invalid(d.u_roughness, d.u_roughness, remap)) return why;
                const float alpha = remap ? roughness_to_alpha(d.u_roughness) : d.u_roughness;
                if (!black(r)) {
                    mul3(r, ks, c);
                    add(microfacet_reflection(c, alpha, alpha, 1.0f, 1.5f));
                }
                if (!black(t)) {
                    mul3(t, ks, c);
                    add(microfacet_transmission(c, alpha, alpha, 1.0f, 1.5f));
                }
            }
        }
    } else if (d.type == PBRT_LOBEMAT_MIX) {
        if (bad_colour(d.amount)) return "amount must be finite and >= 0";
        if (!a || !b) return "a mix needs both operands' lists";
        if (a->n < 0 || b->n < 0 || a->n > kMaxLobes || b->n > kMaxLobes) return "an operand's lobe count is out of range";
        if (a->n + b->n > kMaxLobes) return "a mix of more than 8 lobes";
        float s1[3], s2[3];
        clamp3(d.amount, s1);
        for (int k = 0; k < 3; ++k) s2[k] = clamp01(1.0f - s1[k]);
        for (int side = 0; side < 2; ++side) {
            const LobeList* src = side ? b : a;
            const float* s = side ? s2 : s1;
            for (int i = 0; i < src->n; ++i) {
                PbrtLobe l = src->lobes[i];
                mul3(s, l.scale, l.scale);  // ScaledBxDF (reflection.rs:521-563); a black scale is kept, as pbrt-v3 keeps it
                add(l);
            }
        }
        L.eta = a->eta;
    } else {
        return "unknown lobe material type";
    }
    *out = L;
    return nullptr;
}

DevLobeRow lobe_row_of(const LobeList& l) {
    DevLobeRow r{};
    r.n = l.n;
    r.eta = l.eta;
    for (int i = 0; i < l.n; ++i) {
        r.lobes[i] = l.lobes[i];
        r.type_or |= l.lobes[i].type;
        if (!(l.lobes[i].type & kSpecular)) r.n_nonspec += 1;
    }
    return r;
}

}  // namespace pb

// Context-free lobe list of any row description (include/pbrt_hip.h)
extern "C" int pbrt_hip_material_lobes(const PbrtMaterial* row, const PbrtMaterialDesc* desc, const PbrtLobeMaterialDesc* lobe_desc,
                                       const PbrtLobe* a, int32_t n_a, float eta_a, const PbrtLobe* b, int32_t n_b, PbrtLobe lobes[8],
                                       int32_t* n, float* eta, const char** reason) try {
    auto refuse = [&](const char* why) {
        if (reason) *reason = why;
        return PBRT_HIP_ERR_INVALID;
    };
    if (reason) *reason = "";
    if (!lobes || !n || !eta) return refuse("null pointer");
    if ((row ? 1 : 0) + (desc ? 1 : 0) + (lobe_desc ? 1 : 0) != 1) return refuse("exactly one of row, desc and lobe_desc");
    pb::LobeList L;
    if (row) {
        if (const char* why = pb::material_invalid(*row)) return refuse(why);
        if (const char* why = pb::lobes_of_row(pb::row_of_material(*row), &L)) return refuse(why);
    } else if (desc) {
        pb::DevMaterial m;
        if (const char* why = pb::row_of_desc(*desc, &m)) return refuse(why);
        if (const char* why = pb::lobes_of_row(m, &L)) return refuse(why);
    } else {
        pb::LobeList la, lb;
        const bool mix = lobe_desc->type == PBRT_LOBEMAT_MIX;
        if (mix) {
            if (n_a < 0 || n_b < 0 || n_a > pb::kMaxLobes || n_b > pb::kMaxLobes) return refuse("an operand's lobe count is out of range");
            if ((n_a && !a) || (n_b && !b)) return refuse("null operand list");
            la.n = n_a;
            la.eta = eta_a;
            lb.n = n_b;
            for (int i = 0; i < n_a; ++i) la.lobes[i] = a[i];
            for (int i = 0; i < n_b; ++i) lb.lobes[i] = b[i];
        }
        if (const char* why = pb::lobes_of_lobe_desc(*lobe_desc, mix ? &la : nullptr, mix ? &lb : nullptr, &L)) return refuse(why);
    }
    for (int i = 0; i < pb::kMaxLobes; ++i) lobes[i] = i < L.n ? L.lobes[i] : PbrtLobe{};
    *n = L.n;
    *eta = L.eta;
    return PBRT_HIP_OK;
}
PB_ABI_CATCH
