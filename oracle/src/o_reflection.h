// ORACLE — TEST INFRASTRUCTURE ONLY (see o_math.h header / oracle/README.md).
//
// o_reflection.h — BxDFs, BSDF, and the five materials the configs need.
//
// Follows:
//   src/core/reflection.rs:19-40      fr_dielectric
//   src/core/reflection.rs:135-156    reflect / refract / same_hemisphere
//   src/core/reflection.rs:162-170    BxDFType bitflags
//   src/core/reflection.rs:207-449    BSDF::{new, num_components, world_to_local, local_to_world, f, sample_f, pdf}
//   src/core/reflection.rs:453-509    trait BxDF defaults (cosine sample_f, pdf)
//   src/core/reflection.rs:614-659    SpecularReflection (+ FresnelNoOp :607-612, FresnelDielectric :590-604)
//   src/core/reflection.rs:661-731    SpecularTransmission
//   src/core/reflection.rs:733-819    FresnelSpecular
//   src/core/reflection.rs:821-855    LambertianReflection
//   src/core/reflection.rs:977-1056   MicrofacetReflection (distribution and Fresnel objects: o_microfacet.h)
//   src/core/material.rs:16-55        TransportMode, Material::compute_scattering_functions
// src/materials/*.rs are empty stubs in the reference; matte / mirror / glass are restated from
// pbrt-v3 on top of the reference's BxDFs:
//   matte  = LambertianReflection(Kd)            (sigma = 0)
//   mirror = SpecularReflection(Kr, FresnelNoOp)
//   glass  = FresnelSpecular(Kr, Kt, 1, eta) when allow_multiple_lobes, else
//            SpecularReflection(Kr, FresnelDielectric(1, eta)) + SpecularTransmission(Kt, 1, eta)
// Defect dispositions: D35 (matches_flags), D38 (sample_f unwraps None) — intended;
// D36, D37 [Q] behind quirk bits; D46 (face_forward returns the wrong operand) — intended.
#pragma once
#include "o_microfacet.h"
#include "o_shapes.h"

namespace oracle {

enum BxDFType : uint8_t {
    BSDF_NONE = 0,
    BSDF_REFLECTION = 1 << 0,
    BSDF_TRANSMISSION = 1 << 1,
    BSDF_DIFFUSE = 1 << 2,
    BSDF_GLOSSY = 1 << 3,
    BSDF_SPECULAR = 1 << 4,
    BSDF_ALL = 31,
};
enum TransportMode { MODE_RADIANCE = 0, MODE_IMPORTANCE = 1 };

// reflection.rs:19-40
inline Float fr_dielectric(Float cos_theta_i, Float eta_i, Float eta_t) {
    cos_theta_i = clampf(cos_theta_i, -1.0f, 1.0f);
    bool entering = cos_theta_i > 0.0f;
    if (!entering) {
        Float tmp = eta_i;
        eta_i = eta_t;
        eta_t = tmp;
        cos_theta_i = std::fabs(cos_theta_i);
    }
    Float sin_theta_i = std::sqrt(fmaxr(1.0f - cos_theta_i * cos_theta_i, 0.0f));
    Float sin_theta_t = eta_i / eta_t * sin_theta_i;
    if (sin_theta_t >= 1.0f) return 1.0f;
    Float cos_theta_t = std::sqrt(fmaxr(1.0f - sin_theta_t * sin_theta_t, 0.0f));
    Float r_parl = (eta_t * cos_theta_i - eta_i * cos_theta_t) / (eta_t * cos_theta_i + eta_i * cos_theta_t);
    Float r_perp = (eta_i * cos_theta_i - eta_t * cos_theta_t) / (eta_i * cos_theta_i + eta_t * cos_theta_t);
    return (r_parl * r_parl + r_perp * r_perp) / 2.0f;
}

inline Float cos_theta(const Vector3f& w) { return w.z; }
inline Float abs_cos_theta(const Vector3f& w) { return std::fabs(w.z); }
inline bool same_hemisphere(const Vector3f& w, const Vector3f& wp) { return w.z * wp.z > 0.0f; }

// reflection.rs:142-156 — D37 [Q]: as written tests sin2_theta_i.
inline bool refract(const Vector3f& wi, const Normal3f& n, Float eta, Vector3f* wt, uint32_t quirks = 0) {
    Float cos_theta_i = n.dot(wi);
    Float sin2_theta_i = fmaxr(1.0f - cos_theta_i * cos_theta_i, 0.0f);
    Float sin2_theta_t = eta * eta * sin2_theta_i;
    if (quirks & Q_D37_REFRACT) {
        if (sin2_theta_i >= 1.0f) return false;
    } else {
        if (sin2_theta_t >= 1.0f) return false;
    }
    Float cos_theta_t = std::sqrt(1.0f - sin2_theta_t);
    *wt = -wi * eta + n * (eta * cos_theta_i - cos_theta_t);
    return true;
}

// reflection.rs:453-509
struct BxDF {
    uint8_t type;
    uint32_t quirks = 0;
    explicit BxDF(uint8_t t) : type(t) {}
    virtual ~BxDF() {}
    // D35: intended (type & flags) == type
    bool matches_flags(uint8_t t) const { return (type & t) == type; }
    virtual Spectrum f(const Vector3f& wo, const Vector3f& wi) const = 0;
    virtual Spectrum sample_f(const Vector3f& wo, Vector3f* wi, const Point2f& u, Float* pdf,
                              uint8_t* sampled_type) const {
        *wi = cosine_sample_hemisphere(u, quirks);
        if (wo.z < 0.0f) wi->z *= -1.0f;
        *pdf = this->pdf(wo, *wi);
        return f(wo, *wi);
    }
    virtual Float pdf(const Vector3f& wo, const Vector3f& wi) const {
        return same_hemisphere(wo, wi) ? abs_cos_theta(wi) * INV_PI : 0.0f;
    }
};

// reflection.rs:821-855
struct LambertianReflection : BxDF {
    Spectrum r;
    explicit LambertianReflection(const Spectrum& r_) : BxDF(BSDF_REFLECTION | BSDF_DIFFUSE), r(r_) {}
    Spectrum f(const Vector3f&, const Vector3f&) const override { return r * INV_PI; }
};

// reflection.rs:614-659; fresnel: no-op (eta_t == 0 marker) or dielectric
struct SpecularReflection : BxDF {
    Spectrum r;
    bool fresnel_noop;
    Float eta_i, eta_t;
    SpecularReflection(const Spectrum& r_, bool noop, Float ei = 1.0f, Float et = 1.0f)
        : BxDF(BSDF_REFLECTION | BSDF_SPECULAR), r(r_), fresnel_noop(noop), eta_i(ei), eta_t(et) {}
    Spectrum f(const Vector3f&, const Vector3f&) const override { return Spectrum(0.0f); }
    Spectrum sample_f(const Vector3f& wo, Vector3f* wi, const Point2f&, Float* pdf, uint8_t*) const override {
        *wi = Vector3f(-wo.x, -wo.y, wo.z);
        *pdf = 1.0f;
        Spectrum fr = fresnel_noop ? Spectrum(1.0f) : Spectrum(fr_dielectric(cos_theta(*wi), eta_i, eta_t));
        return r * fr / abs_cos_theta(*wi);
    }
    Float pdf(const Vector3f&, const Vector3f&) const override { return 0.0f; }
};

// reflection.rs:661-731
struct SpecularTransmission : BxDF {
    Spectrum t;
    Float eta_a, eta_b;
    TransportMode mode;
    SpecularTransmission(const Spectrum& t_, Float a, Float b, TransportMode m)
        : BxDF(BSDF_SPECULAR | BSDF_TRANSMISSION), t(t_), eta_a(a), eta_b(b), mode(m) {}
    Spectrum f(const Vector3f&, const Vector3f&) const override { return Spectrum(0.0f); }
    Spectrum sample_f(const Vector3f& wo, Vector3f* wi, const Point2f&, Float* pdf, uint8_t*) const override {
        bool entering = cos_theta(wo) > 0.0f;
        Float eta_i = entering ? eta_a : eta_b;
        Float eta_t = entering ? eta_b : eta_a;
        if (!refract(wo, Normal3f(0.0f, 0.0f, 1.0f).face_forward(wo), eta_i / eta_t, wi, quirks))
            return Spectrum(0.0f);
        *pdf = 1.0f;
        Spectrum ft = t * (Spectrum(1.0f) - Spectrum(fr_dielectric(cos_theta(*wi), eta_a, eta_b)));
        if (mode == MODE_RADIANCE) ft *= (eta_i * eta_i) / (eta_t * eta_t);
        return ft / abs_cos_theta(*wi);
    }
    Float pdf(const Vector3f&, const Vector3f&) const override { return 0.0f; }
};

// reflection.rs:733-819
struct FresnelSpecular : BxDF {
    Spectrum r, t;
    Float eta_a, eta_b;
    TransportMode mode;
    FresnelSpecular(const Spectrum& r_, const Spectrum& t_, Float a, Float b, TransportMode m)
        : BxDF(BSDF_TRANSMISSION | BSDF_SPECULAR | BSDF_REFLECTION), r(r_), t(t_), eta_a(a), eta_b(b), mode(m) {}
    Spectrum f(const Vector3f&, const Vector3f&) const override { return Spectrum(0.0f); }
    Spectrum sample_f(const Vector3f& wo, Vector3f* wi, const Point2f& u, Float* pdf,
                      uint8_t* sampled_type) const override {
        Float fr = fr_dielectric(cos_theta(wo), eta_a, eta_b);
        if (u.x < fr) {
            *wi = Vector3f(-wo.x, -wo.y, wo.z);
            if (sampled_type) *sampled_type = BSDF_SPECULAR | BSDF_REFLECTION;
            *pdf = fr;
            return r * fr / abs_cos_theta(*wi);
        } else {
            bool entering = cos_theta(wo) > 0.0f;
            Float eta_i = entering ? eta_a : eta_b;
            Float eta_t = entering ? eta_b : eta_a;
            if (!refract(wo, Normal3f(0.0f, 0.0f, 1.0f).face_forward(wo), eta_i / eta_t, wi, quirks))
                return Spectrum(0.0f);
            Spectrum ft = t * (1.0f - fr);
            if (mode == MODE_RADIANCE) ft *= (eta_i * eta_i) / (eta_t * eta_t);
            if (sampled_type) *sampled_type = BSDF_SPECULAR | BSDF_TRANSMISSION;
            *pdf = 1.0f - fr;
            return ft / abs_cos_theta(*wi);
        }
    }
    Float pdf(const Vector3f&, const Vector3f&) const override { return 0.0f; }
};

// reflection.rs:977-1056 (D63: sample_f writes wi = reflect(wo, wh), pbrt-v3's reading)
struct MicrofacetReflection : BxDF {
    Spectrum r;
    TrowbridgeReitzDistribution distribution;
    std::shared_ptr<Fresnel> fresnel;
    MicrofacetReflection(const Spectrum& r_, const TrowbridgeReitzDistribution& d, const std::shared_ptr<Fresnel>& fr)
        : BxDF(BSDF_GLOSSY | BSDF_REFLECTION), r(r_), distribution(d), fresnel(fr) {}
    // reflection.rs:1000-1018
    Spectrum f(const Vector3f& wo, const Vector3f& wi) const override {
        Float cos_theta_o = abs_cos_theta(wo), cos_theta_i = abs_cos_theta(wi);
        Vector3f wh = wi + wo;
        if (cos_theta_i == 0.0f || cos_theta_o == 0.0f) return Spectrum(0.0f);
        if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return Spectrum(0.0f);
        wh = wh.normalize();
        Spectrum fr = fresnel->evaluate(wi.dot(wh.face_forward(Vector3f(0.0f, 0.0f, 1.0f))));
        return r * distribution.d(wh) * distribution.g(wo, wi) * fr / (4.0f * cos_theta_i * cos_theta_o);
    }
    // reflection.rs:1020-1043
    Spectrum sample_f(const Vector3f& wo, Vector3f* wi, const Point2f& u, Float* pdf, uint8_t*) const override {
        if (wo.z == 0.0f) return Spectrum(0.0f);
        Vector3f wh = distribution.sample_wh(wo, u);
        if (wo.dot(wh) < 0.0f) return Spectrum(0.0f);
        *wi = reflect(wo, wh);
        if (!same_hemisphere(wo, *wi)) return Spectrum(0.0f);
        *pdf = distribution.pdf(wo, wh) / (4.0f * wo.dot(wh));
        return f(wo, *wi);
    }
    // reflection.rs:1045-1051
    Float pdf(const Vector3f& wo, const Vector3f& wi) const override {
        if (!same_hemisphere(wo, wi)) return 0.0f;
        Vector3f wh = (wo + wi).normalize();
        return distribution.pdf(wo, wh) / (4.0f * wo.dot(wh));
    }
};

// reflection.rs:207-449
struct BSDF {
    Float eta;
    Normal3f ns, ng;
    Vector3f ss, ts;
    int n_bxdfs = 0;
    static const int MAX_BXDFS = 8;
    std::shared_ptr<BxDF> bxdfs[MAX_BXDFS];
    uint32_t quirks = 0;
    // reflection.rs:220-234
    BSDF(const SurfaceInteraction& si, Float eta_ = 1.0f, uint32_t q = 0) : eta(eta_), quirks(q) {
        ns = si.shading.n;
        ng = si.n;
        ss = si.shading.dpdu.normalize();
        ts = ns.cross(ss);
    }
    void add(const std::shared_ptr<BxDF>& b) {
        b->quirks = quirks;
        bxdfs[n_bxdfs++] = b;
    }
    int num_components(uint8_t flags) const {
        int num = 0;
        for (int i = 0; i < n_bxdfs; ++i)
            if (bxdfs[i]->matches_flags(flags)) ++num;
        return num;
    }
    Vector3f world_to_local(const Vector3f& v) const { return Vector3f(v.dot(ss), v.dot(ts), v.dot(ns)); }
    // reflection.rs:256-262 — D36 [Q]
    Vector3f local_to_world(const Vector3f& v) const {
        Float y = (quirks & Q_D36_LOCAL_TO_WORLD) ? (ss.y * v.x + ts.y * v.y * ns.y * v.z)
                                                  : (ss.y * v.x + ts.y * v.y + ns.y * v.z);
        return Vector3f(ss.x * v.x + ts.x * v.y + ns.x * v.z, y, ss.z * v.x + ts.z * v.y + ns.z * v.z);
    }
    // reflection.rs:264-283
    Spectrum f(const Vector3f& wo_w, const Vector3f& wi_w, uint8_t flags) const {
        Vector3f wi = world_to_local(wi_w), wo = world_to_local(wo_w);
        if (wo.z == 0.0f) return Spectrum(0.0f);
        bool reflect = wi_w.dot(ng) * wo_w.dot(ng) > 0.0f;
        Spectrum f(0.0f);
        for (int i = 0; i < n_bxdfs; ++i)
            if (bxdfs[i]->matches_flags(flags) &&
                ((reflect && (bxdfs[i]->type & BSDF_REFLECTION)) || (!reflect && (bxdfs[i]->type & BSDF_TRANSMISSION))))
                f += bxdfs[i]->f(wo, wi);
        return f;
    }
    // reflection.rs:285-377
    Spectrum sample_f(const Vector3f& wo_w, Vector3f* wi_w, const Point2f& u, Float* pdf, uint8_t type,
                      uint8_t* sampled_type) const {
        int matching_comps = num_components(type);
        if (matching_comps == 0) {
            *pdf = 0.0f;
            if (sampled_type) *sampled_type = BSDF_NONE;
            return Spectrum(0.0f);
        }
        int comp = std::min((int)std::floor(u.x * (Float)matching_comps), matching_comps - 1);
        const BxDF* bxdf = nullptr;
        int count = comp;
        for (int i = 0; i < n_bxdfs; ++i)
            if (bxdfs[i]->matches_flags(type) && count-- == 0) {
                bxdf = bxdfs[i].get();
                break;
            }
        Point2f u_remapped(fminr(u.x * (Float)matching_comps - (Float)comp, ONE_MINUS_EPSILON), u.y);
        Vector3f wi, wo = world_to_local(wo_w);
        if (wo.z == 0.0f) return Spectrum(0.0f);
        *pdf = 0.0f;
        if (sampled_type) *sampled_type = bxdf->type;
        Spectrum f = bxdf->sample_f(wo, &wi, u_remapped, pdf, sampled_type);
        if (*pdf == 0.0f) {
            if (sampled_type) *sampled_type = BSDF_NONE;
            return Spectrum(0.0f);
        }
        *wi_w = local_to_world(wi);
        if (!(bxdf->type & BSDF_SPECULAR) && matching_comps > 1)
            for (int i = 0; i < n_bxdfs; ++i)
                if (bxdfs[i].get() != bxdf && bxdfs[i]->matches_flags(type)) *pdf += bxdfs[i]->pdf(wo, wi);
        if (matching_comps > 1) *pdf /= (Float)matching_comps;
        if (!(bxdf->type & BSDF_SPECULAR)) {
            bool reflect = wi_w->dot(ng) * wo_w.dot(ng) > 0.0f;
            f = Spectrum(0.0f);
            for (int i = 0; i < n_bxdfs; ++i)
                if (bxdfs[i]->matches_flags(type) && ((reflect && (bxdfs[i]->type & BSDF_REFLECTION)) ||
                                                      (!reflect && (bxdfs[i]->type & BSDF_TRANSMISSION))))
                    f += bxdfs[i]->f(wo, wi);
        }
        return f;
    }
    // reflection.rs:414-446
    Float pdf(const Vector3f& wo_w, const Vector3f& wi_w, uint8_t flags) const {
        if (n_bxdfs == 0) return 0.0f;
        Vector3f wo = world_to_local(wo_w), wi = world_to_local(wi_w);
        if (wo.z == 0.0f) return 0.0f;
        Float pdf = 0.0f;
        int matching_comps = 0;
        for (int i = 0; i < n_bxdfs; ++i)
            if (bxdfs[i]->matches_flags(flags)) {
                ++matching_comps;
                pdf += bxdfs[i]->pdf(wo, wi);
            }
        return matching_comps > 0 ? pdf / (Float)matching_comps : 0.0f;
    }
};

// Material description shared with the C ABI (include/pbrt_hip.h PbrtMaterial).
enum MaterialType { MAT_NONE = 0, MAT_MATTE = 1, MAT_MIRROR = 2, MAT_GLASS = 3, MAT_PLASTIC = 4, MAT_METAL = 5 };
struct MaterialDesc {
    int type;
    Spectrum kd;  // matte Kd / mirror-glass Kr / plastic Kd / metal eta
    Spectrum kt;  // glass Kt / plastic Ks / metal k
    Float eta;    // glass index; plastic / metal: the isotropic roughness, remapped
    // plastic / metal: the roughness pair and pbrt-v3's remaproughness switch (orc_scene_set_material_roughness);
    // set_roughness(eta, eta, true) is what a material row alone means
    Float u_roughness = 0.0f, v_roughness = 0.0f;
    bool remap_roughness = true;
    Float alpha_u = 0.0f, alpha_v = 0.0f;  // TrowbridgeReitzDistribution::new's arguments (plastic.cpp / metal.cpp)
    void set_roughness(Float u, Float v, bool remap) {
        u_roughness = u, v_roughness = v, remap_roughness = remap;
        alpha_u = remap ? TrowbridgeReitzDistribution::roughness_to_alpha(u) : u;
        alpha_v = remap ? TrowbridgeReitzDistribution::roughness_to_alpha(v) : v;
    }
    static MaterialDesc from_row(const float* m) {  // {type, kd rgb, kt rgb, eta}
        MaterialDesc d;
        d.type = (int)m[0];
        d.kd = Spectrum(m[1], m[2], m[3]);
        d.kt = Spectrum(m[4], m[5], m[6]);
        d.eta = m[7];
        d.set_roughness(m[7], m[7], true);
        return d;
    }
};

// src/core/material.rs:16-55 trait Material::compute_scattering_functions
inline std::shared_ptr<BSDF> compute_scattering_functions(const MaterialDesc& m, const SurfaceInteraction& si,
                                                          TransportMode mode, bool allow_multiple_lobes,
                                                          uint32_t quirks = 0) {
    if (m.type == MAT_NONE) return nullptr;
    if (m.type == MAT_MATTE) {
        auto bsdf = std::make_shared<BSDF>(si, 1.0f, quirks);
        if (!m.kd.is_black()) bsdf->add(std::make_shared<LambertianReflection>(m.kd));
        return bsdf;
    }
    if (m.type == MAT_MIRROR) {
        auto bsdf = std::make_shared<BSDF>(si, 1.0f, quirks);
        if (!m.kd.is_black()) bsdf->add(std::make_shared<SpecularReflection>(m.kd, true));
        return bsdf;
    }
    if (m.type == MAT_PLASTIC || m.type == MAT_METAL) {
        // pbrt-v3 PlasticMaterial / MetalMaterial on the reference's BxDFs (src/materials/*.rs are empty stubs):
        //   plastic = LambertianReflection(Kd) if Kd is not black, then
        //             MicrofacetReflection(Ks, TrowbridgeReitz(a, a), FresnelDielectric(1.5, 1)) if Ks is not black
        //   metal   = MicrofacetReflection(1, TrowbridgeReitz(a_u, a_v), FresnelConductor(1, eta, k))
        auto bsdf = std::make_shared<BSDF>(si, 1.0f, quirks);
        TrowbridgeReitzDistribution distrib(m.alpha_u, m.alpha_v);
        if (m.type == MAT_PLASTIC) {
            if (!m.kd.is_black()) bsdf->add(std::make_shared<LambertianReflection>(m.kd));
            if (!m.kt.is_black())
                bsdf->add(std::make_shared<MicrofacetReflection>(m.kt, distrib, std::make_shared<FresnelDielectric>(1.5f, 1.0f)));
        } else {
            bsdf->add(std::make_shared<MicrofacetReflection>(
                Spectrum(1.0f), distrib, std::make_shared<FresnelConductor>(Spectrum(1.0f), m.kd, m.kt)));
        }
        return bsdf;
    }
    // glass (pbrt-v3 GlassMaterial, roughness 0)
    auto bsdf = std::make_shared<BSDF>(si, m.eta, quirks);
    if (m.kd.is_black() && m.kt.is_black()) return bsdf;
    if (allow_multiple_lobes) {
        bsdf->add(std::make_shared<FresnelSpecular>(m.kd, m.kt, 1.0f, m.eta, mode));
    } else {
        if (!m.kd.is_black()) bsdf->add(std::make_shared<SpecularReflection>(m.kd, false, 1.0f, m.eta));
        if (!m.kt.is_black()) bsdf->add(std::make_shared<SpecularTransmission>(m.kt, 1.0f, m.eta, mode));
    }
    return bsdf;
}

}  // namespace oracle
