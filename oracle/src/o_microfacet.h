// ORACLE — TEST INFRASTRUCTURE ONLY (see o_math.h header / oracle/README.md).
//
// o_microfacet.h — the Trowbridge-Reitz microfacet distribution and the Fresnel objects, i.e. what plastic's and metal's
// MicrofacetReflection lobe is made of (o_reflection.h: MicrofacetReflection, compute_scattering_functions).
//
// Follows:
//   src/core/reflection.rs:42-67       fr_conductor
//   src/core/reflection.rs:71-124      cos_theta .. sin2_phi
//   src/core/reflection.rs:139-142     reflect
//   src/core/reflection.rs:565-612     trait Fresnel, FresnelConductor, FresnelDielectric, FresnelNoOp
//   src/core/microfacet.rs:11-30       trait MicrofacetDistribution defaults (g1, g, pdf)
//   src/core/microfacet.rs:145-248     TrowbridgeReitzDistribution::{roughness_to_alpha, d, lambda, sample_wh}
//   src/core/microfacet.rs:336-406     trowbridge_reitz_sample11 / trowbridge_reitz_sample
// Defect dispositions, all intended pbrt-v3 semantics:
//   D64 the slopes are unstretched as alpha_x * slope_x, alpha_y * slope_y (microfacet.rs:402-403 assign alpha^2);
//   D65 the discriminant's second term carries `* tmp` and the fit's constant is 0.597999 (microfacet.rs:362, 381);
//   D66 the non-visible-area sample_wh (microfacet.rs:203-227) is not restated: sample_visible_area is always on;
//   D46 face_forward returns +-self.
// roughness_to_alpha is evaluated in double and rounded once, as DESIGN.md states for the library's host side; phi.cos() /
// phi.sin() of the normal-incidence branch are the deterministic det_sincos.
#pragma once
#include <algorithm>

#include "o_shapes.h"

namespace oracle {

// reflection.rs:71-124 (cos_theta / abs_cos_theta / same_hemisphere live in o_reflection.h)
inline Float mf_cos2_theta(const Vector3f& w) { return w.z * w.z; }
inline Float mf_sin2_theta(const Vector3f& w) { return fmaxr(1.0f - mf_cos2_theta(w), 0.0f); }
inline Float mf_sin_theta(const Vector3f& w) { return std::sqrt(mf_sin2_theta(w)); }
inline Float mf_tan_theta(const Vector3f& w) { return mf_sin_theta(w) / w.z; }
inline Float mf_tan2_theta(const Vector3f& w) { return mf_sin2_theta(w) / mf_cos2_theta(w); }
inline Float mf_cos_phi(const Vector3f& w) {
    Float st = mf_sin_theta(w);
    return st == 0.0f ? 1.0f : clampf(w.x / st, -1.0f, 1.0f);
}
inline Float mf_sin_phi(const Vector3f& w) {
    Float st = mf_sin_theta(w);
    return st == 0.0f ? 0.0f : clampf(w.y / st, -1.0f, 1.0f);
}
inline Float mf_cos2_phi(const Vector3f& w) { return mf_cos_phi(w) * mf_cos_phi(w); }
inline Float mf_sin2_phi(const Vector3f& w) { return mf_sin_phi(w) * mf_sin_phi(w); }
// reflection.rs:139-142
inline Vector3f reflect(const Vector3f& wo, const Vector3f& n) { return -wo + n * (2.0f * wo.dot(n)); }

// reflection.rs:42-67, one channel of the Spectrum arithmetic
inline Float fr_conductor_channel(Float cos_theta_i, Float eta_i, Float eta_t, Float k) {
    cos_theta_i = clampf(cos_theta_i, -1.0f, 1.0f);
    Float eta = eta_t / eta_i;
    Float eta_k = k / eta_i;
    Float cos_theta_i2 = cos_theta_i * cos_theta_i;
    Float sin_theta_i2 = 1.0f - cos_theta_i2;
    Float eta2 = eta * eta;
    Float eta_k2 = eta_k * eta_k;
    Float t0 = eta2 - eta_k2 - sin_theta_i2;
    Float a2_plus_b2 = std::sqrt(t0 * t0 + eta2 * eta_k2 * 4.0f);
    Float t1 = a2_plus_b2 + cos_theta_i2;
    Float a = std::sqrt((a2_plus_b2 + t0) * 0.5f);
    Float t2 = a * (2.0f * cos_theta_i);
    Float rs = (t1 - t2) / (t1 + t2);
    Float t3 = a2_plus_b2 * cos_theta_i2 + sin_theta_i2 * sin_theta_i2;
    Float t4 = t2 * sin_theta_i2;
    Float rp = rs * (t3 - t4) / (t3 + t4);
    return (rp + rs) * 0.5f;
}
inline Spectrum fr_conductor(Float cos_theta_i, const Spectrum& eta_i, const Spectrum& eta_t, const Spectrum& k) {
    return Spectrum(fr_conductor_channel(cos_theta_i, eta_i.c[0], eta_t.c[0], k.c[0]),
                    fr_conductor_channel(cos_theta_i, eta_i.c[1], eta_t.c[1], k.c[1]),
                    fr_conductor_channel(cos_theta_i, eta_i.c[2], eta_t.c[2], k.c[2]));
}

inline Float fr_dielectric(Float cos_theta_i, Float eta_i, Float eta_t);  // o_reflection.h

// reflection.rs:565-612
struct Fresnel {
    virtual ~Fresnel() {}
    virtual Spectrum evaluate(Float cos_i) const = 0;
};
struct FresnelConductor : Fresnel {
    Spectrum eta_i, eta_t, k;
    FresnelConductor(const Spectrum& ei, const Spectrum& et, const Spectrum& k_) : eta_i(ei), eta_t(et), k(k_) {}
    Spectrum evaluate(Float cos_i) const override { return fr_conductor(std::fabs(cos_i), eta_i, eta_t, k); }
};
struct FresnelDielectric : Fresnel {
    Float eta_i, eta_t;
    FresnelDielectric(Float ei, Float et) : eta_i(ei), eta_t(et) {}
    Spectrum evaluate(Float cos_i) const override { return Spectrum(fr_dielectric(cos_i, eta_i, eta_t)); }
};
struct FresnelNoOp : Fresnel {
    Spectrum evaluate(Float) const override { return Spectrum(1.0f); }
};

// microfacet.rs:336-384 (D65)
inline void trowbridge_reitz_sample11(Float cos_theta, Float u1, Float u2, Float* slope_x, Float* slope_y) {
    if (cos_theta > 0.9999f) {
        Float r = std::sqrt(u1 / (1.0f - u1));
        Float phi = 6.28318530718f * u2;
        Float sp, cp;
        det_sincos(phi, &sp, &cp);
        *slope_x = r * cp;
        *slope_y = r * sp;
        return;
    }
    Float sin_theta = std::sqrt(fmaxr(1.0f - cos_theta * cos_theta, 0.0f));
    Float tan_theta = sin_theta / cos_theta;
    Float a = 1.0f / tan_theta;
    Float g1 = 2.0f / (1.0f + std::sqrt(1.0f + 1.0f / (a * a)));

    Float A = 2.0f * u1 / g1 - 1.0f;
    Float tmp = 1.0f / (A * A - 1.0f);
    if (tmp > 1e10f) tmp = 1e10f;
    Float b = tan_theta;
    Float d = std::sqrt(fmaxr(b * b * tmp * tmp - (A * A - b * b) * tmp, 0.0f));
    Float slope_x_1 = b * tmp - d;
    Float slope_x_2 = b * tmp + d;
    *slope_x = (A < 0.0f || slope_x_2 > 1.0f / tan_theta) ? slope_x_1 : slope_x_2;

    Float s;
    if (u2 > 0.5f) {
        s = 1.0f;
        u2 = 2.0f * (u2 - 0.5f);
    } else {
        s = -1.0f;
        u2 = 2.0f * (0.5f - u2);
    }
    Float z = (u2 * (u2 * (u2 * 0.27385f - 0.73369f) + 0.46341f)) /
              (u2 * (u2 * (u2 * 0.093073f + 0.309420f) - 1.00000f) + 0.597999f);
    *slope_y = s * z * std::sqrt(1.0f + *slope_x * *slope_x);
}

// microfacet.rs:386-406 (D64)
inline Vector3f trowbridge_reitz_sample(const Vector3f& wi, Float alpha_x, Float alpha_y, Float u1, Float u2) {
    Vector3f wi_stretched = Vector3f(alpha_x * wi.x, alpha_y * wi.y, wi.z).normalize();
    Float slope_x = 0.0f, slope_y = 0.0f;
    trowbridge_reitz_sample11(wi_stretched.z, u1, u2, &slope_x, &slope_y);
    Float tmp = mf_cos_phi(wi_stretched) * slope_x - mf_sin_phi(wi_stretched) * slope_y;
    slope_y = mf_sin_phi(wi_stretched) * slope_x + mf_cos_phi(wi_stretched) * slope_y;
    slope_x = tmp;
    slope_x = alpha_x * slope_x;
    slope_y = alpha_y * slope_y;
    return Vector3f(-slope_x, -slope_y, 1.0f).normalize();
}

// microfacet.rs:11-30, 145-248
struct TrowbridgeReitzDistribution {
    Float alphax, alphay;
    TrowbridgeReitzDistribution(Float ax, Float ay) : alphax(ax), alphay(ay) {}
    // microfacet.rs:160-169
    static Float roughness_to_alpha(Float roughness) {
        double x = std::log(std::max((double)roughness, 1e-3));
        return (Float)(1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x * x * x + 0.000640711 * x * x * x * x);
    }
    // microfacet.rs:176-186
    Float d(const Vector3f& wh) const {
        Float tan2_theta = mf_tan2_theta(wh);
        if (std::isinf(tan2_theta)) return 0.0f;
        Float cos4_theta = mf_cos2_theta(wh) * mf_cos2_theta(wh);
        Float e = (mf_cos2_phi(wh) / (alphax * alphax) + mf_sin2_phi(wh) / (alphay * alphay)) * tan2_theta;
        return 1.0f / (PI * alphax * alphay * cos4_theta * (1.0f + e) * (1.0f + e));
    }
    // microfacet.rs:188-199
    Float lambda(const Vector3f& w) const {
        Float abs_tan_theta = std::fabs(mf_tan_theta(w));
        if (std::isinf(abs_tan_theta)) return 0.0f;
        Float alpha = std::sqrt(mf_cos2_phi(w) * alphax * alphax + mf_sin2_phi(w) * alphay * alphay);
        Float alpha2_tan2_theta = (alpha * abs_tan_theta) * (alpha * abs_tan_theta);
        return (-1.0f + std::sqrt(1.0f + alpha2_tan2_theta)) / 2.0f;
    }
    // microfacet.rs:15-20
    Float g1(const Vector3f& w) const { return 1.0f / (1.0f + lambda(w)); }
    Float g(const Vector3f& wo, const Vector3f& wi) const { return 1.0f / (1.0f + lambda(wo) + lambda(wi)); }
    // microfacet.rs:23-29, sample_visible_area on
    Float pdf(const Vector3f& wo, const Vector3f& wh) const { return d(wh) * g1(wo) * wo.abs_dot(wh) / std::fabs(wo.z); }
    // microfacet.rs:228-241
    Vector3f sample_wh(const Vector3f& wo, const Point2f& u) const {
        bool flip = wo.z < 0.0f;
        Vector3f wh = trowbridge_reitz_sample(flip ? -wo : wo, alphax, alphay, u.x, u.y);
        if (flip) wh = -wh;
        return wh;
    }
};

}  // namespace oracle
