// wf_microfacet.h — the non-specular BSDF of matte / plastic / metal: LambertianReflection and MicrofacetReflection over the
// Trowbridge-Reitz distribution with visible-area sampling, FresnelDielectric / FresnelConductor, and BSDF::f / pdf / sample_f
// over those lobes (part of wavefront.h). Semantics and departures: DESIGN.md D63-D67.
#pragma once
#include "wf_surface.h"

namespace pb {

// BxDFType bits (reflection.rs BxDFType; pbrt_hip_bsdf_query's sampled_flags)
constexpr int kBxdfReflection = 1, kBxdfTransmission = 2, kBxdfDiffuse = 4, kBxdfGlossy = 8, kBxdfSpecular = 16;

// ---- shading-frame trigonometry (geometry.rs cos_theta ... sin_phi) ----
PB_DEV float mf_cos2_theta(V3 w) { return w.z * w.z; }
PB_DEV float mf_sin2_theta(V3 w) { return fmaxr(0.0f, 1.0f - mf_cos2_theta(w)); }
PB_DEV float mf_cos_phi(V3 w) {
    float st = __builtin_sqrtf(mf_sin2_theta(w));
    return st == 0.0f ? 1.0f : clampf(w.x / st, -1.0f, 1.0f);
}
PB_DEV float mf_sin_phi(V3 w) {
    float st = __builtin_sqrtf(mf_sin2_theta(w));
    return st == 0.0f ? 0.0f : clampf(w.y / st, -1.0f, 1.0f);
}

// ---- TrowbridgeReitzDistribution (microfacet.rs:145-232) ----
PB_DEV float tr_d(V3 wh, float ax, float ay) {
    float tan2 = mf_sin2_theta(wh) / mf_cos2_theta(wh);
    if (__builtin_isinf(tan2)) return 0.0f;
    float cos4 = mf_cos2_theta(wh) * mf_cos2_theta(wh);
    float cp = mf_cos_phi(wh), sp = mf_sin_phi(wh);
    float e = (cp * cp / (ax * ax) + sp * sp / (ay * ay)) * tan2;
    return 1.0f / (kPi * ax * ay * cos4 * (1.0f + e) * (1.0f + e));
}
PB_DEV float tr_lambda(V3 w, float ax, float ay) {
    float abs_tan = __builtin_fabsf(__builtin_sqrtf(mf_sin2_theta(w)) / w.z);
    if (__builtin_isinf(abs_tan)) return 0.0f;
    float cp = mf_cos_phi(w), sp = mf_sin_phi(w);
    float alpha = __builtin_sqrtf(cp * cp * ax * ax + sp * sp * ay * ay);
    float a2t2 = (alpha * abs_tan) * (alpha * abs_tan);
    return (-1.0f + __builtin_sqrtf(1.0f + a2t2)) / 2.0f;
}
PB_DEV float tr_g1(V3 w, float ax, float ay) { return 1.0f / (1.0f + tr_lambda(w, ax, ay)); }
PB_DEV float tr_g(V3 wo, V3 wi, float ax, float ay) { return 1.0f / (1.0f + tr_lambda(wo, ax, ay) + tr_lambda(wi, ax, ay)); }
// MicrofacetDistribution::pdf with sample_visible_area (microfacet.rs:23-29)
PB_DEV float tr_pdf(V3 wo, V3 wh, float ax, float ay) {
    return tr_d(wh, ax, ay) * tr_g1(wo, ax, ay) * absdot(wo, wh) / __builtin_fabsf(wo.z);
}
// trowbridge_reitz_sample11 (microfacet.rs:336-386): the slopes of a visible normal for a stretched direction with
// cos_theta. D65: the discriminant's second term carries tmp, and the rational fit ends in 0.597999, as pbrt-v3 / Heitz 2014.
PB_DEV void tr_sample11(float cos_theta, float u1, float u2, float* slope_x, float* slope_y) {
    if (cos_theta > 0.9999f) {  // normal incidence
        float r = __builtin_sqrtf(u1 / (1.0f - u1));
        float s, c;
        det_sincos(6.28318530718f * u2, &s, &c);
        *slope_x = r * c;
        *slope_y = r * s;
        return;
    }
    float sin_theta = __builtin_sqrtf(fmaxr(0.0f, 1.0f - cos_theta * cos_theta));
    float tan_theta = sin_theta / cos_theta;
    float a = 1.0f / tan_theta;
    float g1 = 2.0f / (1.0f + __builtin_sqrtf(1.0f + 1.0f / (a * a)));
    float A = 2.0f * u1 / g1 - 1.0f;
    float tmp = 1.0f / (A * A - 1.0f);
    if (tmp > 1e10f) tmp = 1e10f;
    float B = tan_theta;
    float D = __builtin_sqrtf(fmaxr(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
    float sx1 = B * tmp - D, sx2 = B * tmp + D;
    float sx = (A < 0.0f || sx2 > 1.0f / tan_theta) ? sx1 : sx2;
    float S;
    if (u2 > 0.5f) {
        S = 1.0f;
        u2 = 2.0f * (u2 - 0.5f);
    } else {
        S = -1.0f;
        u2 = 2.0f * (0.5f - u2);
    }
    float z = (u2 * (u2 * (u2 * 0.27385f - 0.73369f) + 0.46341f)) / (u2 * (u2 * (u2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
    *slope_x = sx;
    *slope_y = S * z * __builtin_sqrtf(1.0f + sx * sx);
}
// trowbridge_reitz_sample (microfacet.rs:388-406): stretch, sample, rotate, unstretch (D64: alpha times the slope), normal
PB_DEV V3 tr_sample(V3 wi, float ax, float ay, float u1, float u2) {
    V3 ws = normalize(V3{ax * wi.x, ay * wi.y, wi.z});
    float sx, sy;
    tr_sample11(ws.z, u1, u2, &sx, &sy);
    float cp = mf_cos_phi(ws), sp = mf_sin_phi(ws);
    float tmp = cp * sx - sp * sy;
    sy = sp * sx + cp * sy;
    sx = tmp;
    sx = ax * sx;
    sy = ay * sy;
    return normalize(V3{-sx, -sy, 1.0f});
}
// TrowbridgeReitzDistribution::sample_wh, visible-area branch (microfacet.rs:228-240)
PB_DEV V3 tr_sample_wh(V3 wo, float ax, float ay, float u0, float u1) {
    bool flip = wo.z < 0.0f;
    V3 wh = tr_sample(flip ? -wo : wo, ax, ay, u0, u1);
    return flip ? -wh : wh;
}

// fr_conductor (reflection.rs:42-67) of one channel with eta_i = 1
PB_DEV float fr_conductor1(float cos_theta_i, float eta_t, float k) {
    cos_theta_i = clampf(cos_theta_i, -1.0f, 1.0f);
    float eta = eta_t / 1.0f, eta_k = k / 1.0f;
    float cos2 = cos_theta_i * cos_theta_i;
    float sin2 = 1.0f - cos2;
    float eta2 = eta * eta, eta_k2 = eta_k * eta_k;
    float t0 = eta2 - eta_k2 - sin2;
    float a2_plus_b2 = __builtin_sqrtf(t0 * t0 + eta2 * eta_k2 * 4.0f);
    float t1 = a2_plus_b2 + cos2;
    float a = __builtin_sqrtf((a2_plus_b2 + t0) * 0.5f);
    float t2 = a * (2.0f * cos_theta_i);
    float rs = (t1 - t2) / (t1 + t2);
    float t3 = a2_plus_b2 * cos2 + sin2 * sin2;
    float t4 = t2 * sin2;
    float rp = rs * (t3 - t4) / (t3 + t4);
    return (rp + rs) * 0.5f;
}

// The non-specular BxDFs a material adds: MatteMaterial (sigma 0: one Lambertian lobe), PlasticMaterial, MetalMaterial.
// Lobe order as the materials add them: the Lambertian lobe first.
struct NsBsdf {
    V3 kd;          // LambertianReflection R; metal: eta
    V3 ks;          // plastic: MicrofacetReflection R; metal: k
    float ax, ay;   // TrowbridgeReitzDistribution alphas
    int n;          // number of lobes, 0..2
    bool lambert;   // a LambertianReflection lobe
    bool micro;     // a MicrofacetReflection lobe
    bool metal;     // its Fresnel is FresnelConductor(1, eta, k) with R = 1; else FresnelDielectric(1.5, 1) with R = Ks
};
PB_DEV NsBsdf ns_bsdf(const DevMaterial& m) {
    NsBsdf b;
    b.kd = V3{m.kd[0], m.kd[1], m.kd[2]};
    b.ks = V3{m.kt[0], m.kt[1], m.kt[2]};
    b.ax = m.alpha_u;
    b.ay = m.alpha_v;
    b.metal = m.type == PBRT_MAT_METAL;
    b.lambert = (m.type == PBRT_MAT_MATTE || m.type == PBRT_MAT_PLASTIC) && !is_black(b.kd);
    b.micro = b.metal || (m.type == PBRT_MAT_PLASTIC && !is_black(b.ks));
    b.n = (b.lambert ? 1 : 0) + (b.micro ? 1 : 0);
    return b;
}

// MicrofacetReflection::f (reflection.rs:1003-1024), local directions
PB_DEV V3 microfacet_f(const NsBsdf& b, V3 wo, V3 wi) {
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    float cos_o = __builtin_fabsf(wo.z), cos_i = __builtin_fabsf(wi.z);
    V3 wh = wi + wo;
    if (cos_i == 0.0f || cos_o == 0.0f) return zero;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return zero;
    wh = normalize(wh);
    float c = dot(wi, faceforward(wh, V3{0.0f, 0.0f, 1.0f}));
    V3 F, R;
    if (b.metal) {  // FresnelConductor::evaluate takes |cos|
        float ac = __builtin_fabsf(c);
        F = V3{fr_conductor1(ac, b.kd.x, b.ks.x), fr_conductor1(ac, b.kd.y, b.ks.y), fr_conductor1(ac, b.kd.z, b.ks.z)};
        R = V3{1.0f, 1.0f, 1.0f};
    } else {  // pbrt-v3's PlasticMaterial passes (eta_i, eta_t) = (1.5, 1)
        float fd = fr_dielectric(c, 1.5f, 1.0f);
        F = V3{fd, fd, fd};
        R = b.ks;
    }
    return mulv(R * tr_d(wh, b.ax, b.ay) * tr_g(wo, wi, b.ax, b.ay), F) / (4.0f * cos_i * cos_o);
}
// MicrofacetReflection::pdf (reflection.rs:1046-1052)
PB_DEV float microfacet_pdf(const NsBsdf& b, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0.0f)) return 0.0f;
    V3 wh = normalize(wo + wi);
    return tr_pdf(wo, wh, b.ax, b.ay) / (4.0f * dot(wo, wh));
}
PB_DEV float lambert_pdf(V3 wo, V3 wi) { return (wo.z * wi.z > 0.0f) ? __builtin_fabsf(wi.z) * kInvPi : 0.0f; }

// BSDF::f and BSDF::pdf over every lobe (reflection.rs:264-283, 414-446): f sums the lobes that pass the reflect test on ng,
// pdf averages the lobes. Both 0 without a lobe.
PB_DEV void ns_f_pdf(const NsBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f || b.n == 0) return;
    bool reflect = dot(wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    V3 fs = V3{0.0f, 0.0f, 0.0f};
    float ps = 0.0f;
    if (b.lambert) {
        if (reflect) fs = fs + b.kd * kInvPi;
        ps = ps + lambert_pdf(wo, wi);
    }
    if (b.micro) {
        if (reflect) fs = fs + microfacet_f(b, wo, wi);
        ps = ps + microfacet_pdf(b, wo, wi);
    }
    *f = fs;
    *pdf = ps / (float)b.n;
}
// BSDF::sample_f (reflection.rs:285-377): u0 picks the lobe and is remapped, the lobe samples wi (Lambertian: cosine
// hemisphere; MicrofacetReflection: a visible normal, D63: wi = reflect(wo, wh)), the pdf is averaged over the lobes and f
// summed over those that pass the reflect test. ok = false (and f = 0) when nothing was sampled; pdf then keeps the caller's
// value if wo.z == 0, else 0. `sampled`: the sampled lobe's BxDFType.
PB_DEV V3 ns_sample_f(const NsBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok, int* sampled) {
    *ok = false;
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    if (b.n == 0) {
        *pdf = 0.0f;
        return zero;
    }
    const float nf = (float)b.n;
    int comp = (int)__builtin_floorf(u0 * nf);
    comp = comp < b.n - 1 ? comp : b.n - 1;
    const bool use_micro = b.micro && !(b.lambert && comp == 0);
    float ur = fminr(u0 * nf - (float)comp, kOneMinusEpsilon);
    V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;
    V3 wi = zero;
    float p = 0.0f;
    if (!use_micro) {  // LambertianReflection::sample_f (reflection.rs:459-472)
        wi = cosine_sample_hemisphere(ur, u1);
        if (wo.z < 0.0f) wi.z *= -1.0f;
        p = lambert_pdf(wo, wi);
    } else {  // MicrofacetReflection::sample_f (reflection.rs:1026-1044)
        V3 wh = tr_sample_wh(wo, b.ax, b.ay, ur, u1);
        float wo_wh = dot(wo, wh);
        if (!(wo_wh < 0.0f)) {
            wi = -wo + wh * (2.0f * wo_wh);
            if (wo.z * wi.z > 0.0f) p = tr_pdf(wo, wh, b.ax, b.ay) / (4.0f * wo_wh);
        }
    }
    *pdf = p;
    if (p == 0.0f) return zero;
    *wi_w = to_world(fr, wi);
    *ok = true;
    *sampled = kBxdfReflection | (use_micro ? kBxdfGlossy : kBxdfDiffuse);
    if (b.n > 1) {
        p = p + (use_micro ? lambert_pdf(wo, wi) : microfacet_pdf(b, wo, wi));
        *pdf = p / nf;
    }
    bool reflect = dot(*wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    if (!reflect) return zero;
    V3 f = zero;
    if (b.lambert) f = f + b.kd * kInvPi;
    if (b.micro) f = f + microfacet_f(b, wo, wi);
    return f;
}

// The one Lambertian lobe of matte, for the kernels that shade no plastic or metal (their code as it was)
struct MatteBsdf {
    V3 kd;
};
PB_DEV void bsdf_f_pdf(const MatteBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) { matte_f_pdf(fr, b.kd, wo_w, wi_w, f, pdf); }
PB_DEV V3 bsdf_sample_f(const MatteBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    return matte_sample_f(fr, b.kd, wo_w, u0, u1, wi_w, pdf, ok);
}
PB_DEV void bsdf_f_pdf(const NsBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) { ns_f_pdf(b, fr, wo_w, wi_w, f, pdf); }
PB_DEV V3 bsdf_sample_f(const NsBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    int sampled;
    return ns_sample_f(b, fr, wo_w, u0, u1, wi_w, pdf, ok, &sampled);
}

}  // namespace pb
