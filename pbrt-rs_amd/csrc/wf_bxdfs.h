// wf_bxdfs.h — the BxDFs of the rows pbrt_hip_scene_set_material writes: OrenNayar (matte with sigma > 0), MicrofacetReflection
// with FresnelDielectric(1, eta) and MicrofacetTransmission (glass with roughness), FresnelBlend (substrate), and BSDF::f /
// pdf / sample_f over every non-specular lobe set of the renderer (part of wavefront.h). The shading kernels' level-2
// instantiations use it; the rows of matte / plastic / metal go through wf_microfacet.h's functions unchanged.
// Semantics and departures: DESIGN.md D68-D72.
#pragma once
#include "wf_microfacet.h"

namespace pb {

// OrenNayar::f (reflection.rs:944-970; D68: A and B from sigma in radians, computed on the host; D69: cos(phi_i - phi_o))
PB_DEV V3 oren_nayar_f(V3 r, float a, float b, V3 wo, V3 wi) {
    float sin_theta_i = __builtin_sqrtf(mf_sin2_theta(wi)), sin_theta_o = __builtin_sqrtf(mf_sin2_theta(wo));
    float max_cos = 0.0f;
    if (sin_theta_i > 1e-4f && sin_theta_o > 1e-4f) {
        float d_cos = mf_cos_phi(wi) * mf_cos_phi(wo) + mf_sin_phi(wi) * mf_sin_phi(wo);
        max_cos = fmaxr(d_cos, 0.0f);
    }
    float sin_alpha, tan_beta;
    if (__builtin_fabsf(wi.z) > __builtin_fabsf(wo.z)) {
        sin_alpha = sin_theta_o;
        tan_beta = sin_theta_i / __builtin_fabsf(wi.z);
    } else {
        sin_alpha = sin_theta_i;
        tan_beta = sin_theta_o / __builtin_fabsf(wo.z);
    }
    return r * kInvPi * (a + b * max_cos * sin_alpha * tan_beta);
}

// MicrofacetReflection::f (reflection.rs:1000-1018) with FresnelDielectric(eta_i, eta): (1, eta) is the reflection lobe of rough
// glass and of uber, (1.5, 1) plastic's in a lobe list (wf_lobes.h)
PB_DEV V3 glass_reflection_f(V3 r, float ax, float ay, float eta, V3 wo, V3 wi, float eta_i = 1.0f) {
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    float cos_o = __builtin_fabsf(wo.z), cos_i = __builtin_fabsf(wi.z);
    V3 wh = wi + wo;
    if (cos_i == 0.0f || cos_o == 0.0f) return zero;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return zero;
    wh = normalize(wh);
    float F = fr_dielectric(dot(wi, faceforward(wh, V3{0.0f, 0.0f, 1.0f})), eta_i, eta);
    return r * tr_d(wh, ax, ay) * tr_g(wo, wi, ax, ay) * F / (4.0f * cos_i * cos_o);
}
// MicrofacetReflection::pdf (reflection.rs:1045-1051)
PB_DEV float tr_reflection_pdf(float ax, float ay, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0.0f)) return 0.0f;
    V3 wh = normalize(wo + wi);
    return tr_pdf(wo, wh, ax, ay) / (4.0f * dot(wo, wh));
}

// MicrofacetTransmission::f (reflection.rs:1093-1138) with eta_a = 1, eta_b = eta, TransportMode::Radiance.
// D71: a zero generalised half vector (eta == 1, wi == -wo) gives 0 instead of a NaN. D72: 0 as well when wo or wi sees the
// microfacet from behind (Walter et al.'s chi+ of G1, which pbrt-v3's G leaves out and its sampler never produces).
PB_DEV V3 microfacet_transmission_f(V3 t, float ax, float ay, float eta_b, V3 wo, V3 wi) {
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    if (wo.z * wi.z > 0.0f) return zero;
    float cos_o = wo.z, cos_i = wi.z;
    if (cos_i == 0.0f || cos_o == 0.0f) return zero;
    float eta = cos_o > 0.0f ? (eta_b / 1.0f) : (1.0f / eta_b);
    V3 wh = wo + wi * eta;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return zero;
    wh = normalize(wh);
    if (wh.z < 0.0f) wh = -wh;
    float ow = dot(wo, wh), iw = dot(wi, wh);
    if (ow * iw > 0.0f) return zero;  // same side of the microfacet
    if (!(ow * cos_o > 0.0f && iw * cos_i > 0.0f)) return zero;  // D72: the microfacet seen from behind
    float F = fr_dielectric(ow, 1.0f, eta_b);
    float sqrt_denom = ow + eta * iw;
    float factor = 1.0f / eta;
    float v = __builtin_fabsf((tr_d(wh, ax, ay) * tr_g(wo, wi, ax, ay) * eta * eta * __builtin_fabsf(iw) * __builtin_fabsf(ow) * factor * factor) /
                              (cos_i * cos_o * sqrt_denom * sqrt_denom));
    return t * (1.0f - F) * v;
}
// MicrofacetTransmission::pdf (reflection.rs:1171-1187; D70: the Jacobian divides by the square of the denominator; D71, D72)
PB_DEV float microfacet_transmission_pdf(float ax, float ay, float eta_b, V3 wo, V3 wi) {
    if (wo.z * wi.z > 0.0f) return 0.0f;
    float eta = wo.z > 0.0f ? (eta_b / 1.0f) : (1.0f / eta_b);
    V3 wh = wo + wi * eta;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return 0.0f;
    wh = normalize(wh);
    if (wh.z < 0.0f) wh = -wh;
    float ow = dot(wo, wh), iw = dot(wi, wh);
    if (ow * iw > 0.0f) return 0.0f;
    if (!(ow * wo.z > 0.0f && iw * wi.z > 0.0f)) return 0.0f;  // D72
    float sqrt_denom = ow + eta * iw;
    float dwh_dwi = __builtin_fabsf((eta * eta * iw) / (sqrt_denom * sqrt_denom));
    return tr_pdf(wo, wh, ax, ay) * dwh_dwi;
}

// FresnelBlend::f (reflection.rs:1211-1238)
PB_DEV float pow5(float v) { return (v * v) * (v * v) * v; }
PB_DEV V3 fresnel_blend_f(V3 rd, V3 rs, float ax, float ay, V3 wo, V3 wi) {
    V3 one = V3{1.0f, 1.0f, 1.0f};
    float cos_i = __builtin_fabsf(wi.z), cos_o = __builtin_fabsf(wo.z);
    V3 diffuse = mulv(rd * (28.0f / (23.0f * kPi)), one - rs) * (1.0f - pow5(1.0f - 0.5f * cos_i)) * (1.0f - pow5(1.0f - 0.5f * cos_o));
    V3 wh = wi + wo;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return V3{0.0f, 0.0f, 0.0f};
    wh = normalize(wh);
    V3 schlick = rs + (one - rs) * pow5(1.0f - dot(wi, wh));
    V3 specular = schlick * (tr_d(wh, ax, ay) / (4.0f * absdot(wi, wh) * fmaxr(cos_i, cos_o)));
    return diffuse + specular;
}
// FresnelBlend::pdf (reflection.rs:1267-1275)
PB_DEV float fresnel_blend_pdf(float ax, float ay, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0.0f)) return 0.0f;
    V3 wh = normalize(wo + wi);
    float pdf_wh = tr_pdf(wo, wh, ax, ay);
    return 0.5f * (__builtin_fabsf(wi.z) * kInvPi + pdf_wh / (4.0f * dot(wo, wh)));
}

// Every non-specular lobe set: kind 0 = the rows of matte / plastic / metal (`ns`, evaluated by wf_microfacet.h), otherwise
// the row of pbrt_hip_scene_set_material, whose colours and alphas sit in ns.kd / ns.ks / ns.ax / ns.ay:
//   kMatOrenNayar   OrenNayar(kd; A = ax, B = ay)
//   kMatRoughGlass  MicrofacetReflection(kd = Kr) if Kr is not black, then MicrofacetTransmission(ks = Kt) if Kt is not black
//   kMatSubstrate   FresnelBlend(kd, ks)
struct GenBsdf {
    NsBsdf ns;
    int kind;
    int n;        // number of lobes, 0..2
    float eta;    // rough glass
    bool first;   // rough glass: the reflection lobe is there (it is lobe 0 then)
    bool second;  // rough glass: the transmission lobe is there
};
PB_DEV GenBsdf gen_bsdf(const DevMaterial& m) {
    GenBsdf b;
    b.ns = ns_bsdf(m);
    b.kind = m.type >= kMatOrenNayar ? m.type : 0;
    b.eta = m.eta;
    b.first = b.second = false;
    b.n = b.ns.n;
    if (b.kind == kMatOrenNayar) {
        b.n = is_black(b.ns.kd) ? 0 : 1;
    } else if (b.kind == kMatRoughGlass) {
        b.first = !is_black(b.ns.kd);
        b.second = !is_black(b.ns.ks);
        b.n = (b.first ? 1 : 0) + (b.second ? 1 : 0);
    } else if (b.kind == kMatSubstrate) {
        b.n = (is_black(b.ns.kd) && is_black(b.ns.ks)) ? 0 : 1;
    }
    return b;
}

// BSDF::f over the lobes of a set_material row, local directions: reflection lobes when wi and wo are on the same side of ng
// (`reflect`), transmission lobes otherwise (reflection.rs:271-283)
PB_DEV V3 gen_lobes_f(const GenBsdf& b, V3 wo, V3 wi, bool reflect) {
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    if (b.kind == kMatOrenNayar) return reflect ? oren_nayar_f(b.ns.kd, b.ns.ax, b.ns.ay, wo, wi) : zero;
    if (b.kind == kMatSubstrate) return reflect ? fresnel_blend_f(b.ns.kd, b.ns.ks, b.ns.ax, b.ns.ay, wo, wi) : zero;
    if (reflect) return b.first ? glass_reflection_f(b.ns.kd, b.ns.ax, b.ns.ay, b.eta, wo, wi) : zero;
    return b.second ? microfacet_transmission_f(b.ns.ks, b.ns.ax, b.ns.ay, b.eta, wo, wi) : zero;
}
// the sum of the lobes' pdfs (BSDF::pdf before the division by their number)
PB_DEV float gen_lobes_pdf_sum(const GenBsdf& b, V3 wo, V3 wi) {
    if (b.kind == kMatOrenNayar) return lambert_pdf(wo, wi);  // the BxDF trait's default pdf
    if (b.kind == kMatSubstrate) return fresnel_blend_pdf(b.ns.ax, b.ns.ay, wo, wi);
    float p = 0.0f;
    if (b.first) p = p + tr_reflection_pdf(b.ns.ax, b.ns.ay, wo, wi);
    if (b.second) p = p + microfacet_transmission_pdf(b.ns.ax, b.ns.ay, b.eta, wo, wi);
    return p;
}

// BSDF::f and BSDF::pdf (reflection.rs:264-283, 420-448)
PB_DEV void gen_f_pdf(const GenBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    if (b.kind == 0) {
        ns_f_pdf(b.ns, fr, wo_w, wi_w, f, pdf);
        return;
    }
    V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f || b.n == 0) return;
    bool reflect = dot(wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    *f = gen_lobes_f(b, wo, wi, reflect);
    *pdf = gen_lobes_pdf_sum(b, wo, wi) / (float)b.n;
}
// BSDF::sample_f (reflection.rs:285-381) with the lobes' own sample_f: OrenNayar the trait's cosine hemisphere (:459-472),
// MicrofacetReflection (:1020-1043, D63), MicrofacetTransmission (:1140-1169: a visible normal, then refract), FresnelBlend
// (:1240-1265: u0 < 0.5 cosine hemisphere, else a visible normal and reflect, u0 remapped). Outputs as ns_sample_f.
PB_DEV V3 gen_sample_f(const GenBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok, int* sampled) {
    if (b.kind == 0) return ns_sample_f(b.ns, fr, wo_w, u0, u1, wi_w, pdf, ok, sampled);
    *ok = false;
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    if (b.n == 0) {
        *pdf = 0.0f;
        return zero;
    }
    const float nf = (float)b.n;
    int comp = (int)__builtin_floorf(u0 * nf);
    comp = comp < b.n - 1 ? comp : b.n - 1;
    float ur = fminr(u0 * nf - (float)comp, kOneMinusEpsilon);
    V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;
    const float ax = b.ns.ax, ay = b.ns.ay;
    V3 wi = zero;
    float p = 0.0f;
    int type = kBxdfReflection | kBxdfGlossy;
    if (b.kind == kMatOrenNayar) {
        type = kBxdfReflection | kBxdfDiffuse;
        wi = cosine_sample_hemisphere(ur, u1);
        if (wo.z < 0.0f) wi.z *= -1.0f;
        p = lambert_pdf(wo, wi);
    } else if (b.kind == kMatSubstrate) {
        bool sampled_wi = true;
        if (ur < 0.5f) {
            wi = cosine_sample_hemisphere(fminr(2.0f * ur, kOneMinusEpsilon), u1);
            if (wo.z < 0.0f) wi.z *= -1.0f;
        } else {
            V3 wh = tr_sample_wh(wo, ax, ay, fminr(2.0f * (ur - 0.5f), kOneMinusEpsilon), u1);
            wi = -wo + wh * (2.0f * dot(wo, wh));
            sampled_wi = wo.z * wi.z > 0.0f;
        }
        if (sampled_wi) p = fresnel_blend_pdf(ax, ay, wo, wi);
    } else {
        const bool transmit = !(b.first && comp == 0);
        V3 wh = tr_sample_wh(wo, ax, ay, ur, u1);
        float wo_wh = dot(wo, wh);
        if (!transmit) {
            if (!(wo_wh < 0.0f)) {
                wi = -wo + wh * (2.0f * wo_wh);
                if (wo.z * wi.z > 0.0f) p = tr_pdf(wo, wh, ax, ay) / (4.0f * wo_wh);
            }
        } else {
            type = kBxdfTransmission | kBxdfGlossy;
            float eta = wo.z > 0.0f ? (1.0f / b.eta) : (b.eta / 1.0f);
            if (!(wo_wh < 0.0f) && refract(wo, wh, eta, &wi)) p = microfacet_transmission_pdf(ax, ay, b.eta, wo, wi);
        }
        if (p != 0.0f && b.n > 1)  // the other lobe's pdf at the sampled direction
            p = p + (transmit ? tr_reflection_pdf(ax, ay, wo, wi) : microfacet_transmission_pdf(ax, ay, b.eta, wo, wi));
    }
    *pdf = p;
    if (!(p != 0.0f)) return zero;
    *wi_w = to_world(fr, wi);
    *ok = true;
    *sampled = type;
    *pdf = p / nf;
    bool reflect = dot(*wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    return gen_lobes_f(b, wo, wi, reflect);
}

PB_DEV void bsdf_f_pdf(const GenBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) { gen_f_pdf(b, fr, wo_w, wi_w, f, pdf); }
PB_DEV V3 bsdf_sample_f(const GenBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    int sampled;
    return gen_sample_f(b, fr, wo_w, u0, u1, wi_w, pdf, ok, &sampled);
}

// The BSDF type of a shading-kernel instantiation level: 0 matte only (MatteBsdf, built in place), 1 plus plastic / metal,
// 2 plus the rows of pbrt_hip_scene_set_material, 3 plus Disney rows (wf_disney.h, load_bsdf there)
template <int LEVEL>
struct LevelBsdf {
    typedef NsBsdf type;
};
template <>
struct LevelBsdf<2> {
    typedef GenBsdf type;
};

}  // namespace pb
