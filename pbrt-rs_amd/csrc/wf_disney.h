// wf_disney.h — pbrt-v3's DisneyMaterial without subsurface (pbrt_hip_scene_set_disney_material): DisneyDiffuse, DisneyFakeSS,
// DisneyRetro, DisneySheen, DisneyClearcoat (GTR1) and LambertianTransmission, MicrofacetReflection / MicrofacetTransmission
// over Trowbridge-Reitz with the separable masking G1(wo) G1(wi) and the Disney Fresnel term, and BSDF::f / pdf / sample_f over
// up to eight lobes (part of wavefront.h). The shading kernels' level-3 instantiations use it; the rows of levels 0-2 go
// through wf_bxdfs.h's functions unchanged. A row's constants sit in a DevDisney block (scene.h) beside the material table and
// are read where a lobe needs them. Semantics and departures: DESIGN.md D73-D78.
#pragma once
#include "wf_bxdfs.h"

namespace pb {

constexpr int kDzCosine = kDzDiffuse | kDzFakeSS | kDzRetro | kDzSheen;  // the lobes with the BxDF trait's cosine-hemisphere sampler

// SchlickWeight
PB_DEV float dz_sw(float c) { return pow5(clampf(1.0f - c, 0.0f, 1.0f)); }

// DisneyDiffuse + DisneyFakeSS + DisneyRetro + DisneySheen of the lobes present; they share the half vector and the weights
PB_DEV V3 dz_cosine_lobes_f(const DevDisney* d, int lobes, V3 wo, V3 wi) {
    const float co = __builtin_fabsf(wo.z), ci = __builtin_fabsf(wi.z);
    const float fo = dz_sw(co), fi = dz_sw(ci);
    V3 f = V3{0.0f, 0.0f, 0.0f};
    if (lobes & kDzDiffuse) f = V3{d->diffuse[0], d->diffuse[1], d->diffuse[2]} * (kInvPi * (1.0f - fo / 2.0f) * (1.0f - fi / 2.0f));
    V3 wh = wi + wo;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return f;  // the lobes below use wh
    wh = normalize(wh);
    const float cd = dot(wi, wh);
    if (lobes & kDzFakeSS) {
        float fss90 = cd * cd * d->roughness;
        float fss = ((1.0f - fo) + fo * fss90) * ((1.0f - fi) + fi * fss90);
        f = f + V3{d->fakess[0], d->fakess[1], d->fakess[2]} * (kInvPi * 1.25f * (fss * (1.0f / (co + ci) - 0.5f) + 0.5f));
    }
    if (lobes & kDzRetro) {
        float rr = 2.0f * d->roughness * cd * cd;
        f = f + V3{d->retro[0], d->retro[1], d->retro[2]} * (kInvPi * rr * (fo + fi + fo * fi * (rr - 1.0f)));
    }
    if (lobes & kDzSheen) f = f + V3{d->sheen[0], d->sheen[1], d->sheen[2]} * dz_sw(cd);
    return f;
}

// TrowbridgeReitzDistribution::d as 1 / (pi ax ay (x^2 / ax^2 + y^2 / ay^2 + z^2)^2): tr_d's value without its 1 - cos^2, which at
// the alphas of roughness 0 (1e-3) is float32 noise a few degrees around the normal; and the visible-normal pdf over it
PB_DEV float dz_tr_d(V3 wh, float ax, float ay) {
    float x = wh.x / ax, y = wh.y / ay;
    float s = x * x + y * y + wh.z * wh.z;
    return 1.0f / (kPi * ax * ay * s * s);
}
PB_DEV float dz_tr_pdf(V3 wo, V3 wh, float ax, float ay) { return dz_tr_d(wh, ax, ay) * tr_g1(wo, ax, ay) * absdot(wo, wh) / __builtin_fabsf(wo.z); }
PB_DEV float dz_reflection_pdf(float ax, float ay, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0.0f)) return 0.0f;
    V3 wh = normalize(wo + wi);
    return dz_tr_pdf(wo, wh, ax, ay) / (4.0f * dot(wo, wh));
}
// MicrofacetTransmission::pdf as wf_bxdfs.h has it (D70-D72)
PB_DEV float dz_transmission_pdf(float ax, float ay, float eta_b, V3 wo, V3 wi) {
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
    return dz_tr_pdf(wo, wh, ax, ay) * dwh_dwi;
}

// MicrofacetReflection::f with R = 1, G = G1(wo) G1(wi) and DisneyFresnel
PB_DEV V3 dz_micro_f(const DevDisney* d, V3 wo, V3 wi) {
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    float cos_o = __builtin_fabsf(wo.z), cos_i = __builtin_fabsf(wi.z);
    V3 wh = wi + wo;
    if (cos_i == 0.0f || cos_o == 0.0f) return zero;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return zero;
    wh = normalize(wh);
    const float c = dot(wi, faceforward(wh, V3{0.0f, 0.0f, 1.0f}));
    const float fd = fr_dielectric(c, 1.0f, d->eta), sw = dz_sw(c), metallic = d->metallic;
    const float ax = d->ax, ay = d->ay;
    const float v = dz_tr_d(wh, ax, ay) * (tr_g1(wo, ax, ay) * tr_g1(wi, ax, ay)) / (4.0f * cos_i * cos_o);
    V3 schlick = V3{d->cspec0[0], d->cspec0[1], d->cspec0[2]} * (1.0f - sw) + V3{sw, sw, sw};
    float fdm = (1.0f - metallic) * fd;
    return (V3{fdm, fdm, fdm} + schlick * metallic) * v;
}

// MicrofacetTransmission::f as wf_bxdfs.h has it (D70-D72), with G = G1(wo) G1(wi) when `sep`
PB_DEV V3 dz_transmission_f(V3 t, float ax, float ay, float eta_b, bool sep, V3 wo, V3 wi) {
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
    if (ow * iw > 0.0f) return zero;
    if (!(ow * cos_o > 0.0f && iw * cos_i > 0.0f)) return zero;  // D72
    float F = fr_dielectric(ow, 1.0f, eta_b);
    float sqrt_denom = ow + eta * iw;
    float factor = 1.0f / eta;
    float g = sep ? tr_g1(wo, ax, ay) * tr_g1(wi, ax, ay) : tr_g(wo, wi, ax, ay);
    float v = __builtin_fabsf((dz_tr_d(wh, ax, ay) * g * eta * eta * __builtin_fabsf(iw) * __builtin_fabsf(ow) * factor * factor) /
                              (cos_i * cos_o * sqrt_denom * sqrt_denom));
    return t * (1.0f - F) * v;
}

// DisneyClearcoat. GTR1(cos theta_h, g) = cc_norm / (sin^2 theta_h + g^2 cos^2 theta_h) with cc_norm = (g^2 - 1) / (pi ln g^2):
// the denominator from wh.x^2 + wh.y^2, since at g = 0.001 the float32 1 - cos^2 is noise where the lobe has its mass.
PB_DEV float dz_gtr1(const DevDisney* d, float sin2, float cos2) { return d->cc_norm / (sin2 + d->cc_a2 * cos2); }
PB_DEV float dz_smith_g(float c) { return 1.0f / (c + __builtin_sqrtf(0.0625f + c * c - 0.0625f * c * c)); }  // alpha 0.25
PB_DEV float dz_clearcoat_f(const DevDisney* d, V3 wo, V3 wi) {
    V3 wh = wi + wo;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return 0.0f;
    wh = normalize(wh);
    float dr = dz_gtr1(d, wh.x * wh.x + wh.y * wh.y, wh.z * wh.z);
    float sw = dz_sw(dot(wo, wh));
    float fr = (1.0f - sw) * 0.04f + sw;
    float gr = dz_smith_g(__builtin_fabsf(wo.z)) * dz_smith_g(__builtin_fabsf(wi.z));
    return d->clearcoat * gr * fr * dr / 4.0f;
}
PB_DEV float dz_clearcoat_pdf(const DevDisney* d, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0.0f)) return 0.0f;
    V3 wh = wi + wo;
    if (wh.x == 0.0f && wh.y == 0.0f && wh.z == 0.0f) return 0.0f;
    wh = normalize(wh);
    return dz_gtr1(d, wh.x * wh.x + wh.y * wh.y, wh.z * wh.z) * __builtin_fabsf(wh.z) / (4.0f * dot(wo, wh));
}
PB_DEV float lambert_t_pdf(V3 wo, V3 wi) { return (wo.z * wi.z > 0.0f) ? 0.0f : __builtin_fabsf(wi.z) * kInvPi; }

// BSDF::f over the lobes: reflection lobes when wi and wo are on the same side of ng, transmission lobes otherwise
PB_DEV V3 dz_lobes_f(const DevDisney* d, V3 wo, V3 wi, bool reflect) {
    const int lobes = d->lobes;
    if (reflect) {
        V3 f = dz_micro_f(d, wo, wi);
        if (lobes & kDzCosine) f = f + dz_cosine_lobes_f(d, lobes, wo, wi);
        if (lobes & kDzClearcoat) {
            float c = dz_clearcoat_f(d, wo, wi);
            f = f + V3{c, c, c};
        }
        return f;
    }
    V3 f = V3{0.0f, 0.0f, 0.0f};
    if (lobes & kDzTrans) f = dz_transmission_f(V3{d->trans[0], d->trans[1], d->trans[2]}, d->tax, d->tay, d->eta, d->sep_trans != 0, wo, wi);
    if (lobes & kDzLambertT) f = f + V3{d->lambert_t[0], d->lambert_t[1], d->lambert_t[2]} * kInvPi;
    return f;
}
// the sum of the pdfs of the lobes in `lobes` (BSDF::pdf before the division by the lobe count)
PB_DEV float dz_pdf_sum(const DevDisney* d, int lobes, V3 wo, V3 wi) {
    float p = 0.0f;
    if (lobes & kDzCosine) p = (float)__builtin_popcount(lobes & kDzCosine) * lambert_pdf(wo, wi);
    if (lobes & kDzMicro) p = p + dz_reflection_pdf(d->ax, d->ay, wo, wi);
    if (lobes & kDzClearcoat) p = p + dz_clearcoat_pdf(d, wo, wi);
    if (lobes & kDzTrans) p = p + dz_transmission_pdf(d->tax, d->tay, d->eta, wo, wi);
    if (lobes & kDzLambertT) p = p + lambert_t_pdf(wo, wi);
    return p;
}

// The BSDF of a level-3 kernel: a Disney row's block, or the row's BSDF of levels 0-2
struct DisneyBsdf {
    GenBsdf gen;
    const DevDisney* dz;  // null: not a Disney row
    int n;                // number of lobes
};
PB_DEV void dz_f_pdf(const DevDisney* d, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f) return;
    bool reflect = dot(wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    *f = dz_lobes_f(d, wo, wi, reflect);
    *pdf = dz_pdf_sum(d, d->lobes, wo, wi) / (float)d->n;
}
// BSDF::sample_f (reflection.rs:285-381): u0 picks the lobe and is remapped, the lobe's own sampler runs, the other lobes' pdfs
// are added. Outputs as ns_sample_f.
PB_DEV V3 dz_sample_f(const DevDisney* d, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok, int* sampled) {
    *ok = false;
    V3 zero = V3{0.0f, 0.0f, 0.0f};
    const int lobes = d->lobes, n = d->n;
    const float nf = (float)n;
    int comp = (int)__builtin_floorf(u0 * nf);
    comp = comp < n - 1 ? comp : n - 1;
    float ur = fminr(u0 * nf - (float)comp, kOneMinusEpsilon);
    V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;
    int rest = lobes;
    for (int k = 0; k < comp; ++k) rest &= rest - 1;
    const int which = rest & -rest;  // the comp-th lobe
    V3 wi = zero;
    float p = 0.0f;
    int type;
    if (which & (kDzCosine | kDzLambertT)) {
        const bool across = which == kDzLambertT;
        type = (across ? kBxdfTransmission : kBxdfReflection) | kBxdfDiffuse;
        wi = cosine_sample_hemisphere(ur, u1);
        if ((wo.z < 0.0f) != across) wi.z *= -1.0f;
        p = __builtin_fabsf(wi.z) * kInvPi;
    } else if (which == kDzMicro) {
        type = kBxdfReflection | kBxdfGlossy;
        const float ax = d->ax, ay = d->ay;
        V3 wh = tr_sample_wh(wo, ax, ay, ur, u1);
        float wo_wh = dot(wo, wh);
        if (!(wo_wh < 0.0f)) {
            wi = -wo + wh * (2.0f * wo_wh);
            if (wo.z * wi.z > 0.0f) p = dz_tr_pdf(wo, wh, ax, ay) / (4.0f * wo_wh);
        }
    } else if (which == kDzClearcoat) {
        type = kBxdfReflection | kBxdfGlossy;
        // cos^2 theta_h = (1 - (g^2)^(1 - u0)) / (1 - g^2) and sin^2 theta_h = (g^2)((g^2)^(-u0) - 1) / (1 - g^2), neither as a difference
        const float a2 = d->cc_a2, ln_a2 = d->cc_ln_a2;
        float cos2 = clampf(-expm1f((1.0f - ur) * ln_a2) / (1.0f - a2), 0.0f, 1.0f);
        float sin2 = clampf(a2 * expm1f(-ur * ln_a2) / (1.0f - a2), 0.0f, 1.0f);
        float cos_t = __builtin_sqrtf(cos2), sin_t = __builtin_sqrtf(sin2);
        float sp, cp;
        det_sincos(6.28318530718f * u1, &sp, &cp);
        V3 wh = V3{sin_t * cp, sin_t * sp, cos_t};
        if (wo.z < 0.0f) wh = -wh;
        float wo_wh = dot(wo, wh);
        wi = -wo + wh * (2.0f * wo_wh);
        if (wo.z * wi.z > 0.0f) p = dz_gtr1(d, sin2, cos2) * cos_t / (4.0f * wo_wh);
    } else {
        type = kBxdfTransmission | kBxdfGlossy;
        const float ax = d->tax, ay = d->tay, eta_b = d->eta;
        V3 wh = tr_sample_wh(wo, ax, ay, ur, u1);
        float eta = wo.z > 0.0f ? (1.0f / eta_b) : (eta_b / 1.0f);
        if (!(dot(wo, wh) < 0.0f) && refract(wo, wh, eta, &wi)) p = dz_transmission_pdf(ax, ay, eta_b, wo, wi);
    }
    *pdf = p;
    if (!(p > 0.0f)) {
        *pdf = 0.0f;
        return zero;
    }
    if (n > 1) p = p + dz_pdf_sum(d, lobes & ~which, wo, wi);
    *wi_w = to_world(fr, wi);
    *ok = true;
    *sampled = type;
    *pdf = p / nf;
    bool reflect = dot(*wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    return dz_lobes_f(d, wo, wi, reflect);
}

PB_DEV void bsdf_f_pdf(const DisneyBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    if (b.dz) dz_f_pdf(b.dz, fr, wo_w, wi_w, f, pdf);
    else gen_f_pdf(b.gen, fr, wo_w, wi_w, f, pdf);
}
PB_DEV V3 bsdf_sample_f(const DisneyBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok, int* sampled) {
    if (b.dz) return dz_sample_f(b.dz, fr, wo_w, u0, u1, wi_w, pdf, ok, sampled);
    return gen_sample_f(b.gen, fr, wo_w, u0, u1, wi_w, pdf, ok, sampled);
}
PB_DEV V3 bsdf_sample_f(const DisneyBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    int sampled;
    return bsdf_sample_f(b, fr, wo_w, u0, u1, wi_w, pdf, ok, &sampled);
}

template <>
struct LevelBsdf<3> {
    typedef DisneyBsdf type;
};
// `row`: the material's row in the table; its DevDisney block has the same index
PB_DEV void load_bsdf(const ShadeConsts& sc, int row, const DevMaterial& m, NsBsdf* b) { *b = ns_bsdf(m); }
PB_DEV void load_bsdf(const ShadeConsts& sc, int row, const DevMaterial& m, GenBsdf* b) { *b = gen_bsdf(m); }
PB_DEV void load_bsdf(const ShadeConsts& sc, int row, const DevMaterial& m, DisneyBsdf* b) {
    b->gen = gen_bsdf(m);
    b->dz = m.type == kMatDisney ? sc.disney + row : nullptr;
    b->n = b->dz ? b->dz->n : b->gen.n;
}

}  // namespace pb
