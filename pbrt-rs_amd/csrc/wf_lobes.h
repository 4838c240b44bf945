// wf_lobes.h — the reference's general BSDF (reflection.rs:207-449) on the device: a list of up to 8 lobes of any kind, specular
// and non-specular side by side, matched by BxDFType flags (part of wavefront.h). The rows of pbrt_hip_scene_set_lobe_material
// (uber, translucent, mix) are its users; a row's list is a DevLobeRow in global memory (scene.h), written by host_lobes.cpp.
// A lane keeps the row's pointer and counts and loads one lobe per iteration: nothing is copied into a per-thread array, which
// would be indexed at run time and live in scratch. Every lobe's f and pdf is the function the closed lobe sets already call
// (wf_microfacet.h, wf_bxdfs.h, wf_disney.h; the perfect-specular ones are sample_specular_local of wf_lights.h).
// Semantics: DESIGN.md D90-D94.
#pragma once
#include "wf_lights.h"

namespace pb {

constexpr int kBxdfAll = kBxdfReflection | kBxdfTransmission | kBxdfDiffuse | kBxdfGlossy | kBxdfSpecular;
constexpr int kBxdfNonSpecular = kBxdfAll & ~kBxdfSpecular;

// BxDF::matches_flags (reflection.rs:451-457)
PB_DEV bool lobe_matches(int type, int flags) { return (type & flags) == type; }
PB_DEV V3 lobe_v3(const float* c) { return V3{c[0], c[1], c[2]}; }
// a MicrofacetReflection lobe with FresnelConductor as wf_microfacet.h's metal holds it
PB_DEV NsBsdf lobe_conductor(const DevLobe& l) {
    NsBsdf b;
    b.kd = lobe_v3(l.eta);
    b.ks = lobe_v3(l.k);
    b.ax = l.ax;
    b.ay = l.ay;
    b.n = 1;
    b.lambert = false;
    b.micro = b.metal = true;
    return b;
}
// the specular kinds as the rows sample_specular_local knows: mirror (FresnelNoOp) or glass with eta = eta_t (eta_i is 1)
PB_DEV DevMaterial lobe_specular_row(const DevLobe& l) {
    DevMaterial m;
    m.type = (l.kind == PBRT_LOBE_SPECULAR_REFLECTION && l.fresnel == PBRT_FRESNEL_NOOP) ? PBRT_MAT_MIRROR : PBRT_MAT_GLASS;
    m.eta = l.eta_t;
    return m;
}

// BxDF::f of one lobe, local directions, before ScaledBxDF's factor. The specular kinds are 0 (reflection.rs:631, 689).
PB_DEV V3 lobe_f(const DevLobe& l, V3 wo, V3 wi) {
    const V3 r = lobe_v3(l.r);
    switch (l.kind) {
        case PBRT_LOBE_LAMBERTIAN_REFLECTION:
        case PBRT_LOBE_LAMBERTIAN_TRANSMISSION: return r * kInvPi;
        case PBRT_LOBE_OREN_NAYAR: return oren_nayar_f(r, l.A, l.B, wo, wi);
        case PBRT_LOBE_MICROFACET_REFLECTION:
            if (l.fresnel == PBRT_FRESNEL_CONDUCTOR) return mulv(r, microfacet_f(lobe_conductor(l), wo, wi));
            return glass_reflection_f(r, l.ax, l.ay, l.eta_t, wo, wi, l.eta_i);
        case PBRT_LOBE_MICROFACET_TRANSMISSION: return microfacet_transmission_f(r, l.ax, l.ay, l.eta_t, wo, wi);
        case PBRT_LOBE_FRESNEL_BLEND: return fresnel_blend_f(r, lobe_v3(l.s), l.ax, l.ay, wo, wi);
        default: return V3{0.0f, 0.0f, 0.0f};
    }
}
// BxDF::pdf of one lobe; the specular kinds are 0 (reflection.rs:656, 728)
PB_DEV float lobe_pdf(const DevLobe& l, V3 wo, V3 wi) {
    switch (l.kind) {
        case PBRT_LOBE_LAMBERTIAN_REFLECTION:
        case PBRT_LOBE_OREN_NAYAR: return lambert_pdf(wo, wi);
        case PBRT_LOBE_LAMBERTIAN_TRANSMISSION: return lambert_t_pdf(wo, wi);
        case PBRT_LOBE_MICROFACET_REFLECTION: return tr_reflection_pdf(l.ax, l.ay, wo, wi);
        case PBRT_LOBE_MICROFACET_TRANSMISSION: return microfacet_transmission_pdf(l.ax, l.ay, l.eta_t, wo, wi);
        case PBRT_LOBE_FRESNEL_BLEND: return fresnel_blend_pdf(l.ax, l.ay, wo, wi);
        default: return 0.0f;
    }
}
// BxDF::sample_f of one lobe: wi and its pdf (0: nothing sampled). The value returned is the lobe's f for the specular kinds
// only; BSDF::sample_f evaluates the others again over every matching lobe. The samplers are the ones gen_sample_f and
// dz_sample_f run for the same kinds.
PB_DEV V3 lobe_sample(const DevLobe& l, V3 wo, float ur, float u1, V3* wi, float* pdf) {
    const V3 zero = V3{0.0f, 0.0f, 0.0f};
    float p = 0.0f;
    V3 f = zero;
    *wi = zero;
    switch (l.kind) {
        case PBRT_LOBE_LAMBERTIAN_REFLECTION:
        case PBRT_LOBE_OREN_NAYAR:
        case PBRT_LOBE_LAMBERTIAN_TRANSMISSION: {
            const bool across = l.kind == PBRT_LOBE_LAMBERTIAN_TRANSMISSION;
            *wi = cosine_sample_hemisphere(ur, u1);
            if ((wo.z < 0.0f) != across) wi->z *= -1.0f;
            p = across ? lambert_t_pdf(wo, *wi) : lambert_pdf(wo, *wi);
            break;
        }
        case PBRT_LOBE_MICROFACET_REFLECTION: {
            V3 wh = tr_sample_wh(wo, l.ax, l.ay, ur, u1);
            float wo_wh = dot(wo, wh);
            if (!(wo_wh < 0.0f)) {
                *wi = -wo + wh * (2.0f * wo_wh);
                if (wo.z * wi->z > 0.0f) p = tr_pdf(wo, wh, l.ax, l.ay) / (4.0f * wo_wh);
            }
            break;
        }
        case PBRT_LOBE_MICROFACET_TRANSMISSION: {
            V3 wh = tr_sample_wh(wo, l.ax, l.ay, ur, u1);
            float eta = wo.z > 0.0f ? (1.0f / l.eta_t) : (l.eta_t / 1.0f);
            if (!(dot(wo, wh) < 0.0f) && refract(wo, wh, eta, wi)) p = microfacet_transmission_pdf(l.ax, l.ay, l.eta_t, wo, *wi);
            break;
        }
        case PBRT_LOBE_FRESNEL_BLEND: {
            bool sampled_wi = true;
            if (ur < 0.5f) {
                *wi = cosine_sample_hemisphere(fminr(2.0f * ur, kOneMinusEpsilon), u1);
                if (wo.z < 0.0f) wi->z *= -1.0f;
            } else {
                V3 wh = tr_sample_wh(wo, l.ax, l.ay, fminr(2.0f * (ur - 0.5f), kOneMinusEpsilon), u1);
                *wi = -wo + wh * (2.0f * dot(wo, wh));
                sampled_wi = wo.z * wi->z > 0.0f;
            }
            if (sampled_wi) p = fresnel_blend_pdf(l.ax, l.ay, wo, *wi);
            break;
        }
        case PBRT_LOBE_SPECULAR_REFLECTION:
        case PBRT_LOBE_SPECULAR_TRANSMISSION: {
            const V3 r = lobe_v3(l.r);
            bool tr;
            f = sample_specular_local(lobe_specular_row(l), r, r, wo, ur, l.kind == PBRT_LOBE_SPECULAR_REFLECTION ? 1 : 2, wi, &p, &tr);
            break;
        }
        default: break;
    }
    *pdf = p;
    return f;
}

// BSDF::num_components (reflection.rs:241-251)
PB_DEV int lobes_num_components(const DevLobeRow* row, int flags) {
    const int n = row->n;
    int num = 0;
    for (int k = 0; k < n; ++k) num += lobe_matches(row->lobes[k].type, flags) ? 1 : 0;
    return num;
}

// BSDF::f and BSDF::pdf under a flag mask (reflection.rs:264-283, 420-448): f sums the matching lobes on the reflect side of ng,
// each under its ScaledBxDF factor; pdf averages the matching lobes (ScaledBxDF leaves it alone).
PB_DEV void lobes_f_pdf(const DevLobeRow* row, const Frame& fr, V3 wo_w, V3 wi_w, int flags, V3* f, float* pdf) {
    V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f) return;
    const bool reflect = dot(wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    const int n = row->n;
    V3 fs = V3{0.0f, 0.0f, 0.0f};
    float ps = 0.0f;
    int matching = 0;
    for (int k = 0; k < n; ++k) {
        const DevLobe l = row->lobes[k];
        if (!lobe_matches(l.type, flags)) continue;
        matching += 1;
        if (l.type & kBxdfSpecular) continue;  // f and pdf are 0
        ps = ps + lobe_pdf(l, wo, wi);
        if (l.type & (reflect ? kBxdfReflection : kBxdfTransmission)) fs = fs + mulv(lobe_v3(l.scale), lobe_f(l, wo, wi));
    }
    *f = fs;
    *pdf = matching > 0 ? ps / (float)matching : 0.0f;
}

// BSDF::sample_f under a flag mask (reflection.rs:285-381): u0 picks among the MATCHING lobes and is remapped; a specular pick
// returns that lobe's value and pdf / matching alone; any other pick adds the other matching lobes' pdfs and evaluates f again
// over the matching lobes. Outputs as ns_sample_f: ok = false and f = 0 when nothing was sampled (pdf then keeps the caller's
// value if wo.z == 0, else 0); `sampled` = the sampled lobe's BxDFType.
PB_DEV V3 lobes_sample_f(const DevLobeRow* row, const Frame& fr, V3 wo_w, float u0, float u1, int flags, V3* wi_w, float* pdf, bool* ok,
                         int* sampled) {
    *ok = false;
    const V3 zero = V3{0.0f, 0.0f, 0.0f};
    const int n = row->n;
    const int matching = lobes_num_components(row, flags);
    if (matching == 0) {
        *pdf = 0.0f;
        return zero;
    }
    const float nf = (float)matching;
    int comp = (int)__builtin_floorf(u0 * nf);
    comp = comp < matching - 1 ? comp : matching - 1;
    const float ur = fminr(u0 * nf - (float)comp, kOneMinusEpsilon);
    int idx = 0;
    for (int k = 0, count = comp; k < n; ++k) {
        if (!lobe_matches(row->lobes[k].type, flags)) continue;
        if (count == 0) {
            idx = k;
            break;
        }
        count -= 1;
    }
    V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;
    const DevLobe picked = row->lobes[idx];
    V3 wi;
    float p;
    V3 f = lobe_sample(picked, wo, ur, u1, &wi, &p);
    *pdf = p;
    if (!(p != 0.0f)) {
        *pdf = 0.0f;
        return zero;
    }
    *wi_w = to_world(fr, wi);
    *ok = true;
    *sampled = picked.type;
    if (picked.type & kBxdfSpecular) {
        *pdf = p / nf;
        return mulv(lobe_v3(picked.scale), f);
    }
    const bool reflect = dot(*wi_w, fr.ng) * dot(wo_w, fr.ng) > 0.0f;
    f = zero;
    for (int k = 0; k < n; ++k) {
        const DevLobe l = row->lobes[k];
        if (!lobe_matches(l.type, flags) || (l.type & kBxdfSpecular)) continue;
        if (k != idx) p = p + lobe_pdf(l, wo, wi);
        if (l.type & (reflect ? kBxdfReflection : kBxdfTransmission)) f = f + mulv(lobe_v3(l.scale), lobe_f(l, wo, wi));
    }
    *pdf = p / nf;
    return f;
}

// The BSDF of a lobe-list kernel: a lobe row's list, or the row's BSDF of levels 0-3. As a BSDF type of estimate_direct_emit it
// applies estimate_direct's mask BSDF_ALL & !BSDF_SPECULAR (integrator.rs:146); n counts the lobes under that mask.
struct LobeBsdf {
    DisneyBsdf base;
    const DevLobeRow* row;  // null: not a lobe row
    int n;
};
PB_DEV void bsdf_f_pdf(const LobeBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    if (b.row) lobes_f_pdf(b.row, fr, wo_w, wi_w, kBxdfNonSpecular, f, pdf);
    else bsdf_f_pdf(b.base, fr, wo_w, wi_w, f, pdf);
}
PB_DEV V3 bsdf_sample_f(const LobeBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    int sampled;
    if (b.row) return lobes_sample_f(b.row, fr, wo_w, u0, u1, kBxdfNonSpecular, wi_w, pdf, ok, &sampled);
    return bsdf_sample_f(b.base, fr, wo_w, u0, u1, wi_w, pdf, ok, &sampled);
}
template <>
struct LevelBsdf<4> {
    typedef LobeBsdf type;
};
PB_DEV void load_bsdf(const ShadeConsts& sc, int row, const DevMaterial& m, LobeBsdf* b) {
    load_bsdf(sc, row, m, &b->base);
    b->row = m.type == kMatLobes ? sc.lobe_rows + row : nullptr;
    b->n = b->row ? b->row->n_nonspec : b->base.n;
}

}  // namespace pb
