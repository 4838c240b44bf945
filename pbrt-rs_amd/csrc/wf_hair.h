// wf_hair.h — pbrt-v3's HairBSDF (Chiang et al.: lobes R, TT, TRT and a residual, pMax = 3) for the kMatHair rows of a scene with
// curves, as a BSDF type of the shading kernels. Included by hair_kernels.hip alone, behind wavefront.h: the translation units of
// the older kernels never see it. DESIGN.md D107-D114; tests/hair_model.py is the float64 model it is held to.
//
// Frame: x runs along the fibre (fr.ss = normalize(shading.dpdu)): sin(theta) = w.x, phi = atan2(w.z, w.y). h = -1 + 2 v of the
// curve's hit. Nothing here is indexed by a runtime p: the three lobes are written out, and the sampler picks with selects.
#pragma once
#include "wf_lobes.h"

namespace pb {

PB_DEV float hair_safe_sqrt(float x) { return __builtin_sqrtf(fmaxr(x, 0.0f)); }
PB_DEV float hair_safe_asin(float x) { return kPiOver2 - det_acos(clampf(x, -1.0f, 1.0f)); }

// I0(x) = sum_{i < 20} (x^2 / 4)^i / (i!)^2, nested: 1 + t (1 + t / 4 (1 + t / 9 (...))). pbrt-v3 stops after ten terms, short by
// 1.5 % at x = 12, the end of the range the series serves, and Mp is then not normalised: the normalisations decide (D112).
PB_DEV float hair_i0(float x) {
    const float t = x * x * 0.25f;
    float val = 1.0f;
#pragma unroll
    for (int i = 19; i >= 1; --i) val = 1.0f + t * (1.0f / (float)(i * i)) * val;
    return val;
}
// log I0: past 12 the asymptotic series x - log(2 pi x) / 2 + log(1 + 1 / (8 x) + 9 / (128 x^2) + 225 / (3072 x^3)), 5e-6 at
// x = 12 (pbrt-v3 has 1 / (16 x) for the last logarithm and is 0.5 % short there: D112)
PB_DEV float hair_log_i0(float x) {
    if (x > 12.0f) {
        const float r = 1.0f / x;
        return x + 0.5f * (-1.8378770664093453f + logf(r)) + logf(1.0f + 0.125f * r * (1.0f + 0.5625f * r * (1.0f + (25.0f / 24.0f) * r)));
    }
    return logf(hair_i0(x));
}
// the longitudinal scattering function
PB_DEV float hair_mp(float cos_i, float cos_o, float sin_i, float sin_o, float v) {
    const float a = cos_i * cos_o / v, b = sin_i * sin_o / v;
    if (v <= 0.1f) return expf(hair_log_i0(a) - b - 1.0f / v + 0.6931f + logf(1.0f / (2.0f * v)));
    return expf(-b) * hair_i0(a) / (sinhf(1.0f / v) * 2.0f * v);
}
// the azimuthal one: the logistic of scale s trimmed to [-pi, pi] around Phi(p) = 2 p gamma_t - 2 gamma_o + p pi
PB_DEV float hair_np(float phi, float p, const DevHair* hr, float gamma_o, float gamma_t) {
    float dphi = phi - (2.0f * p * gamma_t - 2.0f * gamma_o + p * kPi);
    dphi = dphi - 2.0f * kPi * __builtin_rintf(dphi * kInv2Pi);  // into [-pi, pi]
    const float s = hr->s;
    const float e = expf(-__builtin_fabsf(dphi) / s);
    return e / (s * (1.0f + e) * (1.0f + e)) / hr->trim_k;
}

// what f, pdf and sample_f share at one (wo, h): the angles and the attenuations Ap
struct HairGeom {
    float sin_o, cos_o, phi_o, gamma_o, gamma_t;
    V3 ap0, ap1, ap2, ap3;
};
PB_DEV HairGeom hair_geometry(const DevHair* hr, float h, V3 wo) {
    HairGeom g;
    const float eta = hr->eta;
    g.sin_o = wo.x;
    g.cos_o = hair_safe_sqrt(1.0f - g.sin_o * g.sin_o);
    g.phi_o = det_atan2(wo.z, wo.y);
    const float sin_t = g.sin_o / eta;
    const float cos_t = hair_safe_sqrt(1.0f - sin_t * sin_t);
    const float etap = __builtin_sqrtf(eta * eta - g.sin_o * g.sin_o) / g.cos_o;
    const float sin_gt = h / etap;
    const float cos_gt = hair_safe_sqrt(1.0f - sin_gt * sin_gt);
    g.gamma_t = hair_safe_asin(sin_gt);
    g.gamma_o = hair_safe_asin(h);
    const float len = 2.0f * cos_gt / cos_t;
    const V3 T = V3{expf(-hr->sigma_a[0] * len), expf(-hr->sigma_a[1] * len), expf(-hr->sigma_a[2] * len)};
    const float cos_go = hair_safe_sqrt(1.0f - h * h);
    const float F = fr_dielectric(g.cos_o * cos_go, 1.0f, eta);
    const float q = (1.0f - F) * (1.0f - F);
    g.ap0 = V3{F, F, F};
    g.ap1 = T * q;
    g.ap2 = mulv(g.ap1, T) * F;
    // 1 - T F == 0 only where F == 1 and T == 1 (h = +-1 or a grazing wo, no absorption): ap2 is 0 there and so is the residual (D111)
    const V3 den = V3{1.0f - T.x * F, 1.0f - T.y * F, 1.0f - T.z * F};
    g.ap3 = V3{den.x == 0.0f ? 0.0f : g.ap2.x * F * T.x / den.x, den.y == 0.0f ? 0.0f : g.ap2.y * F * T.y / den.y,
               den.z == 0.0f ? 0.0f : g.ap2.z * F * T.z / den.z};
    return g;
}
PB_DEV float hair_y(V3 c) { return 0.212671f * c.x + 0.715160f * c.y + 0.072169f * c.z; }

// the outgoing angles tilted by the scales of lobe P (0, 1, 2)
template <int P>
PB_DEV void hair_tilt(const DevHair* hr, float sin_o, float cos_o, float* sin_op, float* cos_op) {
    if (P == 0) {
        *sin_op = sin_o * hr->cos2k[1] - cos_o * hr->sin2k[1];
        *cos_op = cos_o * hr->cos2k[1] + sin_o * hr->sin2k[1];
    } else if (P == 1) {
        *sin_op = sin_o * hr->cos2k[0] + cos_o * hr->sin2k[0];
        *cos_op = cos_o * hr->cos2k[0] - sin_o * hr->sin2k[0];
    } else {
        *sin_op = sin_o * hr->cos2k[2] + cos_o * hr->sin2k[2];
        *cos_op = cos_o * hr->cos2k[2] - sin_o * hr->sin2k[2];
    }
}

// f's sum (before the division by |wi.z|) and the pdf's, which differ in the weights alone: ap[p] and ap[p].y / sum ap.y
PB_DEV void hair_lobes(const DevHair* hr, const HairGeom& g, float sin_i, float cos_i, float phi, V3* f, float* pdf) {
    const float y0 = hair_y(g.ap0), y1 = hair_y(g.ap1), y2 = hair_y(g.ap2), y3 = hair_y(g.ap3);
    const float ysum = y0 + y1 + y2 + y3;
    float sin_op, cos_op, w;
    hair_tilt<0>(hr, g.sin_o, g.cos_o, &sin_op, &cos_op);
    w = hair_mp(cos_i, __builtin_fabsf(cos_op), sin_i, sin_op, hr->v[0]) * hair_np(phi, 0.0f, hr, g.gamma_o, g.gamma_t);
    V3 fs = g.ap0 * w;
    float ps = w * (y0 / ysum);
    hair_tilt<1>(hr, g.sin_o, g.cos_o, &sin_op, &cos_op);
    w = hair_mp(cos_i, __builtin_fabsf(cos_op), sin_i, sin_op, hr->v[1]) * hair_np(phi, 1.0f, hr, g.gamma_o, g.gamma_t);
    fs = fs + g.ap1 * w;
    ps = ps + w * (y1 / ysum);
    hair_tilt<2>(hr, g.sin_o, g.cos_o, &sin_op, &cos_op);
    w = hair_mp(cos_i, __builtin_fabsf(cos_op), sin_i, sin_op, hr->v[2]) * hair_np(phi, 2.0f, hr, g.gamma_o, g.gamma_t);
    fs = fs + g.ap2 * w;
    ps = ps + w * (y2 / ysum);
    w = hair_mp(cos_i, g.cos_o, sin_i, g.sin_o, hr->v[3]) / (2.0f * kPi);
    *f = fs + g.ap3 * w;
    *pdf = ps + w * (y3 / ysum);
}

// BSDF::f and BSDF::pdf with HairBSDF as the only lobe (GLOSSY | REFLECTION | TRANSMISSION: the side of ng selects nothing away)
PB_DEV void hair_f_pdf(const DevHair* hr, float h, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    const V3 wi = to_local(fr, wi_w), wo = to_local(fr, wo_w);
    *f = V3{0.0f, 0.0f, 0.0f};
    *pdf = 0.0f;
    if (wo.z == 0.0f) return;
    const HairGeom g = hair_geometry(hr, h, wo);
    const float sin_i = wi.x, cos_i = hair_safe_sqrt(1.0f - sin_i * sin_i);
    const float phi = det_atan2(wi.z, wi.y) - g.phi_o;
    hair_lobes(hr, g, sin_i, cos_i, phi, f, pdf);
    const float az = __builtin_fabsf(wi.z);
    if (az > 0.0f) *f = *f / az;
}

// DemuxFloat: the even and the odd bits of uint64(u 2^32), each over 2^16
PB_DEV uint32_t hair_compact1by1(uint64_t v) {
    uint32_t x = (uint32_t)v & 0x55555555u;
    x = (x ^ (x >> 1)) & 0x33333333u;
    x = (x ^ (x >> 2)) & 0x0f0f0f0fu;
    x = (x ^ (x >> 4)) & 0x00ff00ffu;
    x = (x ^ (x >> 8)) & 0x0000ffffu;
    return x;
}
PB_DEV void hair_demux(float u, float* a, float* b) {
    const uint64_t bits = (uint64_t)(u * 4294967296.0f);
    *a = (float)hair_compact1by1(bits) * (1.0f / 65536.0f);
    *b = (float)hair_compact1by1(bits >> 1) * (1.0f / 65536.0f);
}

// BSDF::sample_f with HairBSDF as the only lobe: u0 is remapped for one component; the value is f(wo, wi), the pdf the lobes' sum
// at the sampled angles. Never specular. Outputs as dz_sample_f's.
PB_DEV V3 hair_sample_f(const DevHair* hr, float h, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    *ok = false;
    const V3 zero = V3{0.0f, 0.0f, 0.0f};
    const V3 wo = to_local(fr, wo_w);
    if (wo.z == 0.0f) return zero;
    const float ur = fminr(u0 * 1.0f - 0.0f, kOneMinusEpsilon);
    float u00, u01, u10, u11;
    hair_demux(ur, &u00, &u01);
    hair_demux(u1, &u10, &u11);
    const HairGeom g = hair_geometry(hr, h, wo);
    const float y0 = hair_y(g.ap0), y1 = hair_y(g.ap1), y2 = hair_y(g.ap2), y3 = hair_y(g.ap3);
    const float ysum = y0 + y1 + y2 + y3;
    // p: u00 walked through apPdf[0..2]
    const float q0 = y0 / ysum, q1 = y1 / ysum, q2 = y2 / ysum;
    const float r1 = u00 - q0, r2 = r1 - q1;
    const bool t0 = u00 < q0, t1 = !t0 && r1 < q1, t2 = !t0 && !t1 && r2 < q2;
    // the p-th tilt, without the absolute value (pbrt-v3's sampler, D108)
    float s0, c0, s1, c1, s2, c2;
    hair_tilt<0>(hr, g.sin_o, g.cos_o, &s0, &c0);
    hair_tilt<1>(hr, g.sin_o, g.cos_o, &s1, &c1);
    hair_tilt<2>(hr, g.sin_o, g.cos_o, &s2, &c2);
    const float sin_op = t0 ? s0 : t1 ? s1 : t2 ? s2 : g.sin_o;
    const float cos_op = t0 ? c0 : t1 ? c1 : t2 ? c2 : g.cos_o;
    const float vp = t0 ? hr->v[0] : t1 ? hr->v[1] : t2 ? hr->v[2] : hr->v[3];
    const float pf = t0 ? 0.0f : t1 ? 1.0f : 2.0f;
    u10 = fmaxr(u10, 1e-5f);
    const float cos_t = 1.0f + vp * logf(u10 + (1.0f - u10) * expf(-2.0f / vp));
    const float sin_t = hair_safe_sqrt(1.0f - cos_t * cos_t);
    float sp, cp;
    det_sincos(2.0f * kPi * u11, &sp, &cp);
    const float sin_i = -cos_t * sin_op + sin_t * cp * cos_op;
    const float cos_i = hair_safe_sqrt(1.0f - sin_i * sin_i);
    float dphi;
    if (t0 || t1 || t2) {
        const float s = hr->s;
        float x = -s * logf(1.0f / (u01 * hr->trim_k + hr->cdf_lo) - 1.0f);
        x = clampf(x, -kPi, kPi);
        dphi = (2.0f * pf * g.gamma_t - 2.0f * g.gamma_o + pf * kPi) + x;
    } else {
        dphi = 2.0f * kPi * u01;
    }
    det_sincos(g.phi_o + dphi, &sp, &cp);
    const V3 wi = V3{sin_i, cos_i * cp, cos_i * sp};
    V3 f;
    float p;
    hair_lobes(hr, g, sin_i, cos_i, dphi, &f, &p);
    *pdf = p;
    if (!(p > 0.0f)) {
        *pdf = 0.0f;
        return zero;
    }
    const float az = __builtin_fabsf(wi.z);
    if (az > 0.0f) f = f / az;
    *wi_w = to_world(fr, wi);
    *ok = true;
    return f;
}

// The BSDF of a hair build: a hair row's block with the hit's h, or the row's BSDF of levels 0-3
struct HairBsdf {
    DisneyBsdf base;
    const DevHair* hr;  // null: not a hair row
    float h;            // -1 + 2 v of the curve's hit, set by the kernel after load_bsdf
    int n;
};
PB_DEV void bsdf_f_pdf(const HairBsdf& b, const Frame& fr, V3 wo_w, V3 wi_w, V3* f, float* pdf) {
    if (b.hr) hair_f_pdf(b.hr, b.h, fr, wo_w, wi_w, f, pdf);
    else bsdf_f_pdf(b.base, fr, wo_w, wi_w, f, pdf);
}
PB_DEV V3 bsdf_sample_f(const HairBsdf& b, const Frame& fr, V3 wo_w, float u0, float u1, V3* wi_w, float* pdf, bool* ok) {
    if (b.hr) return hair_sample_f(b.hr, b.h, fr, wo_w, u0, u1, wi_w, pdf, ok);
    return bsdf_sample_f(b.base, fr, wo_w, u0, u1, wi_w, pdf, ok);
}
template <>  // kHairBsdfLevel: wf_path.h
struct LevelBsdf<kHairBsdfLevel> {
    typedef HairBsdf type;
};
// the block lives in the row's slot of the Disney table (scene.h: DevHair)
PB_DEV void load_bsdf(const ShadeConsts& sc, int row, const DevMaterial& m, HairBsdf* b) {
    load_bsdf(sc, row, m, &b->base);
    b->hr = m.type == kMatHair ? (const DevHair*)(sc.disney + row) : nullptr;
    b->h = 0.0f;
    b->n = b->hr ? 1 : b->base.n;
}

}  // namespace pb
