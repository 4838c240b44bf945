"""pbrt-v3's HairBSDF (Chiang et al.: lobes R, TT, TRT and a residual, pMax = 3) in numpy, as HairMaterial puts it on a curve
(DESIGN.md D107-D114). Vectorised over points; the arithmetic runs in the dtype of the inputs, so the same text is the float64
model and, with HairModel.as32() and float32 inputs, its float32 restatement.

Frame: x runs along the fibre. sin(theta) = w.x, phi = atan2(w.z, w.y). h = -1 + 2 v of the curve's hit is given per point.
"""
import math

import numpy as np

P_MAX = 3
FLAGS = 4 | 1 | 2  # BSDF_GLOSSY | BSDF_REFLECTION | BSDF_TRANSMISSION
ONE_MINUS_EPSILON = float(np.float32(1.0) - np.float32(2.0 ** -24))
EUMELANIN = (0.419, 0.697, 1.37)
PHEOMELANIN = (0.187, 0.4, 1.05)


def sigma_a_from_color(c, beta_n):
    c = np.asarray(c, np.float64)
    bn = float(beta_n)
    d = 5.969 - 0.215 * bn + 2.532 * bn ** 2 - 10.73 * bn ** 3 + 5.574 * bn ** 4 + 0.245 * bn ** 5
    return (np.log(c) / d) ** 2


def sigma_a_from_melanin(ce, cp):
    return float(ce) * np.array(EUMELANIN) + float(cp) * np.array(PHEOMELANIN)


class HairModel:
    """the constants of one row: sigma_a[3], eta, v[4], s, sin2k[3], cos2k[3], from float32 parameters, in double"""

    def __init__(self, sigma_a=(0.0, 0.0, 0.0), eta=1.55, beta_m=0.3, beta_n=0.3, alpha=2.0):
        f32 = lambda x: float(np.float32(x))
        bm, bn, al = f32(beta_m), f32(beta_n), f32(alpha)
        self.beta_m, self.beta_n, self.alpha = bm, bn, al
        self.eta = np.float64(f32(eta))
        self.sigma_a = np.array([f32(x) for x in sigma_a], np.float64)
        v0 = (0.726 * bm + 0.812 * bm ** 2 + 3.7 * bm ** 20) ** 2
        self.v = np.array([v0, 0.25 * v0, 4.0 * v0, 4.0 * v0])
        self.s = np.float64(math.sqrt(math.pi / 8.0) * (0.265 * bn + 1.194 * bn ** 2 + 5.372 * bn ** 22))
        sk = [math.sin(math.radians(al))]
        ck = [math.sqrt(max(0.0, 1.0 - sk[0] ** 2))]
        for i in (1, 2):
            sk.append(2.0 * ck[i - 1] * sk[i - 1])
            ck.append(ck[i - 1] ** 2 - sk[i - 1] ** 2)
        self.sin2k, self.cos2k = np.array(sk), np.array(ck)

    def as32(self):
        """every constant rounded to float32, as the device holds it; the arithmetic follows in float32"""
        m = HairModel.__new__(HairModel)
        m.__dict__.update(self.__dict__)
        for k in ("sigma_a", "v", "sin2k", "cos2k"):
            setattr(m, k, getattr(self, k).astype(np.float32))
        m.eta, m.s = np.float32(self.eta), np.float32(self.s)
        return m

    def tables(self):
        """the 15 constants in PbrtHairTables' order, rounded to float32"""
        return np.concatenate([self.sigma_a, [self.eta], self.v, [self.s], self.sin2k, self.cos2k]).astype(np.float32)


def safe_sqrt(x):
    return np.sqrt(np.maximum(x, 0))


def safe_asin(x):
    return np.arcsin(np.clip(x, -1, 1))


def fr_dielectric(cos_i, eta_i, eta_t):
    """the project's fr_dielectric for eta_i = 1 outside (cos_i >= 0 here: a product of two non-negative cosines)"""
    cos_i = np.clip(cos_i, -1, 1)
    sin_i = safe_sqrt(1 - cos_i * cos_i)
    sin_t = eta_i / eta_t * sin_i
    cos_t = safe_sqrt(1 - sin_t * sin_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_parl = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
        r_perp = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
    return np.where(sin_t >= 1, np.ones_like(cos_i), (r_parl * r_parl + r_perp * r_perp) / 2)


I0_TERMS = 20


def i0(x):
    """I0(x) = sum_{i < 20} (x^2 / 4)^i / (i!)^2, nested: 1 + t (1 + t / 4 (1 + t / 9 (...))). pbrt-v3 stops after ten terms, which
    is short by 1.5 % at x = 12, the end of the range it serves; the normalisations decide."""
    t = x * x * 0.25
    val = np.ones_like(x)
    for i in range(I0_TERMS - 1, 0, -1):
        val = 1 + t * (1.0 / (i * i)) * val
    return val


def log_i0(x):
    big = x > 12
    xs = np.where(big, x, 13 * np.ones_like(x))
    # x - log(2 pi x) / 2 + log(1 + 1 / (8 x) + 9 / (128 x^2) + 225 / (3072 x^3)): 5e-6 at x = 12. pbrt-v3 has 1 / (16 x) for the
    # last logarithm, half its first term, and is 0.5 % short there
    r = 1 / xs
    hi = xs + 0.5 * (-math.log(2 * math.pi) + np.log(r)) + np.log(1 + 0.125 * r * (1 + 0.5625 * r * (1 + (25.0 / 24.0) * r)))
    lo = np.log(i0(np.where(big, np.zeros_like(x), x)))
    return np.where(big, hi, lo)


def mp(cos_i, cos_o, sin_i, sin_o, v):
    a = cos_i * cos_o / v
    b = sin_i * sin_o / v
    if float(v) <= 0.1:
        return np.exp(log_i0(a) - b - 1 / v + 0.6931 + np.log(1 / (2 * v)))
    return np.exp(-b) * i0(a) / (np.sinh(1 / v) * 2 * v)


def logistic(x, s):
    e = np.exp(-np.abs(x) / s)
    return e / (s * (1 + e) * (1 + e))


def logistic_cdf(x, s):
    return 1 / (1 + np.exp(-x / s))


def phi_p(p, gamma_o, gamma_t):
    return 2 * p * gamma_t - 2 * gamma_o + p * math.pi


def np_(phi, p, s, gamma_o, gamma_t):
    dphi = phi - phi_p(p, gamma_o, gamma_t)
    for _ in range(4):  # |phi| <= 2 pi, |Phi| <= 2 p pi/2 + pi + p pi: at most four turns
        dphi = np.where(dphi > math.pi, dphi - 2 * math.pi, dphi)
        dphi = np.where(dphi < -math.pi, dphi + 2 * math.pi, dphi)
    return logistic(dphi, s) / (logistic_cdf(math.pi, s) - logistic_cdf(-math.pi, s))


def y_value(c):
    return 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]


class _Geom:
    pass


def _geometry(m, h, wo):
    """what f, pdf and sample_f share: the angles of wo, the refracted gamma_t and the attenuations ap[0..3] (n, 3)"""
    g = _Geom()
    g.sin_o = wo[:, 0]
    g.cos_o = safe_sqrt(1 - g.sin_o * g.sin_o)
    g.phi_o = np.arctan2(wo[:, 2], wo[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        sin_t = g.sin_o / m.eta
        cos_t = safe_sqrt(1 - sin_t * sin_t)
        etap = np.sqrt(m.eta * m.eta - g.sin_o * g.sin_o) / g.cos_o
        sin_gt = h / etap
        cos_gt = safe_sqrt(1 - sin_gt * sin_gt)
        g.gamma_t = safe_asin(sin_gt)
        g.gamma_o = safe_asin(h)
        T = np.exp(-m.sigma_a[None, :] * (2 * cos_gt / cos_t)[:, None])
        cos_go = safe_sqrt(1 - h * h)
        F = fr_dielectric(g.cos_o * cos_go, 1.0, m.eta)[:, None]
        ap0 = F * np.ones_like(T)
        ap1 = (1 - F) * (1 - F) * T
        ap2 = ap1 * T * F
        den = 1 - T * F
        # 1 - T F == 0 only where F == 1 and T == 1 (h = +-1 or grazing wo, no absorption): ap[2] is 0 there and so is the residual (D111)
        ap3 = np.where(den == 0, np.zeros_like(T), ap2 * F * T / np.where(den == 0, np.ones_like(den), den))
    g.ap = [ap0, ap1, ap2, ap3]
    return g


def _tilt(m, p, sin_o, cos_o, absolute=True):
    if p == 0:
        s = sin_o * m.cos2k[1] - cos_o * m.sin2k[1]
        c = cos_o * m.cos2k[1] + sin_o * m.sin2k[1]
    elif p == 1:
        s = sin_o * m.cos2k[0] + cos_o * m.sin2k[0]
        c = cos_o * m.cos2k[0] - sin_o * m.sin2k[0]
    else:
        s = sin_o * m.cos2k[2] + cos_o * m.sin2k[2]
        c = cos_o * m.cos2k[2] - sin_o * m.sin2k[2]
    return s, (np.abs(c) if absolute else c)


def ap_pdf(g):
    ys = [y_value(a) for a in g.ap]
    tot = ys[0] + ys[1] + ys[2] + ys[3]
    return [y / tot for y in ys]


def _lobe_sum(m, g, weights, sin_i, cos_i, phi):
    """sum over p of Mp * weights[p] * Np, plus the residual; weights[p] is (n,) or (n, 3)"""
    def w(k, x):
        return weights[k] * (x[:, None] if weights[k].ndim == 2 else x)
    total = 0
    for p in range(P_MAX):
        sin_op, cos_op = _tilt(m, p, g.sin_o, g.cos_o)
        total = total + w(p, mp(cos_i, cos_op, sin_i, sin_op, m.v[p]) * np_(phi, p, m.s, g.gamma_o, g.gamma_t))
    return total + w(3, mp(cos_i, g.cos_o, sin_i, g.sin_o, m.v[3]) / (2 * math.pi))


def hair_f(m, h, wo, wi, g=None):
    """HairBSDF::f, (n, 3)"""
    g = g or _geometry(m, h, wo)
    sin_i = wi[:, 0]
    cos_i = safe_sqrt(1 - sin_i * sin_i)
    phi = np.arctan2(wi[:, 2], wi[:, 1]) - g.phi_o
    f = _lobe_sum(m, g, g.ap, sin_i, cos_i, phi)
    az = np.abs(wi[:, 2])
    return np.where((az > 0)[:, None], f / np.where(az > 0, az, np.ones_like(az))[:, None], f)


def hair_pdf(m, h, wo, wi, g=None):
    """HairBSDF::Pdf, (n,)"""
    g = g or _geometry(m, h, wo)
    sin_i = wi[:, 0]
    cos_i = safe_sqrt(1 - sin_i * sin_i)
    phi = np.arctan2(wi[:, 2], wi[:, 1]) - g.phi_o
    return _lobe_sum(m, g, ap_pdf(g), sin_i, cos_i, phi)


def demux(u):
    """DemuxFloat: the even and the odd bits of uint64(u 2^32), each over 2^16"""
    bits = (np.asarray(u, np.float64) * 4294967296.0).astype(np.uint64)

    def compact(x):
        x = x & np.uint64(0x55555555)
        x = (x ^ (x >> np.uint64(1))) & np.uint64(0x33333333)
        x = (x ^ (x >> np.uint64(2))) & np.uint64(0x0F0F0F0F)
        x = (x ^ (x >> np.uint64(4))) & np.uint64(0x00FF00FF)
        x = (x ^ (x >> np.uint64(8))) & np.uint64(0x0000FFFF)
        return x
    return compact(bits).astype(np.float64) / 65536.0, compact(bits >> np.uint64(1)).astype(np.float64) / 65536.0


def hair_sample_f(m, h, wo, u):
    """HairBSDF::Sample_f: (wi, f, pdf, p)"""
    dt = wo.dtype
    g = _geometry(m, h, wo)
    u00, u01 = (x.astype(dt) for x in demux(u[:, 0]))
    u10, u11 = (x.astype(dt) for x in demux(u[:, 1]))
    apq = ap_pdf(g)
    p = np.zeros(len(wo), np.int64)
    rest = u00.copy()
    open_ = np.ones(len(wo), bool)
    for k in range(P_MAX):
        take = open_ & (rest < apq[k])
        p[take] = k
        open_ &= ~take
        rest = np.where(open_, rest - apq[k], rest)
    p[open_] = P_MAX
    sin_op, cos_op, vp = g.sin_o.copy(), g.cos_o.copy(), np.full(len(wo), m.v[3], dt)
    for k in range(P_MAX):
        s_k, c_k = _tilt(m, k, g.sin_o, g.cos_o, absolute=False)
        sin_op, cos_op, vp = np.where(p == k, s_k, sin_op), np.where(p == k, c_k, cos_op), np.where(p == k, m.v[k], vp)
    u10 = np.maximum(u10, 1e-5)
    cos_t = 1 + vp * np.log(u10 + (1 - u10) * np.exp(-2 / vp))
    sin_t = safe_sqrt(1 - cos_t * cos_t)
    sin_i = -cos_t * sin_op + sin_t * np.cos(2 * math.pi * u11) * cos_op
    cos_i = safe_sqrt(1 - sin_i * sin_i)
    # sample_trimmed_logistic(u01, s, -pi, pi)
    k_ = logistic_cdf(math.pi, m.s) - logistic_cdf(-math.pi, m.s)
    with np.errstate(divide="ignore"):
        x = -m.s * np.log(1 / (u01 * k_ + logistic_cdf(-math.pi, m.s)) - 1)
    x = np.clip(x, -math.pi, math.pi)
    dphi = np.where(p < P_MAX, phi_p(p.astype(dt), g.gamma_o, g.gamma_t) + x, 2 * math.pi * u01)
    phi_i = g.phi_o + dphi
    wi = np.stack([sin_i, cos_i * np.cos(phi_i), cos_i * np.sin(phi_i)], axis=1)
    pdf = _lobe_sum(m, g, apq, sin_i, cos_i, dphi)
    return wi, hair_f(m, h, wo, wi, g), pdf, p


# ---- inside BSDF::f / pdf / sample_f (reflection.rs:264-446) as the only lobe ----
def bsdf_f(m, h, wo, wi):
    return np.where((wo[:, 2] == 0)[:, None], 0, hair_f(m, h, wo, wi))


def bsdf_pdf(m, h, wo, wi):
    return np.where(wo[:, 2] == 0, 0, hair_pdf(m, h, wo, wi))


def bsdf_sample_f(m, h, wo, u):
    """(wi, f, pdf, ok, p): u[0] remapped for one component; nothing sampled at wo.z == 0 or pdf == 0"""
    u = np.stack([np.minimum(u[:, 0], ONE_MINUS_EPSILON), u[:, 1]], axis=1)
    wi, f, pdf, p = hair_sample_f(m, h, wo, u)
    ok = (wo[:, 2] != 0) & (pdf > 0)
    return np.where(ok[:, None], wi, 0), np.where(ok[:, None], f, 0), np.where(ok, pdf, 0), ok, p
