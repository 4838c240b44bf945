"""float64 numpy restatement of pbrt-v3's DisneyMaterial without subsurface as pbrt_hip_scene_set_disney_material defines it
(DESIGN.md "Disney", D73-D78): DisneyDiffuse, DisneyFakeSS, DisneyRetro, DisneySheen, MicrofacetReflection with the separable
masking and the Disney Fresnel term, DisneyClearcoat (GTR1) with its sampler, MicrofacetTransmission and LambertianTransmission,
and BSDF::f / pdf / sample_f over up to eight lobes with the sampled lobe's BxDFType. Written from the formulas of DESIGN.md;
Trowbridge-Reitz's Lambda and visible-normal sampler come from microfacet_model.py, MicrofacetTransmission's half vector, pdf
and sampler and the quadrature nodes from bxdf_model.py. Directions are in the shading frame (n = ng = +z), arrays of shape (n, 3).

As in bxdf_model.py every function computes in the dtype of the directions it is given, so the same text on float32 arrays is
the 'float32 restatement' the GPU test measures its tolerances with."""
from types import SimpleNamespace

import numpy as np

import bxdf_model as bm
import microfacet_model as mm

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY = bm.REFLECTION, bm.TRANSMISSION, bm.DIFFUSE, bm.GLOSSY
LOBES = ("diffuse", "fakess", "retro", "sheen", "micro", "clearcoat", "trans", "lambert_t")  # the order DisneyMaterial adds them
FLAGS = {"diffuse": REFLECTION | DIFFUSE, "fakess": REFLECTION | DIFFUSE, "retro": REFLECTION | DIFFUSE, "sheen": REFLECTION | DIFFUSE,
         "micro": REFLECTION | GLOSSY, "clearcoat": REFLECTION | GLOSSY, "trans": TRANSMISSION | GLOSSY, "lambert_t": TRANSMISSION | DIFFUSE}
COSINE = ("diffuse", "fakess", "retro", "sheen")  # the BxDF trait's cosine-hemisphere sampler and pdf
SCALARS = ("metallic", "eta", "roughness", "specular_tint", "anisotropic", "sheen", "sheen_tint", "clearcoat", "clearcoat_gloss", "spec_trans",
           "flatness", "diff_trans")
_COLOURS = ("c_diffuse", "c_fakess", "c_retro", "c_sheen", "cspec0", "c_trans", "c_lambert_t")
_FLOATS = ("metallic", "eta", "roughness", "ax", "ay", "tax", "tay", "clearcoat", "a2")


def lerp(t, a, b):
    return (1 - t) * a + t * b


class Disney:
    """the per-row constants of a descriptor (scenes.disney's dict), from its float32 fields, in float64"""

    def __init__(self, desc):
        d = {k: float(np.float32(desc[k])) for k in SCALARS}
        c = np.asarray(desc["color"], np.float32).astype(np.float64)
        self.thin = bool(desc["thin"])
        lum = float(np.dot([0.212671, 0.715160, 0.072169], c))
        tint = c / lum if lum > 0 else np.ones(3)
        dw = (1 - d["metallic"]) * (1 - d["spec_trans"])
        dt = d["diff_trans"] / 2
        aspect = np.sqrt(1 - 0.9 * d["anisotropic"])
        r = d["roughness"]
        self.metallic, self.eta, self.roughness = d["metallic"], d["eta"], r
        self.ax, self.ay = max(1e-3, r * r / aspect), max(1e-3, r * r * aspect)
        r0 = ((self.eta - 1) / (self.eta + 1)) ** 2
        self.cspec0 = lerp(self.metallic, r0 * lerp(d["specular_tint"], 1.0, tint), c)
        z = np.zeros(3)
        self.c_diffuse = self.c_fakess = self.c_retro = self.c_sheen = self.c_trans = self.c_lambert_t = z
        lobes = []
        if dw > 0:
            if self.thin:
                self.c_diffuse = dw * (1 - d["flatness"]) * (1 - dt) * c
                self.c_fakess = dw * d["flatness"] * (1 - dt) * c
                lobes += ["diffuse", "fakess"]
            else:
                self.c_diffuse = dw * c
                lobes += ["diffuse"]
            self.c_retro = dw * c
            lobes += ["retro"]
            if d["sheen"] > 0:
                self.c_sheen = dw * d["sheen"] * lerp(d["sheen_tint"], 1.0, tint)
                lobes += ["sheen"]
        lobes += ["micro"]
        self.clearcoat = d["clearcoat"]
        self.a2 = lerp(d["clearcoat_gloss"], 0.1, 0.001) ** 2  # the clearcoat's g^2
        if self.clearcoat > 0:
            lobes += ["clearcoat"]
        self.tax, self.tay, self.sep_trans = self.ax, self.ay, not self.thin
        if d["spec_trans"] > 0:
            self.c_trans = d["spec_trans"] * np.sqrt(c)
            if self.thin:
                rs = (0.65 * self.eta - 0.35) * r
                self.tax, self.tay = max(1e-3, rs * rs / aspect), max(1e-3, rs * rs * aspect)
            lobes += ["trans"]
        if self.thin:
            self.c_lambert_t = dt * c
            lobes += ["lambert_t"]
        self.lobes = lobes
        self.n = len(lobes)

    def as32(self):
        """the same BSDF with its constants rounded to float32, as the device holds them"""
        b = object.__new__(Disney)
        b.__dict__.update(self.__dict__)
        for k in _COLOURS:
            setattr(b, k, getattr(self, k).astype(np.float32).astype(np.float64))
        for k in _FLOATS:
            setattr(b, k, float(np.float32(getattr(self, k))))
        return b

    def trans_shim(self):
        """the transmission lobe as bxdf_model reads a rough-glass model: half vector, pdf, sampler, quadrature cuts"""
        has = "trans" in self.lobes
        return SimpleNamespace(kind=bm.GLASS if has else bm.OREN, lobes=["trans"] if has else [], eta=self.eta, ax=self.tax, ay=self.tay,
                               pdf_form="taken", ks=self.c_trans)


_dot, _unit = bm._dot, bm._unit


def sw(c):
    """SchlickWeight"""
    m = np.clip(1 - c, 0, 1)
    return (m * m) * (m * m) * m


def _half(wo, wi):
    wh = wo + wi
    nrm = np.linalg.norm(wh, axis=-1)
    return wh / np.where(nrm == 0, 1, nrm)[..., None], nrm != 0


def _c(v, like):
    return v.astype(like.dtype)


def tr_d(wh, ax, ay):
    """Trowbridge-Reitz D as 1 / (pi ax ay (x^2 / ax^2 + y^2 / ay^2 + z^2)^2): the form without 1 - cos^2 (the device's, D77)"""
    T = wh.dtype.type
    s = (wh[..., 0] / T(ax)) ** 2 + (wh[..., 1] / T(ay)) ** 2 + wh[..., 2] ** 2
    return 1 / (T(np.pi) * T(ax) * T(ay) * s * s)


def tr_pdf(wo, wh, ax, ay):
    return tr_d(wh, ax, ay) * mm.tr_g1(wo, ax, ay) * np.abs(_dot(wo, wh)) / np.abs(wo[..., 2])


# ---- the lobes ----
def diffuse_f(m, wo, wi):
    T = wo.dtype.type
    fo, fi = sw(np.abs(wo[..., 2])), sw(np.abs(wi[..., 2]))
    return _c(m.c_diffuse, wo) * (T(1 / np.pi) * (1 - fo / 2) * (1 - fi / 2))[..., None]


def fakess_f(m, wo, wi):
    T = wo.dtype.type
    wh, ok = _half(wo, wi)
    cd = _dot(wi, wh)
    co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
    fss90 = cd * cd * T(m.roughness)
    fss = lerp(sw(co), T(1), fss90) * lerp(sw(ci), T(1), fss90)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = T(1 / np.pi) * T(1.25) * (fss * (1 / (co + ci) - T(0.5)) + T(0.5))
    return np.where(ok[..., None], _c(m.c_fakess, wo) * v[..., None], 0).astype(wo.dtype)


def retro_f(m, wo, wi):
    T = wo.dtype.type
    wh, ok = _half(wo, wi)
    cd = _dot(wi, wh)
    fo, fi = sw(np.abs(wo[..., 2])), sw(np.abs(wi[..., 2]))
    rr = 2 * T(m.roughness) * cd * cd
    v = T(1 / np.pi) * rr * (fo + fi + fo * fi * (rr - 1))
    return np.where(ok[..., None], _c(m.c_retro, wo) * v[..., None], 0).astype(wo.dtype)


def sheen_f(m, wo, wi):
    wh, ok = _half(wo, wi)
    return np.where(ok[..., None], _c(m.c_sheen, wo) * sw(_dot(wi, wh))[..., None], 0).astype(wo.dtype)


def disney_fresnel(m, c):
    """lerp(metallic, FrDielectric(c, 1, eta), FrSchlick(Cspec0, c)), (n, 3)"""
    T = c.dtype.type
    fd = bm.fr_dielectric(c, 1.0, m.eta)
    s = sw(c)[..., None]
    schlick = (1 - s) * _c(m.cspec0, c) + s
    return (1 - T(m.metallic)) * fd[..., None] + T(m.metallic) * schlick


def micro_f(m, wo, wi):
    co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
    wh, ok = _half(wo, wi)
    ok = ok & (co != 0) & (ci != 0)
    whf = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    F = disney_fresnel(m, _dot(wi, whf))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = tr_d(wh, m.ax, m.ay) * mm.tr_g1(wo, m.ax, m.ay) * mm.tr_g1(wi, m.ax, m.ay) / (4 * ci * co)
    return np.where(ok[..., None], F * v[..., None], 0).astype(wo.dtype)


def micro_pdf(m, wo, wi):
    same = wo[..., 2] * wi[..., 2] > 0
    wh = _unit(wo + wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = tr_pdf(wo, wh, m.ax, m.ay) / (4 * _dot(wo, wh))
    return np.where(same, p, 0).astype(wo.dtype)


def gtr1(m, wh):
    """GTR1(|cos theta_h|, g) with the denominator 1 + (g^2 - 1) cos^2 as sin^2 + g^2 cos^2"""
    T = wh.dtype.type
    norm = (m.a2 - 1) / (np.pi * np.log(m.a2))
    return T(norm) / (wh[..., 0] ** 2 + wh[..., 1] ** 2 + T(m.a2) * wh[..., 2] ** 2)


def smith_g(c, a=0.25):
    T = c.dtype.type
    a2 = T(a * a)
    return 1 / (c + np.sqrt(a2 + c * c - a2 * c * c))


def clearcoat_f(m, wo, wi):
    T = wo.dtype.type
    wh, ok = _half(wo, wi)
    s = sw(_dot(wo, wh))
    fr = (1 - s) * T(0.04) + s
    v = T(m.clearcoat) * smith_g(np.abs(wo[..., 2])) * smith_g(np.abs(wi[..., 2])) * fr * gtr1(m, wh) / 4
    return np.where(ok[..., None], np.repeat(v[..., None], 3, -1), 0).astype(wo.dtype)


def clearcoat_pdf(m, wo, wi):
    same = wo[..., 2] * wi[..., 2] > 0
    wh, ok = _half(wo, wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = gtr1(m, wh) * np.abs(wh[..., 2]) / (4 * _dot(wo, wh))
    return np.where(same & ok, p, 0).astype(wo.dtype)


def trans_f(m, wo, wi):
    """MicrofacetTransmission::f (bxdf_model.trans_f, D70-D72) with G = G1(wo) G1(wi) when not thin"""
    T = wo.dtype.type
    s = m.trans_shim()
    co, ci = wo[..., 2], wi[..., 2]
    wh, ow, iw, eta = bm.trans_parts(s, wo, wi)
    ok = ~(co * ci > 0) & (co != 0) & (ci != 0) & ~(ow * iw > 0) & bm._front(s, wo, wi, ow, iw)
    F = bm.fr_dielectric(ow, 1.0, m.eta)
    sd = ow + eta * iw
    factor = 1 / eta
    g = mm.tr_g1(wo, m.tax, m.tay) * mm.tr_g1(wi, m.tax, m.tay) if m.sep_trans else mm.tr_g(wo, wi, m.tax, m.tay)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.abs(tr_d(wh, m.tax, m.tay) * g * eta * eta * np.abs(iw) * np.abs(ow) * factor * factor / (ci * co * sd * sd))
        v = (T(1) - F) * v
    return np.where(ok[..., None], _c(m.c_trans, wo) * v[..., None], 0).astype(wo.dtype)


def trans_pdf(m, wo, wi):
    s = m.trans_shim()
    wh, ow, iw, eta = bm.trans_parts(s, wo, wi)
    ok = ~(wo[..., 2] * wi[..., 2] > 0) & ~(ow * iw > 0) & bm._front(s, wo, wi, ow, iw)
    sd = ow + eta * iw
    with np.errstate(divide="ignore", invalid="ignore"):
        p = tr_pdf(wo, wh, m.tax, m.tay) * np.abs(eta * eta * iw / (sd * sd))
    return np.where(ok, p, 0).astype(wo.dtype)


def lambert_t_f(m, wo, wi):
    T = wo.dtype.type
    return np.broadcast_to(_c(m.c_lambert_t, wo) * T(1 / np.pi), wo.shape).astype(wo.dtype)


def lambert_t_pdf(wo, wi):
    return np.where(wo[..., 2] * wi[..., 2] > 0, 0, np.abs(wi[..., 2]) * wo.dtype.type(1 / np.pi)).astype(wo.dtype)


_F = {"diffuse": diffuse_f, "fakess": fakess_f, "retro": retro_f, "sheen": sheen_f, "micro": micro_f, "clearcoat": clearcoat_f,
      "trans": trans_f, "lambert_t": lambert_t_f}
_PDF = {"micro": micro_pdf, "clearcoat": clearcoat_pdf, "trans": trans_pdf, "lambert_t": lambda m, wo, wi: lambert_t_pdf(wo, wi)}
_PDF.update({k: (lambda m, wo, wi: bm.cos_pdf(wo, wi)) for k in COSINE})


# ---- BSDF::f / pdf / sample_f ----
def lobe_f(m, lobe, wo, wi):
    return _F[lobe](m, wo, wi)


def bsdf_f(m, wo, wi):
    """reflection lobes where wi and wo are on the same side of ng = +z, transmission lobes otherwise"""
    reflect = (wi[..., 2] * wo[..., 2] > 0)[..., None]
    f = np.zeros(wo.shape[:-1] + (3,), wo.dtype)
    for lobe in m.lobes:
        transmissive = (FLAGS[lobe] & TRANSMISSION) != 0
        f = f + np.where(reflect != transmissive, _F[lobe](m, wo, wi), 0).astype(wo.dtype)
    return np.where((wo[..., 2] == 0)[..., None], 0, f).astype(wo.dtype)


def bsdf_pdf(m, wo, wi):
    p = np.zeros(wo.shape[:-1], wo.dtype)
    for lobe in m.lobes:
        p = p + _PDF[lobe](m, wo, wi)
    return np.where(wo[..., 2] == 0, 0, p / m.n).astype(wo.dtype)


def clearcoat_sample_wh(m, wo, u0, u1):
    """cos theta_h = sqrt(max(0, (1 - (g^2)^(1 - u0)) / (1 - g^2))), phi = 2 pi u1, wh flipped into wo's hemisphere"""
    cos_t = np.sqrt(np.maximum(0, (1 - m.a2 ** (1 - u0)) / (1 - m.a2)))
    sin_t = np.sqrt(np.maximum(0, 1 - cos_t * cos_t))
    phi = 2 * np.pi * u1
    wh = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], -1)
    return np.where((wo[:, 2] < 0)[:, None], -wh, wh)


def _sample_lobe(m, lobe, wo, ur, u1, exact_slope):
    """(wi, pdf) of one BxDF::sample_f; pdf 0 = nothing sampled"""
    if lobe in COSINE:
        wi = bm._cosine_hemisphere(wo, ur, u1)
        return wi, bm.cos_pdf(wo, wi)
    if lobe == "lambert_t":
        wi = bm._cosine_hemisphere(-wo, ur, u1)
        return wi, lambert_t_pdf(wo, wi)
    if lobe == "micro":
        wh = bm._sample_wh(wo, m.ax, m.ay, ur, u1, exact_slope)
        ow = _dot(wo, wh)
        wi = -wo + 2 * ow[:, None] * wh
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where((ow >= 0) & (wo[:, 2] * wi[:, 2] > 0), tr_pdf(wo, wh, m.ax, m.ay) / (4 * ow), 0.0)
        return wi, p
    if lobe == "clearcoat":
        wh = clearcoat_sample_wh(m, wo, ur, u1)
        ow = _dot(wo, wh)
        wi = -wo + 2 * ow[:, None] * wh
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(wo[:, 2] * wi[:, 2] > 0, gtr1(m, wh) * np.abs(wh[:, 2]) / (4 * ow), 0.0)
        return wi, p
    # trans: a visible normal of the lobe's own alphas, then refract (bxdf_model._sample_lobe), with this module's pdf
    wi, p = bm._sample_lobe(m.trans_shim(), "trans", wo, ur, u1, exact_slope)
    return wi, np.where(p != 0, trans_pdf(m, wo, wi), 0.0)


def bsdf_sample_f(m, wo, u, exact_slope=False):
    """BSDF::sample_f with BSDF_ALL: (wi, f, pdf, ok, flags, lobe index); u[:, 0] picks the lobe and is remapped. float64 only.
    exact_slope: the visible-normal sampler with the exact slope_y inverse (bxdf_model._sample11_exact) instead of pbrt-v3's fit."""
    n = len(wo)
    wo = wo.astype(np.float64)
    u0, u1 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    flags = np.zeros(n, np.int32)
    comp = np.minimum(np.floor(u0 * m.n), m.n - 1).astype(np.int64)
    ur = np.minimum(u0 * m.n - comp, mm.ONE_MINUS_EPSILON)
    wi, p = np.zeros((n, 3)), np.zeros(n)
    for k, lobe in enumerate(m.lobes):
        pick = comp == k
        if not pick.any():
            continue
        wk, pk = _sample_lobe(m, lobe, wo[pick], ur[pick], u1[pick], exact_slope)
        wi[pick], p[pick] = wk, pk
        flags[pick] = FLAGS[lobe]
    ok = (p > 0) & np.isfinite(p) & (wo[:, 2] != 0)
    wi = np.where(ok[:, None], wi, np.array([0.0, 0.0, 1.0]))
    pdf = np.where(ok, bsdf_pdf(m, wo, wi) if m.n > 1 else p, 0.0)
    f = np.where(ok[:, None], bsdf_f(m, wo, wi), 0.0)
    return np.where(ok[:, None], wi, 0.0), f, pdf, ok, np.where(ok, flags, 0), comp


# ---- quadrature over the whole sphere (bxdf_model's nodes: cut at wo's polar angle and where the transmission pdf jumps) ----
def albedo_parts(m, wo, n_theta=128, n_phi=512):
    """integral of f(wo, wi) |cos theta_i|: the part from wo's own side of the surface and the part from across it"""
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = bm._sphere_nodes(m.trans_shim(), wo, n_theta, n_phi)
    g = bsdf_f(m, np.broadcast_to(wo, wi.shape), wi) * (np.abs(wi[:, 2]) * w)[:, None]
    same = wi[:, 2] * wo[2] > 0
    return np.sum(g[same], 0), np.sum(g[~same], 0)


def albedo(m, wo, n_theta=128, n_phi=512):
    a, b = albedo_parts(m, wo, n_theta, n_phi)
    return a + b


def pdf_integral(m, wo, n_theta=128, n_phi=512):
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = bm._sphere_nodes(m.trans_shim(), wo, n_theta, n_phi)
    return float(np.sum(bsdf_pdf(m, np.broadcast_to(wo, wi.shape), wi) * w))


def _pdf_bins_on(m, wo, c_edges, p_edges, xs, wxs):
    n_cos, n_phi, sub = len(c_edges) - 1, len(p_edges) - 1, len(xs)
    c = 0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * xs + 0.5 * (c_edges[1:] + c_edges[:-1])[:, None]
    wc = 0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * wxs
    p = 0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * xs + 0.5 * (p_edges[1:] + p_edges[:-1])[:, None]
    wp = 0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * wxs
    C = np.broadcast_to(c[:, None, :, None], (n_cos, n_phi, sub, sub))
    P = np.broadcast_to(p[None, :, None, :], (n_cos, n_phi, sub, sub))
    W = wc[:, None, :, None] * wp[None, :, None, :]
    wi = mm.sphere_dir(C.reshape(-1), P.reshape(-1))
    v = bsdf_pdf(m, np.broadcast_to(np.asarray(wo, np.float64).reshape(1, 3), wi.shape), wi).reshape(n_cos, n_phi, sub, sub)
    return np.sum(v * W, axis=(2, 3))


def pdf_bins(m, wo, n_cos=16, n_phi=32, sub=16):
    """integral of BSDF::pdf(wo, .) over the (cos theta, phi) bins of microfacet_model.bin_of. Rows of bins are integrated in
    pieces where the pdf is not smooth: at the horizon's neighbours nothing, at the transmission pdf's jump (bxdf_model._jump_cos)
    and at the mirror direction's cos theta, where the clearcoat and the reflection lobe peak."""
    xs, wxs = np.polynomial.legendre.leggauss(sub)
    wo = np.asarray(wo, np.float64).reshape(3)
    c_edges = np.linspace(-1, 1, n_cos + 1)
    p_edges = np.linspace(0, 2 * np.pi, n_phi + 1)
    out = _pdf_bins_on(m, wo, c_edges, p_edges, xs, wxs)
    cuts = [c for c in (bm._jump_cos(m.trans_shim(), wo), float(wo[2])) if c is not None and np.min(np.abs(c_edges - c)) > 1e-9]
    for c_star in cuts:
        k = int(np.searchsorted(c_edges, c_star)) - 1
        total = 0
        for a, b in ((c_edges[k], c_star), (c_star, c_edges[k + 1])):
            e = c_edges.copy()
            e[k], e[k + 1] = a, b
            total = total + _pdf_bins_on(m, wo, e, p_edges, xs, wxs)[k]
        out[k] = total
    return out


def chi2_p(m, wo, wi_s, ok, n):
    """bxdf_model.chi2_p's construction on this module's pdf: (p, chi2, bins, samples where the pdf has no mass)"""
    from scipy import stats
    expected = pdf_bins(m, wo).reshape(-1) * n
    counts = np.bincount(mm.bin_of(wi_s[ok].astype(np.float64)), minlength=expected.size)
    exp = np.append(expected, max(n - expected.sum(), 0.0))
    obs = np.append(counts, n - ok.sum())
    small = exp < 5
    e = np.append(exp[~small], exp[small].sum())
    o = np.append(obs[~small], obs[small].sum())
    keep = e > 0
    chi2 = np.sum((o[keep] - e[keep]) ** 2 / e[keep])
    return float(stats.chi2.sf(chi2, keep.sum() - 1)), float(chi2), int(keep.sum()), int(o[~keep].sum())
