"""float64 numpy model of the general lobe-list BSDF (reflection.rs:207-449) and of pbrt-v3's UberMaterial, TranslucentMaterial
and MixMaterial on it: a list of up to 8 lobes of any kind, each with the BxDFType the reference gives it,
ScaledBxDF, and BSDF::num_components / f / pdf / sample_f under a flag mask. The lobes themselves are the ones
microfacet_model.py, bxdf_model.py and disney_model.py already hold; what is written here is the list, the flag matching, the
two perfect-specular lobes and LambertianTransmission's sampler. Directions are in the shading frame (n = ng = +z), arrays of
shape (n, 3). f and pdf compute in the dtype of the directions they are given (the float32 restatement); sample_f is float64."""
from types import SimpleNamespace

import numpy as np

import bxdf_model as bm
import disney_model as dm
import microfacet_model as mm

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY, SPECULAR = 1, 2, 4, 8, 16  # BxDFType
ALL = 31
NON_SPECULAR = ALL & ~SPECULAR
# PbrtLobeKind
LAMBERT_R, LAMBERT_T, OREN, SPEC_R, SPEC_T, MICRO_R, MICRO_T, BLEND = range(1, 9)
TYPE = {LAMBERT_R: REFLECTION | DIFFUSE, LAMBERT_T: TRANSMISSION | DIFFUSE, OREN: REFLECTION | DIFFUSE, SPEC_R: REFLECTION | SPECULAR,
        SPEC_T: TRANSMISSION | SPECULAR, MICRO_R: REFLECTION | GLOSSY, MICRO_T: TRANSMISSION | GLOSSY, BLEND: REFLECTION | GLOSSY}
NOOP, DIELECTRIC, CONDUCTOR = 0, 1, 2  # PbrtLobeFresnel
_COLOURS = ("scale", "r", "s", "eta", "k")
_FLOATS = ("ax", "ay", "eta_i", "eta_t", "A", "B")


class Lobe:
    def __init__(self, kind, r, fresnel=NOOP, scale=(1, 1, 1), s=(0, 0, 0), ax=0.0, ay=0.0, eta_i=1.0, eta_t=1.0, eta=(0, 0, 0), k=(0, 0, 0),
                 A=0.0, B=0.0):
        self.kind, self.type, self.fresnel = kind, TYPE[kind], fresnel
        for name, v in zip(_COLOURS, (scale, r, s, eta, k)):
            setattr(self, name, np.asarray(v, np.float64).reshape(3).copy())
        self.ax, self.ay, self.eta_i, self.eta_t, self.A, self.B = (float(v) for v in (ax, ay, eta_i, eta_t, A, B))

    def copy(self):
        return Lobe(self.kind, self.r, self.fresnel, self.scale, self.s, self.ax, self.ay, self.eta_i, self.eta_t, self.eta, self.k,
                    self.A, self.B)

    def literal(self):
        """(kind, fresnel, scale, r) as plain tuples, for tests that state a list literally"""
        return (self.kind, self.fresnel, tuple(float(v) for v in self.scale), tuple(float(v) for v in self.r))


class Bsdf:
    """lobes in the order the material adds them (sample_f picks by index among the matching ones) and BSDF::eta"""

    def __init__(self, lobes, eta=1.0):
        assert len(lobes) <= 8
        self.lobes = list(lobes)
        self.eta = float(eta)
        self.n = len(self.lobes)

    def trans_shim(self):
        """the (first) MicrofacetTransmission lobe as bxdf_model reads a rough-glass model: half vector, grazing band, quadrature cuts"""
        t = [l for l in self.lobes if l.kind == MICRO_T]
        if not t:
            return SimpleNamespace(kind=bm.OREN, lobes=[], eta=1.0)
        return SimpleNamespace(kind=bm.GLASS, lobes=["trans"], eta=t[0].eta_t, ax=t[0].ax, ay=t[0].ay, pdf_form="taken", ks=t[0].r)

    def as32(self):
        """the same BSDF with its parameters rounded to float32, as the device holds them"""
        out = []
        for l in self.lobes:
            c = l.copy()
            for name in _COLOURS:
                setattr(c, name, getattr(l, name).astype(np.float32).astype(np.float64))
            for name in _FLOATS:
                setattr(c, name, float(np.float32(getattr(l, name))))
            out.append(c)
        return Bsdf(out, float(np.float32(self.eta)))


def num_components(m, flags=ALL):
    return sum(1 for l in m.lobes if (l.type & flags) == l.type)


# ---- the materials' list rules. Colours are clamped to [0, 1] and multiplied in float32, in pbrt-v3's order ----
def _rgb(c):
    return np.full(3, c, np.float32) if np.isscalar(c) else np.asarray(c, np.float32).reshape(3)


def _clamp(c):
    return np.clip(_rgb(c), np.float32(0), np.float32(1))


def _black(c):
    return not np.any(c != 0)


def _alpha(r, remap):
    """the descriptor's roughness is a float32; roughness_to_alpha runs in double on that value"""
    r = float(np.float32(r))
    return mm.roughness_to_alpha(r) if remap else r


def uber(kd=0.25, ks=0.25, kr=0.0, kt=0.0, opacity=1.0, eta=1.5, u_roughness=0.1, v_roughness=0.1, remap=True):
    op = _clamp(opacity)
    t = np.clip(-op + np.float32(1), np.float32(0), np.float32(1))
    lobes = []
    if not _black(t):
        lobes.append(Lobe(SPEC_T, t, DIELECTRIC, eta_i=1.0, eta_t=1.0))
    c = op * _clamp(kd)
    if not _black(c):
        lobes.append(Lobe(LAMBERT_R, c))
    c = op * _clamp(ks)
    if not _black(c):
        lobes.append(Lobe(MICRO_R, c, DIELECTRIC, ax=_alpha(u_roughness, remap), ay=_alpha(v_roughness, remap), eta_i=1.0, eta_t=eta))
    c = op * _clamp(kr)
    if not _black(c):
        lobes.append(Lobe(SPEC_R, c, DIELECTRIC, eta_i=1.0, eta_t=eta))
    c = op * _clamp(kt)
    if not _black(c):
        lobes.append(Lobe(SPEC_T, c, DIELECTRIC, eta_i=1.0, eta_t=eta))
    return Bsdf(lobes, 1.0 if not _black(t) else eta)


def translucent(kd=0.25, ks=0.25, reflect=0.5, transmit=0.5, roughness=0.1, remap=True):
    r, t, kd, ks = _clamp(reflect), _clamp(transmit), _clamp(kd), _clamp(ks)
    lobes = []
    if not (_black(r) and _black(t)):
        if not _black(kd):
            if not _black(r):
                lobes.append(Lobe(LAMBERT_R, r * kd))
            if not _black(t):
                lobes.append(Lobe(LAMBERT_T, t * kd))
        if not _black(ks):
            a = _alpha(roughness, remap)
            if not _black(r):
                lobes.append(Lobe(MICRO_R, r * ks, DIELECTRIC, ax=a, ay=a, eta_i=1.0, eta_t=1.5))
            if not _black(t):
                lobes.append(Lobe(MICRO_T, t * ks, DIELECTRIC, ax=a, ay=a, eta_i=1.0, eta_t=1.5))
    return Bsdf(lobes, 1.5)


def mix(a, b, amount=0.5):
    """a's lobes under ScaledBxDF(s1), then b's under ScaledBxDF(s2); a black scale is kept; eta is a's"""
    s1 = _clamp(amount)
    s2 = np.clip(np.float32(1) - s1, np.float32(0), np.float32(1))
    lobes = []
    for src, s in ((a, s1), (b, s2)):
        for l in src.lobes:
            c = l.copy()
            c.scale = (s * l.scale.astype(np.float32)).astype(np.float64)
            lobes.append(c)
    assert len(lobes) <= 8
    return Bsdf(lobes, a.eta)


# the rows of levels 0-2 as lists (what a mix reads of its operands)
def matte(kd):
    kd = _rgb(kd)
    return Bsdf([] if _black(kd) else [Lobe(LAMBERT_R, kd)])


def mirror(kr):
    kr = _rgb(kr)
    return Bsdf([] if _black(kr) else [Lobe(SPEC_R, kr, NOOP)])


def plastic(kd, ks, roughness, remap=True):
    kd, ks = _rgb(kd), _rgb(ks)
    a = _alpha(roughness, remap)
    return Bsdf(([] if _black(kd) else [Lobe(LAMBERT_R, kd)]) +
                ([] if _black(ks) else [Lobe(MICRO_R, ks, DIELECTRIC, ax=a, ay=a, eta_i=1.5, eta_t=1.0)]))


def metal(eta, k, u_roughness, v_roughness=None, remap=True):
    v_roughness = u_roughness if v_roughness is None else v_roughness
    return Bsdf([Lobe(MICRO_R, (1, 1, 1), CONDUCTOR, ax=_alpha(u_roughness, remap), ay=_alpha(v_roughness, remap), eta=_rgb(eta), k=_rgb(k))])


def from_bxdf_model(b):
    """bxdf_model.Bsdf (matte with sigma, rough glass, substrate) as a list"""
    if b.kind == bm.OREN:
        return Bsdf([Lobe(OREN, b.kd, A=b.A, B=b.B)] if b.n else [])
    if b.kind == bm.GLASS:
        return Bsdf(([Lobe(MICRO_R, b.kd, DIELECTRIC, ax=b.ax, ay=b.ay, eta_i=1.0, eta_t=b.eta)] if "refl" in b.lobes else []) +
                    ([Lobe(MICRO_T, b.ks, DIELECTRIC, ax=b.ax, ay=b.ay, eta_i=1.0, eta_t=b.eta)] if "trans" in b.lobes else []), b.eta)
    return Bsdf([Lobe(BLEND, b.kd, s=b.ks, ax=b.ax, ay=b.ay)] if b.n else [])


# ---- one lobe: f, pdf, sample (before ScaledBxDF) ----
def _shim(l):
    """the lobe as bxdf_model's functions read a Bsdf (kd / ks are what each of them calls its colour)"""
    return SimpleNamespace(kd=l.r, ks=l.s if l.kind == BLEND else l.r, eta=l.eta_t, ax=l.ax, ay=l.ay, A=l.A, B=l.B, pdf_form="taken")


def _micro_r_f(l, wo, wi):
    """MicrofacetReflection::f with FresnelDielectric(eta_i, eta_t): bxdf_model.refl_f, whose Fresnel is (1, eta), with the pair"""
    co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
    wh = wo + wi
    nrm = np.linalg.norm(wh, axis=-1)
    ok = (co != 0) & (ci != 0) & (nrm != 0)
    wh = wh / np.where(nrm == 0, 1, nrm)[..., None]
    whf = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    F = bm.fr_dielectric(bm._dot(wi, whf), l.eta_i, l.eta_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = mm.tr_d(wh, l.ax, l.ay) * mm.tr_g(wo, wi, l.ax, l.ay) * F / (4 * ci * co)
    return np.where(ok[..., None], l.r.astype(wo.dtype) * v[..., None], 0).astype(wo.dtype)


def lobe_f(l, wo, wi):
    T = wo.dtype.type
    zero = np.zeros(wo.shape[:-1] + (3,), wo.dtype)
    if l.kind in (LAMBERT_R, LAMBERT_T):
        return zero + l.r.astype(wo.dtype) * T(1 / np.pi)
    if l.kind == OREN:
        return bm.oren_f(_shim(l), wo, wi)
    if l.kind == MICRO_R:
        if l.fresnel == CONDUCTOR:
            return mm.microfacet_f(SimpleNamespace(metal=True, kd=l.eta, ks=l.k, ax=l.ax, ay=l.ay), wo, wi).astype(wo.dtype)
        return _micro_r_f(l, wo, wi)
    if l.kind == MICRO_T:
        return bm.trans_f(_shim(l), wo, wi)
    if l.kind == BLEND:
        return bm.blend_f(_shim(l), wo, wi)
    return zero  # the specular kinds


def lobe_pdf(l, wo, wi):
    if l.kind in (LAMBERT_R, OREN):
        return bm.cos_pdf(wo, wi)
    if l.kind == LAMBERT_T:
        return dm.lambert_t_pdf(wo, wi).astype(wo.dtype)
    if l.kind == MICRO_R:
        return bm.refl_pdf(_shim(l), wo, wi)
    if l.kind == MICRO_T:
        return bm.trans_pdf(_shim(l), wo, wi)
    if l.kind == BLEND:
        return bm.blend_pdf(_shim(l), wo, wi)
    return np.zeros(wo.shape[:-1], wo.dtype)


def specular_sample(l, wo):
    """(wi, f, pdf) of SpecularReflection / SpecularTransmission::sample_f (reflection.rs:633-654, 691-726; Radiance mode), in the
    dtype of wo"""
    T = wo.dtype.type
    n = len(wo)
    r = l.r.astype(wo.dtype)
    one = np.ones(n, wo.dtype)
    if l.kind == SPEC_R:
        wi = wo * np.array([-1, -1, 1], wo.dtype)
        F = one if l.fresnel == NOOP else bm.fr_dielectric(wi[:, 2], l.eta_i, l.eta_t)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = r * (F / np.abs(wi[:, 2]))[:, None]
        return wi, f.astype(wo.dtype), one
    entering = wo[:, 2] > 0
    ei, et = np.where(entering, T(l.eta_i), T(l.eta_t)), np.where(entering, T(l.eta_t), T(l.eta_i))
    eta = ei / et
    cos_i = np.abs(wo[:, 2])
    sin2_t = eta * eta * np.maximum(T(0), T(1) - cos_i * cos_i)
    tir = sin2_t >= 1
    cos_t = np.sqrt(np.where(tir, T(0), T(1) - sin2_t))
    nz = np.where(entering, T(1), T(-1))
    wi = -wo * eta[:, None]
    wi[:, 2] += nz * (eta * cos_i - cos_t)
    F = bm.fr_dielectric(wi[:, 2], l.eta_i, l.eta_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = r * ((T(1) - F) * (ei * ei) / (et * et) / np.abs(wi[:, 2]))[:, None]
    return wi, np.where(tir[:, None], T(0), f).astype(wo.dtype), np.where(tir, T(0), T(1)).astype(wo.dtype)


def _sample_lobe(l, wo, ur, u1, exact_slope=False):
    """(wi, pdf, f) of one BxDF::sample_f; pdf 0 = nothing sampled; f is meaningful for the specular kinds only"""
    zero3 = np.zeros((len(wo), 3))
    if l.kind in (LAMBERT_R, OREN):
        wi = bm._cosine_hemisphere(wo, ur, u1)
        return wi, bm.cos_pdf(wo, wi), zero3
    if l.kind == LAMBERT_T:
        wi = bm._cosine_hemisphere(wo, ur, u1)
        wi[:, 2] *= -1
        return wi, dm.lambert_t_pdf(wo, wi), zero3
    if l.kind in (SPEC_R, SPEC_T):
        wi, f, p = specular_sample(l, wo)
        return wi, p, f
    lobe = {MICRO_R: "refl", MICRO_T: "trans", BLEND: "blend"}[l.kind]
    wi, p = bm._sample_lobe(_shim(l), lobe, wo, ur, u1, exact_slope)
    return wi, p, zero3


# ---- BSDF::f / pdf / sample_f under a flag mask (reflection.rs:264-448) ----
def _matching(m, flags):
    return [(k, l) for k, l in enumerate(m.lobes) if (l.type & flags) == l.type]


def bsdf_f(m, wo, wi, flags=ALL):
    reflect = wi[..., 2] * wo[..., 2] > 0
    f = np.zeros(wo.shape[:-1] + (3,), wo.dtype)
    for _, l in _matching(m, flags):
        if l.type & SPECULAR:
            continue
        side = reflect if (l.type & REFLECTION) else ~reflect
        f = f + np.where(side[..., None], l.scale.astype(wo.dtype) * lobe_f(l, wo, wi), 0).astype(wo.dtype)
    return np.where((wo[..., 2] == 0)[..., None], 0, f).astype(wo.dtype)


def bsdf_pdf(m, wo, wi, flags=ALL):
    p = np.zeros(wo.shape[:-1], wo.dtype)
    match = _matching(m, flags)
    if not match:
        return p
    for _, l in match:
        p = p + lobe_pdf(l, wo, wi)
    return np.where(wo[..., 2] == 0, 0, p / len(match)).astype(wo.dtype)


def bsdf_sample_f(m, wo, u, flags=ALL, exact_slope=False):
    """(wi, f, pdf, ok, sampled BxDFType, index of the picked lobe in m.lobes); u[:, 0] picks among the MATCHING lobes and is
    remapped. A specular pick returns that lobe's scaled value and pdf / matching alone."""
    n = len(wo)
    wo = wo.astype(np.float64)
    u0, u1 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    zero3 = np.zeros((n, 3))
    match = _matching(m, flags)
    nm = len(match)
    if nm == 0:
        return zero3, zero3, np.zeros(n), np.zeros(n, bool), np.zeros(n, np.int32), np.full(n, -1)
    comp = np.minimum(np.floor(u0 * nm), nm - 1).astype(np.int64)
    ur = np.minimum(u0 * nm - comp, mm.ONE_MINUS_EPSILON)
    wi, p, fs = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3))
    types, index = np.zeros(n, np.int32), np.full(n, -1)
    for j, (k, l) in enumerate(match):
        pick = comp == j
        if not pick.any():
            continue
        wk, pk, fk = _sample_lobe(l, wo, ur, u1, exact_slope)
        wi[pick], p[pick], fs[pick] = wk[pick], pk[pick], (fk * l.scale)[pick]
        types[pick], index[pick] = l.type, k
    ok = (p != 0) & np.isfinite(p) & (wo[:, 2] != 0)
    spec = (types & SPECULAR) != 0
    wi_e = np.where(ok[:, None], wi, np.array([0.0, 0.0, 1.0]))
    pdf = np.where(spec, p / nm, bsdf_pdf(m, wo, wi_e, flags) if nm > 1 else p)
    f = np.where(spec[:, None], fs, bsdf_f(m, wo, wi_e, flags))
    return (np.where(ok[:, None], wi, 0.0), np.where(ok[:, None], f, 0.0), np.where(ok, pdf, 0.0), ok, np.where(ok, types, 0),
            np.where(ok, index, -1))


# ---- quadrature ----
def _nodes(m, wo, n_theta, n_phi):
    """bxdf_model's sphere nodes, split where a MicrofacetTransmission lobe's pdf jumps"""
    return bm._sphere_nodes(m.trans_shim(), wo, n_theta, n_phi)


def albedo(m, wo, n_theta=128, n_phi=512):
    """rho(wo): the quadrature of the non-specular f |cos| over the sphere, plus the specular lobes' weights f |cos| / pdf"""
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = _nodes(m, wo, n_theta, n_phi)
    f = bsdf_f(m, np.broadcast_to(wo, wi.shape), wi, NON_SPECULAR)
    total = np.sum(f * (np.abs(wi[:, 2]) * w)[:, None], 0)
    for l in m.lobes:
        if l.type & SPECULAR:
            ws, fs, ps = specular_sample(l, wo.reshape(1, 3))
            if ps[0] != 0:
                total = total + l.scale * fs[0] * abs(ws[0, 2]) / ps[0]
    return total


def pdf_bins(m, wo, flags=NON_SPECULAR, n_cos=16, n_phi=32, sub=16):
    """integral of BSDF::pdf(wo, ., flags) over microfacet_model.bin_of's (cos theta, phi) bins: Gauss-Legendre, sub x sub nodes per
    bin (bxdf_model.pdf_bins' construction)"""
    xs, wxs = np.polynomial.legendre.leggauss(sub)
    wo = np.asarray(wo, np.float64).reshape(1, 3)
    c_edges, p_edges = np.linspace(-1, 1, n_cos + 1), np.linspace(0, 2 * np.pi, n_phi + 1)
    c = 0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * xs + 0.5 * (c_edges[1:] + c_edges[:-1])[:, None]
    wc = 0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * wxs
    ph = 0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * xs + 0.5 * (p_edges[1:] + p_edges[:-1])[:, None]
    wp = 0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * wxs
    C = np.broadcast_to(c[:, None, :, None], (n_cos, n_phi, sub, sub))
    P = np.broadcast_to(ph[None, :, None, :], (n_cos, n_phi, sub, sub))
    wi = mm.sphere_dir(C.reshape(-1), P.reshape(-1))
    v = bsdf_pdf(m, np.broadcast_to(wo, wi.shape), wi, flags).reshape(n_cos, n_phi, sub, sub)
    return np.sum(v * (wc[:, None, :, None] * wp[None, :, None, :]), axis=(2, 3))
