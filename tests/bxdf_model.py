"""float64 numpy restatement of the BSDFs of matte with sigma > 0, rough glass and substrate (pbrt-v3's MatteMaterial,
GlassMaterial and SubstrateMaterial on the reference's BxDFs): OrenNayar, MicrofacetReflection with
FresnelDielectric(1, eta), MicrofacetTransmission in radiance mode, FresnelBlend, and BSDF::f / pdf / sample_f over those lobes
with the sampled lobe's BxDFType. Written from the formulas; the Trowbridge-Reitz distribution, its visible-normal sampler and
the quadrature nodes come from microfacet_model.py. Directions are in the shading frame (n = ng = +z), arrays of shape (n, 3).

Every function computes in the dtype of the directions it is given, so the same text evaluated on float32 arrays is the
'float32 restatement' the GPU test measures its tolerances with (test_gpu_bxdfs.py); everything else uses float64."""
import numpy as np

import microfacet_model as mm

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY = 1, 2, 4, 8  # BxDFType bits
OREN, GLASS, SUBSTRATE = "oren_nayar", "rough_glass", "substrate"


class Bsdf:
    """kind OREN: kd, A, B. kind GLASS: kr, kt, eta, ax, ay (lobe order: reflection, transmission). kind SUBSTRATE: kd, ks, ax, ay.
    pdf_form: how MicrofacetTransmission is read. 'taken' (the default, what the device computes): pbrt-v3's f and Pdf, 0 for a
    microfacet seen from behind (D72); 'v3': pbrt-v3 as it stands; 'reference': reflection.rs:1185's Jacobian as written (D70)."""

    def __init__(self, kind, kd=(0, 0, 0), ks=(0, 0, 0), eta=1.0, ax=0.0, ay=None, A=1.0, B=0.0, pdf_form="taken"):
        self.kind = kind
        self.kd = np.asarray(kd, np.float64)  # matte / substrate Kd; glass Kr
        self.ks = np.asarray(ks, np.float64)  # substrate Ks; glass Kt
        self.eta = float(eta)
        self.ax = float(ax)
        self.ay = float(ax if ay is None else ay)
        self.A, self.B = float(A), float(B)
        self.pdf_form = pdf_form
        if kind == OREN:
            self.lobes = ["oren"] if np.any(self.kd != 0) else []
        elif kind == GLASS:
            self.lobes = (["refl"] if np.any(self.kd != 0) else []) + (["trans"] if np.any(self.ks != 0) else [])
        else:
            self.lobes = ["blend"] if (np.any(self.kd != 0) or np.any(self.ks != 0)) else []
        self.n = len(self.lobes)

    def as32(self):
        """the same BSDF with its parameters rounded to float32, as the device holds them"""
        f = lambda v: float(np.float32(v))
        b = Bsdf(self.kind, self.kd.astype(np.float32).astype(np.float64), self.ks.astype(np.float32).astype(np.float64), f(self.eta),
                 f(self.ax), f(self.ay), f(self.A), f(self.B), self.pdf_form)
        return b


def _alpha(r, remap):
    return mm.roughness_to_alpha(r) if remap else float(r)


def matte_sigma(kd, sigma):
    """MatteMaterial: sigma in degrees, clamped to [0, 90]; OrenNayar's A and B from sigma in radians (D68)"""
    s = np.radians(min(max(float(sigma), 0.0), 90.0))
    s2 = s * s
    return Bsdf(OREN, kd, A=1.0 - s2 / (2.0 * (s2 + 0.33)), B=0.45 * s2 / (s2 + 0.09))


def rough_glass(kr, kt, eta, u_roughness, v_roughness=None, remap=True, pdf_form="taken"):
    v_roughness = u_roughness if v_roughness is None else v_roughness
    return Bsdf(GLASS, kr, kt, eta, _alpha(u_roughness, remap), _alpha(v_roughness, remap), pdf_form=pdf_form)


def substrate(kd, ks, u_roughness, v_roughness=None, remap=True):
    v_roughness = u_roughness if v_roughness is None else v_roughness
    return Bsdf(SUBSTRATE, kd, ks, 1.0, _alpha(u_roughness, remap), _alpha(v_roughness, remap))


# ---- helpers that keep the dtype of their arguments ----
def _dot(a, b):
    return np.sum(a * b, -1)


def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return v / np.where(n == 0, 1, n)


def _col(m, v, like):
    """a colour of the BSDF in the dtype of `like`"""
    return v.astype(like.dtype)


def fr_dielectric(cos_i, eta_i, eta_t):
    """reflection.rs:15-40; eta_i / eta_t python floats, rounded to cos_i's dtype"""
    T = cos_i.dtype.type
    cos_i = np.clip(cos_i, -1, 1)
    entering = cos_i > 0
    ei = np.where(entering, T(eta_i), T(eta_t))
    et = np.where(entering, T(eta_t), T(eta_i))
    cos_i = np.abs(cos_i)
    sin_t = ei / et * np.sqrt(np.maximum(0, 1 - cos_i * cos_i))
    cos_t = np.sqrt(np.maximum(0, 1 - sin_t * sin_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_parl = (et * cos_i - ei * cos_t) / (et * cos_i + ei * cos_t)
        r_perp = (ei * cos_i - et * cos_t) / (ei * cos_i + et * cos_t)
    return np.where(sin_t >= 1, T(1), (r_parl ** 2 + r_perp ** 2) / 2)


# ---- OrenNayar (reflection.rs:917-975 with pbrt-v3's sigma in radians and cos(phi_i - phi_o)) ----
def oren_f(m, wo, wi):
    T = wo.dtype.type
    si, so = np.sqrt(mm._sin2(wi)), np.sqrt(mm._sin2(wo))
    d_cos = mm._cos_phi(wi) * mm._cos_phi(wo) + mm._sin_phi(wi) * mm._sin_phi(wo)
    max_cos = np.where((si > 1e-4) & (so > 1e-4), np.maximum(d_cos, 0), T(0))
    ci, co = np.abs(wi[..., 2]), np.abs(wo[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        i_steeper = ci > co
        sin_alpha = np.where(i_steeper, so, si)
        tan_beta = np.where(i_steeper, si / ci, so / co)
        v = T(m.A) + T(m.B) * max_cos * sin_alpha * tan_beta
    return _col(m, m.kd, wo) * T(1 / np.pi) * v[..., None]


# ---- MicrofacetReflection with FresnelDielectric(1, eta) (reflection.rs:1000-1051; D63: wi = reflect(wo, wh)) ----
def refl_f(m, wo, wi):
    co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
    wh = wo + wi
    nrm = np.linalg.norm(wh, axis=-1)
    ok = (co != 0) & (ci != 0) & (nrm != 0)
    wh = wh / np.where(nrm == 0, 1, nrm)[..., None]
    whf = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    F = fr_dielectric(_dot(wi, whf), 1.0, m.eta)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = mm.tr_d(wh, m.ax, m.ay) * mm.tr_g(wo, wi, m.ax, m.ay) * F / (4 * ci * co)
    return np.where(ok[..., None], _col(m, m.kd, wo) * v[..., None], 0).astype(wo.dtype)


def refl_pdf(m, wo, wi):
    same = wo[..., 2] * wi[..., 2] > 0
    wh = _unit(wo + wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = mm.tr_pdf(wo, wh, m.ax, m.ay) / (4 * _dot(wo, wh))
    return np.where(same, p, 0).astype(wo.dtype)


# ---- MicrofacetTransmission(T, TR, 1, eta, Radiance) (reflection.rs:1093-1187; pdf: pbrt-v3, D70; back faces: D72) ----
def _front(m, wo, wi, ow, iw):
    """both directions see the front of the microfacet wh (on +z): Walter et al.'s chi+ in G1, which pbrt-v3's G leaves out"""
    if m.pdf_form != "taken":
        return np.ones(ow.shape, bool)
    return (ow * wo[..., 2] > 0) & (iw * wi[..., 2] > 0)


def _trans_eta(m, wo):
    T = wo.dtype.type
    return np.where(wo[..., 2] > 0, T(m.eta) / T(1), T(1) / T(m.eta))


def trans_parts(m, wo, wi):
    """(wh flipped to +z, wo.wh, wi.wh, eta) of the generalised half vector wo + wi eta"""
    eta = _trans_eta(m, wo)
    wh = _unit(wo + wi * eta[..., None])
    wh = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    return wh, _dot(wo, wh), _dot(wi, wh), eta


def trans_f(m, wo, wi):
    T = wo.dtype.type
    co, ci = wo[..., 2], wi[..., 2]
    wh, ow, iw, eta = trans_parts(m, wo, wi)
    ok = ~(co * ci > 0) & (co != 0) & (ci != 0) & ~(ow * iw > 0) & _front(m, wo, wi, ow, iw)
    F = fr_dielectric(ow, 1.0, m.eta)
    sd = ow + eta * iw
    factor = 1 / eta  # TransportMode::Radiance
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.abs(mm.tr_d(wh, m.ax, m.ay) * mm.tr_g(wo, wi, m.ax, m.ay) * eta * eta * np.abs(iw) * np.abs(ow) * factor * factor /
                   (ci * co * sd * sd))
        v = (T(1) - F) * v
    return np.where(ok[..., None], _col(m, m.ks, wo) * v[..., None], 0).astype(wo.dtype)


def trans_pdf(m, wo, wi):
    wh, ow, iw, eta = trans_parts(m, wo, wi)
    ok = ~(wo[..., 2] * wi[..., 2] > 0) & ~(ow * iw > 0) & _front(m, wo, wi, ow, iw)
    sd = ow + eta * iw
    with np.errstate(divide="ignore", invalid="ignore"):
        if m.pdf_form == "reference":  # reflection.rs:1185: (eta^2 wi.wh) / sqrt_denom * sqrt_denom
            dwh_dwi = np.abs(eta * eta * iw / sd * sd)
        else:
            dwh_dwi = np.abs(eta * eta * iw / (sd * sd))
        p = mm.tr_pdf(wo, wh, m.ax, m.ay) * dwh_dwi
    return np.where(ok, p, 0).astype(wo.dtype)


# ---- FresnelBlend (reflection.rs:1194-1280; as pbrt-v3) ----
def _pow5(v):
    return (v * v) * (v * v) * v


def blend_f(m, wo, wi):
    T = wo.dtype.type
    ci, co = np.abs(wi[..., 2]), np.abs(wo[..., 2])
    kd, ks = _col(m, m.kd, wo), _col(m, m.ks, wo)
    diffuse = T(28 / (23 * np.pi)) * kd * (1 - ks) * ((1 - _pow5(1 - T(0.5) * ci)) * (1 - _pow5(1 - T(0.5) * co)))[..., None]
    wh = wi + wo
    nrm = np.linalg.norm(wh, axis=-1)
    wh = wh / np.where(nrm == 0, 1, nrm)[..., None]
    iw = _dot(wi, wh)
    schlick = ks + (1 - ks) * _pow5(1 - iw)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        spec = schlick * (mm.tr_d(wh, m.ax, m.ay) / (4 * np.abs(iw) * np.maximum(ci, co)))[..., None]
    return np.where((nrm == 0)[..., None], 0, diffuse + spec).astype(wo.dtype)


def blend_pdf(m, wo, wi):
    T = wo.dtype.type
    same = wo[..., 2] * wi[..., 2] > 0
    wh = _unit(wo + wi)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = T(0.5) * (np.abs(wi[..., 2]) * T(1 / np.pi) + mm.tr_pdf(wo, wh, m.ax, m.ay) / (4 * _dot(wo, wh)))
    return np.where(same, p, 0).astype(wo.dtype)


def cos_pdf(wo, wi):
    return np.where(wo[..., 2] * wi[..., 2] > 0, np.abs(wi[..., 2]) * wo.dtype.type(1 / np.pi), 0).astype(wo.dtype)


_F = {"oren": oren_f, "refl": refl_f, "trans": trans_f, "blend": blend_f}
_PDF = {"oren": lambda m, wo, wi: cos_pdf(wo, wi), "refl": refl_pdf, "trans": trans_pdf, "blend": blend_pdf}
_TRANSMISSIVE = {"oren": False, "refl": False, "trans": True, "blend": False}
FLAGS = {"oren": REFLECTION | DIFFUSE, "refl": REFLECTION | GLOSSY, "trans": TRANSMISSION | GLOSSY, "blend": REFLECTION | GLOSSY}


# ---- BSDF::f / pdf / sample_f (reflection.rs:264-446) ----
def bsdf_f(m, wo, wi):
    """reflection lobes where wi and wo are on the same side of ng = +z, transmission lobes otherwise"""
    reflect = (wi[..., 2] * wo[..., 2] > 0)[..., None]
    f = np.zeros(wo.shape[:-1] + (3,), wo.dtype)
    for lobe in m.lobes:
        f = f + np.where(reflect != _TRANSMISSIVE[lobe], _F[lobe](m, wo, wi), 0).astype(wo.dtype)
    return np.where((wo[..., 2] == 0)[..., None], 0, f).astype(wo.dtype)


def bsdf_pdf(m, wo, wi):
    p = np.zeros(wo.shape[:-1], wo.dtype)
    if m.n == 0:
        return p
    for lobe in m.lobes:
        p = p + _PDF[lobe](m, wo, wi)
    return np.where(wo[..., 2] == 0, 0, p / m.n).astype(wo.dtype)


def _cosine_hemisphere(wo, u0, u1):
    dx, dy = mm._concentric(u0, u1)
    w = np.stack([dx, dy, np.sqrt(np.maximum(1 - dx * dx - dy * dy, 0))], -1)
    w[:, 2] *= np.where(wo[:, 2] < 0, -1, 1)
    return w


FIT_MAX_SLOPE = 0.00357 / (0.093073 + 0.309420 - 1.0 + 0.597999)  # the rational fit of trowbridge_reitz_sample11 at u = 1: 7.26


_FIT11 = mm._sample11


def slope_tail_mass(s):
    """mass of the slope_y distribution p(s) ~ (1 + s^2)^-2 beyond |s| (the function the rational fit inverts)"""
    return 1 - (2 / np.pi) * (np.arctan(s) + s / (1 + s * s))


def _sample11_exact(cos_theta, u1, u2):
    """microfacet_model._sample11 with slope_y from the exact inverse of its CDF (2 / pi) (t + sin t cos t), s = tan t, by
    bisection, in place of pbrt-v3's / Heitz's rational fit, which stops at |s| = 7.26 and so never returns the 1.1e-3 of the
    normals beyond it"""
    sx, sy_fit = _FIT11(cos_theta, u1, u2)
    normal = cos_theta > 0.9999
    a2 = np.where(u2 > 0.5, 2 * (u2 - 0.5), 2 * (0.5 - u2))
    lo, hi = np.zeros_like(a2), np.full_like(a2, np.pi / 2)
    for _ in range(60):
        t = (lo + hi) / 2
        below = (2 / np.pi) * (t + np.sin(t) * np.cos(t)) < a2
        lo, hi = np.where(below, t, lo), np.where(below, hi, t)
    sy = np.where(u2 > 0.5, 1.0, -1.0) * np.tan((lo + hi) / 2) * np.sqrt(1 + sx * sx)
    return sx, np.where(normal, sy_fit, sy)


def _sample_wh(wo, ax, ay, u0, u1, exact_slope):
    if not exact_slope:
        return mm.tr_sample_wh(wo, ax, ay, u0, u1)
    # TrowbridgeReitzDistribution::sample_wh around the exact slopes: stretch, sample, rotate, unstretch (D64), normal
    flip = wo[..., 2] < 0
    w = np.where(flip[..., None], -wo, wo)
    ws = _unit(np.stack([ax * w[..., 0], ay * w[..., 1], w[..., 2]], -1))
    sx, sy = _sample11_exact(ws[..., 2], u0, u1)
    cp, sp = mm._cos_phi(ws), mm._sin_phi(ws)
    sx, sy = cp * sx - sp * sy, sp * sx + cp * sy
    wh = _unit(np.stack([-ax * sx, -ay * sy, np.ones_like(sx)], -1))
    return np.where(flip[..., None], -wh, wh)


def _sample_lobe(m, lobe, wo, ur, u1, exact_slope=False):
    """(wi, pdf) of one BxDF::sample_f; pdf 0 = nothing sampled"""
    n = len(wo)
    if lobe == "oren":
        wi = _cosine_hemisphere(wo, ur, u1)
        return wi, cos_pdf(wo, wi)
    if lobe == "blend":
        first = ur < 0.5
        ua = np.minimum(2 * ur, mm.ONE_MINUS_EPSILON)
        ub = np.minimum(2 * (ur - 0.5), mm.ONE_MINUS_EPSILON)
        wl = _cosine_hemisphere(wo, np.where(first, ua, 0.25), u1)
        wh = _sample_wh(wo, m.ax, m.ay, np.where(first, 0.25, ub), u1, exact_slope)
        wm = -wo + 2 * _dot(wo, wh)[:, None] * wh
        wi = np.where(first[:, None], wl, wm)
        p = np.where(first | (wo[:, 2] * wm[:, 2] > 0), blend_pdf(m, wo, wi), 0.0)
        return wi, p
    wh = _sample_wh(wo, m.ax, m.ay, ur, u1, exact_slope)
    ow = _dot(wo, wh)
    if lobe == "refl":
        wi = -wo + 2 * ow[:, None] * wh
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where((ow >= 0) & (wo[:, 2] * wi[:, 2] > 0), mm.tr_pdf(wo, wh, m.ax, m.ay) / (4 * ow), 0.0)
        return wi, p
    # trans: refract(wo, wh, eta_i / eta_t) (reflection.rs:130-144)
    eta = np.where(wo[:, 2] > 0, 1.0 / m.eta, m.eta)
    sin2_i = np.maximum(0, 1 - ow * ow)
    sin2_t = eta * eta * sin2_i
    tir = sin2_t >= 1
    cos_t = np.sqrt(np.where(tir, 0, 1 - sin2_t))
    wi = -wo * eta[:, None] + wh * (eta * ow - cos_t)[:, None]
    p = np.where((ow >= 0) & ~tir, trans_pdf(m, wo, np.where(tir[:, None], -wo, wi)), 0.0)
    return wi, p


def bsdf_sample_f(m, wo, u, exact_slope=False):
    """BSDF::sample_f with BSDF_ALL: (wi, f, pdf, ok, flags); u[:, 0] picks the lobe and is remapped. float64 only.
    exact_slope: the visible-normal sampler with the exact slope_y inverse (_sample11_exact) instead of pbrt-v3's fit."""
    n = len(wo)
    wo = wo.astype(np.float64)
    u0, u1 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    zero3, flags = np.zeros((n, 3)), np.zeros(n, np.int32)
    if m.n == 0:
        return zero3, zero3, np.zeros(n), np.zeros(n, bool), flags
    comp = np.minimum(np.floor(u0 * m.n), m.n - 1).astype(np.int64)
    ur = np.minimum(u0 * m.n - comp, mm.ONE_MINUS_EPSILON)
    wi, p = np.zeros((n, 3)), np.zeros(n)
    for k, lobe in enumerate(m.lobes):
        wk, pk = _sample_lobe(m, lobe, wo, ur, u1, exact_slope)
        pick = comp == k
        wi[pick], p[pick] = wk[pick], pk[pick]
        flags[pick] = FLAGS[lobe]
    ok = (p != 0) & np.isfinite(p) & (wo[:, 2] != 0)
    wi = np.where(ok[:, None], wi, np.array([0.0, 0.0, 1.0]))
    pdf = np.where(ok, bsdf_pdf(m, wo, wi) if m.n > 1 else p, 0.0)
    f = np.where(ok[:, None], bsdf_f(m, wo, wi), 0.0)
    return np.where(ok[:, None], wi, 0.0), f, pdf, ok, np.where(ok, flags, 0)


# ---- quadrature over the whole sphere ----
def _jump_cos(m, wo):
    """cos theta_i at which the transmission pdf and f jump to 0: the generalised half vector wo + eta wi crosses the horizon
    there, where D(wh) is alpha^2 / pi, not 0. None without a transmission lobe."""
    if m.kind != GLASS or "trans" not in m.lobes or wo[2] == 0:
        return None
    c = -wo[2] / (m.eta if wo[2] > 0 else 1 / m.eta)
    return c if -1 < c < 1 else None


def _sphere_nodes(m, wo, n_theta, n_phi):
    """nodes and weights (d omega) over the sphere: per hemisphere Gauss-Legendre in theta, the interval split at wo's own
    polar angle (OrenNayar's branch on |cos theta_i| > |cos theta_o| has a kink there) and at _jump_cos, and the periodic
    midpoint rule in phi"""
    t_o = np.arccos(min(abs(float(wo[2])), 1.0))
    c_star = _jump_cos(m, wo)
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    dirs, wts = [], []
    for sign in (1.0, -1.0):
        cuts = [0.0, t_o, np.pi / 2]
        if c_star is not None and c_star * sign > 0:
            cuts.append(float(np.arccos(abs(c_star))))
        cuts = sorted(cuts)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b - a < 1e-12:
                continue
            t, wt = mm.gauss_legendre(n_theta, a, b)
            Tm, Pm = np.meshgrid(t, phi, indexing="ij")
            d = np.stack([np.sin(Tm) * np.cos(Pm), np.sin(Tm) * np.sin(Pm), sign * np.cos(Tm)], -1).reshape(-1, 3)
            dirs.append(d)
            wts.append((np.outer(wt * np.sin(t), np.full(n_phi, 2 * np.pi / n_phi))).reshape(-1))
    return np.concatenate(dirs), np.concatenate(wts)


def albedo(m, wo, n_theta=128, n_phi=512):
    """rho(wo) = integral of f(wo, wi) |cos theta_i| over the whole sphere of wi (both hemispheres: rough glass transmits)"""
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = _sphere_nodes(m, wo, n_theta, n_phi)
    f = bsdf_f(m, np.broadcast_to(wo, wi.shape), wi)
    return np.sum(f * (np.abs(wi[:, 2]) * w)[:, None], 0)


def albedo_parts(m, wo, n_theta=128, n_phi=512):
    """albedo split into the part from wo's own side of the surface and the part from across it"""
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = _sphere_nodes(m, wo, n_theta, n_phi)
    g = bsdf_f(m, np.broadcast_to(wo, wi.shape), wi) * (np.abs(wi[:, 2]) * w)[:, None]
    same = wi[:, 2] * wo[2] > 0
    return np.sum(g[same], 0), np.sum(g[~same], 0)


def pdf_integral(m, wo, n_theta=128, n_phi=512):
    wo = np.asarray(wo, np.float64).reshape(3)
    wi, w = _sphere_nodes(m, wo, n_theta, n_phi)
    return float(np.sum(bsdf_pdf(m, np.broadcast_to(wo, wi.shape), wi) * w))


def pdf_bins(m, wo, n_cos=16, n_phi=32, sub=16):
    """integral of BSDF::pdf(wo, .) over the (cos theta, phi) bins of microfacet_model.bin_of: Gauss-Legendre, sub x sub nodes per bin"""
    xs, wxs = np.polynomial.legendre.leggauss(sub)
    wo = np.asarray(wo, np.float64).reshape(3)
    c_edges = np.linspace(-1, 1, n_cos + 1)
    p_edges = np.linspace(0, 2 * np.pi, n_phi + 1)
    if m.kind == GLASS and "trans" in m.lobes:
        # the transmission pdf jumps to 0 where the generalised half vector wo + eta wi crosses the horizon (D(wh) is alpha^2 / pi
        # there, not 0): cos theta_i = -wo.z / eta. The row of bins that holds it is integrated in two pieces.
        c_star = _jump_cos(m, wo)
        if c_star is not None and np.min(np.abs(c_edges - c_star)) > 1e-9:
            k = int(np.searchsorted(c_edges, c_star)) - 1
            parts = []
            for a, b in ((c_edges[k], c_star), (c_star, c_edges[k + 1])):
                e = c_edges.copy()
                e[k], e[k + 1] = a, b
                parts.append(_pdf_bins_on(m, wo, e, p_edges, xs, wxs)[k])
            out = _pdf_bins_on(m, wo, c_edges, p_edges, xs, wxs)
            out[k] = parts[0] + parts[1]
            return out
    return _pdf_bins_on(m, wo, c_edges, p_edges, xs, wxs)


def _pdf_bins_on(m, wo, c_edges, p_edges, xs, wxs):
    n_cos, n_phi, sub = len(c_edges) - 1, len(p_edges) - 1, len(xs)
    c = (0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * xs + 0.5 * (c_edges[1:] + c_edges[:-1])[:, None])  # (n_cos, sub)
    wc = 0.5 * (c_edges[1:] - c_edges[:-1])[:, None] * wxs
    p = (0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * xs + 0.5 * (p_edges[1:] + p_edges[:-1])[:, None])  # (n_phi, sub)
    wp = 0.5 * (p_edges[1:] - p_edges[:-1])[:, None] * wxs
    C = np.broadcast_to(c[:, None, :, None], (n_cos, n_phi, sub, sub))
    P = np.broadcast_to(p[None, :, None, :], (n_cos, n_phi, sub, sub))
    W = wc[:, None, :, None] * wp[None, :, None, :]
    wi = mm.sphere_dir(C.reshape(-1), P.reshape(-1))
    wo = np.asarray(wo, np.float64).reshape(1, 3)
    v = bsdf_pdf(m, np.broadcast_to(wo, wi.shape), wi).reshape(n_cos, n_phi, sub, sub)
    return np.sum(v * W, axis=(2, 3))


def chi2_p(m, wo, wi_s, ok, n):
    """Pearson chi^2 of sampled directions against pdf_bins, the 'nothing sampled' bin last, bins expecting fewer than 5 pooled
    (test_gpu_glossy.py::test_sampler_chi2's construction). Returns (p, chi2, bins, samples where the pdf has no mass)."""
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
