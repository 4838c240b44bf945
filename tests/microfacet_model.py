"""float64 numpy restatement of the plastic / metal BSDFs (pbrt-v3's PlasticMaterial and MetalMaterial on the reference's
BxDFs): Trowbridge-Reitz D / Lambda / G1 / G, the visible-normal sampler step for step, fr_conductor,
fr_dielectric, LambertianReflection, MicrofacetReflection, BSDF::f / pdf / sample_f over the lobes, and the directional albedo
by quadrature. Directions are in the shading frame (n = +z), arrays of shape (n, 3). The GPU tests pin the device to it."""
import numpy as np

ONE_MINUS_EPSILON = float(np.float32(1.0) - np.float32(np.finfo(np.float32).eps))  # the device's kOneMinusEpsilon
MAT_MATTE, MAT_PLASTIC, MAT_METAL = 1, 4, 5


def roughness_to_alpha(r):
    x = np.log(max(float(r), 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x ** 3 + 0.000640711 * x ** 4


# ---- frame trigonometry ----
def _cos2(w):
    return w[..., 2] ** 2


def _sin2(w):
    return np.maximum(0.0, 1.0 - _cos2(w))


def _cos_phi(w):
    st = np.sqrt(_sin2(w))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(st == 0, 1.0, np.clip(w[..., 0] / np.where(st == 0, 1, st), -1, 1))


def _sin_phi(w):
    st = np.sqrt(_sin2(w))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(st == 0, 0.0, np.clip(w[..., 1] / np.where(st == 0, 1, st), -1, 1))


# ---- Trowbridge-Reitz ----
def tr_d(wh, ax, ay):
    with np.errstate(divide="ignore", invalid="ignore"):
        tan2 = _sin2(wh) / _cos2(wh)
        e = (_cos_phi(wh) ** 2 / (ax * ax) + _sin_phi(wh) ** 2 / (ay * ay)) * tan2
        d = 1.0 / (np.pi * ax * ay * _cos2(wh) ** 2 * (1 + e) ** 2)
    return np.where(np.isinf(tan2), 0.0, d)


def tr_lambda(w, ax, ay):
    with np.errstate(divide="ignore", invalid="ignore"):
        abs_tan = np.abs(np.sqrt(_sin2(w)) / w[..., 2])
        alpha = np.sqrt(_cos_phi(w) ** 2 * ax * ax + _sin_phi(w) ** 2 * ay * ay)
        lam = (-1 + np.sqrt(1 + (alpha * abs_tan) ** 2)) / 2
    return np.where(np.isinf(abs_tan), 0.0, lam)


def tr_g1(w, ax, ay):
    return 1 / (1 + tr_lambda(w, ax, ay))


def tr_g(wo, wi, ax, ay):
    return 1 / (1 + tr_lambda(wo, ax, ay) + tr_lambda(wi, ax, ay))


def tr_pdf(wo, wh, ax, ay):
    """visible-normal pdf of wh: D G1(wo) |wo.wh| / |cos theta_o|"""
    return tr_d(wh, ax, ay) * tr_g1(wo, ax, ay) * np.abs(np.sum(wo * wh, -1)) / np.abs(wo[..., 2])


def _sample11(cos_theta, u1, u2):
    """trowbridge_reitz_sample11 with pbrt-v3's discriminant (D65), elementwise"""
    sx = np.empty_like(cos_theta)
    sy = np.empty_like(cos_theta)
    normal = cos_theta > 0.9999
    r = np.sqrt(u1 / (1 - u1))
    phi = 6.28318530718 * u2
    sx[normal], sy[normal] = (r * np.cos(phi))[normal], (r * np.sin(phi))[normal]
    m = ~normal
    c, a1, a2 = cos_theta[m], u1[m], u2[m].copy()
    sin_t = np.sqrt(np.maximum(0.0, 1 - c * c))
    tan_t = sin_t / c
    a = 1 / tan_t
    g1 = 2 / (1 + np.sqrt(1 + 1 / (a * a)))
    A = 2 * a1 / g1 - 1
    with np.errstate(divide="ignore"):
        tmp = 1 / (A * A - 1)
    tmp = np.minimum(tmp, 1e10)
    B = tan_t
    D = np.sqrt(np.maximum(B * B * tmp * tmp - (A * A - B * B) * tmp, 0))
    x1, x2 = B * tmp - D, B * tmp + D
    x = np.where((A < 0) | (x2 > 1 / tan_t), x1, x2)
    S = np.where(a2 > 0.5, 1.0, -1.0)
    a2 = np.where(a2 > 0.5, 2 * (a2 - 0.5), 2 * (0.5 - a2))
    z = (a2 * (a2 * (a2 * 0.27385 - 0.73369) + 0.46341)) / (a2 * (a2 * (a2 * 0.093073 + 0.309420) - 1.0) + 0.597999)
    sx[m], sy[m] = x, S * z * np.sqrt(1 + x * x)
    return sx, sy


def tr_sample_wh(wo, ax, ay, u0, u1):
    """TrowbridgeReitzDistribution::sample_wh, visible-area branch (D64: alpha times the slope)"""
    flip = wo[..., 2] < 0
    w = np.where(flip[..., None], -wo, wo)
    ws = np.stack([ax * w[..., 0], ay * w[..., 1], w[..., 2]], -1)
    ws /= np.linalg.norm(ws, axis=-1, keepdims=True)
    sx, sy = _sample11(ws[..., 2], u0, u1)
    cp, sp = _cos_phi(ws), _sin_phi(ws)
    sx, sy = cp * sx - sp * sy, sp * sx + cp * sy
    wh = np.stack([-ax * sx, -ay * sy, np.ones_like(sx)], -1)
    wh /= np.linalg.norm(wh, axis=-1, keepdims=True)
    return np.where(flip[..., None], -wh, wh)


# ---- Fresnel ----
def fr_dielectric(cos_i, eta_i, eta_t):
    cos_i = np.clip(cos_i, -1, 1)
    entering = cos_i > 0
    ei = np.where(entering, eta_i, eta_t)
    et = np.where(entering, eta_t, eta_i)
    cos_i = np.abs(cos_i)
    sin_t = ei / et * np.sqrt(np.maximum(0, 1 - cos_i * cos_i))
    cos_t = np.sqrt(np.maximum(0, 1 - sin_t * sin_t))
    r_parl = (et * cos_i - ei * cos_t) / (et * cos_i + ei * cos_t)
    r_perp = (ei * cos_i - et * cos_t) / (ei * cos_i + et * cos_t)
    return np.where(sin_t >= 1, 1.0, (r_parl ** 2 + r_perp ** 2) / 2)


def fr_conductor(cos_i, eta, k):
    """reflection.rs:42-67 with eta_i = 1; cos_i (n,), eta / k (3,) -> (n, 3)"""
    c = np.clip(cos_i, -1, 1)[..., None]
    eta, k = np.asarray(eta, np.float64), np.asarray(k, np.float64)
    c2 = c * c
    s2 = 1 - c2
    t0 = eta * eta - k * k - s2
    a2b2 = np.sqrt(t0 * t0 + 4 * eta * eta * k * k)
    t1 = a2b2 + c2
    a = np.sqrt(np.maximum((a2b2 + t0) * 0.5, 0))
    t2 = 2 * c * a
    rs = (t1 - t2) / (t1 + t2)
    t3 = a2b2 * c2 + s2 * s2
    t4 = t2 * s2
    rp = rs * (t3 - t4) / (t3 + t4)
    return (rp + rs) / 2


# ---- the materials' lobes ----
class Material:
    """type MAT_MATTE / MAT_PLASTIC / MAT_METAL; kd, ks: plastic Kd / Ks (matte Kd); metal eta = kd, k = ks; alphas ax, ay"""

    def __init__(self, type, kd, ks=(0, 0, 0), ax=0.0, ay=None):
        self.type = type
        self.kd = np.asarray(kd, np.float64)
        self.ks = np.asarray(ks, np.float64)
        self.ax = float(ax)
        self.ay = float(ax if ay is None else ay)
        self.metal = type == MAT_METAL
        self.lambert = type in (MAT_MATTE, MAT_PLASTIC) and np.any(self.kd != 0)
        self.micro = self.metal or (type == MAT_PLASTIC and np.any(self.ks != 0))
        self.n = int(self.lambert) + int(self.micro)

    @staticmethod
    def plastic(kd, ks, roughness, remap=True):
        a = roughness_to_alpha(roughness) if remap else roughness
        return Material(MAT_PLASTIC, kd, ks, a)

    @staticmethod
    def metal(eta, k, u_roughness, v_roughness=None, remap=True):
        v_roughness = u_roughness if v_roughness is None else v_roughness
        f = roughness_to_alpha if remap else float
        return Material(MAT_METAL, eta, k, f(u_roughness), f(v_roughness))


def microfacet_f(m, wo, wi):
    co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
    wh = wo + wi
    nrm = np.linalg.norm(wh, axis=-1)
    ok = (co != 0) & (ci != 0) & (nrm != 0)
    wh = wh / np.where(nrm == 0, 1, nrm)[..., None]
    whf = np.where((wh[..., 2] < 0)[..., None], -wh, wh)
    c = np.sum(wi * whf, -1)
    if m.metal:
        F, R = fr_conductor(np.abs(c), m.kd, m.ks), np.ones(3)
    else:
        F, R = fr_dielectric(c, 1.5, 1.0)[..., None], m.ks
    with np.errstate(divide="ignore", invalid="ignore"):
        v = R * (tr_d(wh, m.ax, m.ay) * tr_g(wo, wi, m.ax, m.ay))[..., None] * F / (4 * ci * co)[..., None]
    return np.where(ok[..., None], v, 0.0)


def microfacet_pdf(m, wo, wi):
    same = wo[..., 2] * wi[..., 2] > 0
    wh = wo + wi
    nrm = np.linalg.norm(wh, axis=-1)
    wh = wh / np.where(nrm == 0, 1, nrm)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = tr_pdf(wo, wh, m.ax, m.ay) / (4 * np.sum(wo * wh, -1))
    return np.where(same, p, 0.0)


def lambert_pdf(wo, wi):
    return np.where(wo[..., 2] * wi[..., 2] > 0, np.abs(wi[..., 2]) / np.pi, 0.0)


def bsdf_f(m, wo, wi):
    """BSDF::f: the lobes that pass the reflect test on ng = +z"""
    reflect = (wi[..., 2] * wo[..., 2] > 0)[..., None]
    f = np.zeros(wo.shape[:-1] + (3,))
    if m.lambert:
        f = f + np.where(reflect, m.kd / np.pi, 0.0)
    if m.micro:
        f = f + np.where(reflect, microfacet_f(m, wo, wi), 0.0)
    return np.where((wo[..., 2] == 0)[..., None], 0.0, f)


def bsdf_pdf(m, wo, wi):
    """BSDF::pdf: the lobes' average"""
    if m.n == 0:
        return np.zeros(wo.shape[:-1])
    p = np.zeros(wo.shape[:-1])
    if m.lambert:
        p = p + lambert_pdf(wo, wi)
    if m.micro:
        p = p + microfacet_pdf(m, wo, wi)
    return np.where(wo[..., 2] == 0, 0.0, p / m.n)


def _concentric(u0, u1):
    ox, oy = 2 * u0 - 1, 2 * u1 - 1
    zero = (ox == 0) & (oy == 0)
    big = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(big, ox, oy)
        theta = np.where(big, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
    dx, dy = r * np.cos(theta), r * np.sin(theta)
    return np.where(zero, 0.0, dx), np.where(zero, 0.0, dy)


def bsdf_sample_f(m, wo, u):
    """BSDF::sample_f: (wi, f, pdf, ok, glossy) with u (n, 2) picking the lobe in u[:, 0] (D63: wi = reflect(wo, wh))"""
    n = len(wo)
    u0, u1 = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    wi = np.zeros((n, 3))
    pdf = np.zeros(n)
    if m.n == 0:
        return wi, np.zeros((n, 3)), pdf, np.zeros(n, bool), np.zeros(n, bool)
    comp = np.minimum(np.floor(u0 * m.n), m.n - 1)
    use_micro = np.full(n, m.micro) & ~(m.lambert & (comp == 0))
    ur = np.minimum(u0 * m.n - comp, ONE_MINUS_EPSILON)
    # LambertianReflection
    dx, dy = _concentric(ur, u1)
    wl = np.stack([dx, dy, np.sqrt(np.maximum(1 - dx * dx - dy * dy, 0))], -1)
    wl[:, 2] *= np.where(wo[:, 2] < 0, -1, 1)
    # MicrofacetReflection
    if m.micro:
        wh = tr_sample_wh(wo, m.ax, m.ay, ur, u1)
        wo_wh = np.sum(wo * wh, -1)
        wm = -wo + 2 * wo_wh[:, None] * wh
        with np.errstate(divide="ignore", invalid="ignore"):
            pm = np.where((wo_wh >= 0) & (wo[:, 2] * wm[:, 2] > 0), tr_pdf(wo, wh, m.ax, m.ay) / (4 * wo_wh), 0.0)
    else:
        wm, pm = wl, np.zeros(n)
    wi = np.where(use_micro[:, None], wm, wl)
    pdf = np.where(use_micro, pm, lambert_pdf(wo, wl))
    ok = (pdf != 0) & (wo[:, 2] != 0)
    pdf = np.where(ok, bsdf_pdf(m, wo, wi) if m.n > 1 else pdf, 0.0)
    f = np.where(ok[:, None], bsdf_f(m, wo, wi), 0.0)
    return np.where(ok[:, None], wi, 0.0), f, pdf, ok, use_micro & ok


# ---- quadrature ----
def gauss_legendre(n, a, b):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def albedo(m, wo, n_u=256, n_phi=256):
    """rho(wo) = integral of f(wo, wi) |cos theta_i| over the upper hemisphere (wo.z > 0), per RGB channel: the Lambertian
    lobe exactly (Kd), the microfacet lobe over the half vector with tan^2 theta_h = alpha^2 x / (1 - x), where D cos theta_h
    d omega_h = dx dphi / 2 pi (isotropic alpha)"""
    wo = np.asarray(wo, np.float64).reshape(3)
    rho = np.zeros(3)
    if m.lambert:
        rho += m.kd
    if m.micro:
        assert m.ax == m.ay, "the quadrature is written for an isotropic alpha"
        x, wx = gauss_legendre(n_u, 0.0, 1.0)
        phi, wp = gauss_legendre(n_phi, 0.0, 2 * np.pi)
        X, P = np.meshgrid(x, phi, indexing="ij")
        W = np.outer(wx, wp) / (2 * np.pi)
        t2 = m.ax * m.ax * X / (1 - X)
        ct = 1 / np.sqrt(1 + t2)
        st = np.sqrt(np.maximum(0, 1 - ct * ct))
        wh = np.stack([st * np.cos(P), st * np.sin(P), ct], -1).reshape(-1, 3)
        wo_b = np.broadcast_to(wo, wh.shape)
        d = np.sum(wo_b * wh, -1)
        wi = -wo_b + 2 * d[:, None] * wh
        ok = (wi[:, 2] > 0) & (d > 0)
        f = microfacet_f(m, wo_b, wi)
        # f |cos_i| d omega_i, d omega_i = 4 (wo.wh) d omega_h, d omega_h = dx dphi / (2 pi D cos theta_h)
        with np.errstate(divide="ignore", invalid="ignore"):
            jac = np.abs(wi[:, 2]) * 4 * d / (tr_d(wh, m.ax, m.ay) * wh[:, 2])
        g = np.where(ok[:, None], f * jac[:, None], 0.0)
        rho += np.sum(g * W.reshape(-1)[:, None], 0)
    return rho


def sphere_dir(cos_theta, phi):
    st = np.sqrt(np.maximum(0, 1 - cos_theta ** 2))
    return np.stack([st * np.cos(phi), st * np.sin(phi), cos_theta], -1)


def pdf_bins(m, wo, n_cos=16, n_phi=32, sub=16):
    """integral of BSDF::pdf(wo, .) over the (cos theta, phi) bins of the whole sphere (n_cos x n_phi), Gauss-Legendre with
    sub x sub nodes per bin; d omega = d cos theta d phi"""
    xs, wxs = np.polynomial.legendre.leggauss(sub)
    out = np.zeros((n_cos, n_phi))
    c_edges = np.linspace(-1, 1, n_cos + 1)
    p_edges = np.linspace(0, 2 * np.pi, n_phi + 1)
    wo = np.asarray(wo, np.float64).reshape(1, 3)
    for i in range(n_cos):
        c = 0.5 * (c_edges[i + 1] - c_edges[i]) * xs + 0.5 * (c_edges[i + 1] + c_edges[i])
        wc = 0.5 * (c_edges[i + 1] - c_edges[i]) * wxs
        for j in range(n_phi):
            p = 0.5 * (p_edges[j + 1] - p_edges[j]) * xs + 0.5 * (p_edges[j + 1] + p_edges[j])
            wp = 0.5 * (p_edges[j + 1] - p_edges[j]) * wxs
            C, P = np.meshgrid(c, p, indexing="ij")
            wi = sphere_dir(C, P).reshape(-1, 3)
            v = bsdf_pdf(m, np.broadcast_to(wo, wi.shape), wi)
            out[i, j] = np.sum(v * np.outer(wc, wp).reshape(-1))
    return out


def bin_of(wi, n_cos=16, n_phi=32):
    c = np.clip(((wi[:, 2] + 1) / 2 * n_cos).astype(np.int64), 0, n_cos - 1)
    phi = np.arctan2(wi[:, 1], wi[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    p = np.clip((phi / (2 * np.pi) * n_phi).astype(np.int64), 0, n_phi - 1)
    return c * n_phi + p
