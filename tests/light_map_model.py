"""float64 numpy model of ProjectionLight and GonioPhotometricLight (src/lights/projection.rs, goniometric.rs) to pbrt-v3 intent
(SURVEY.md D88, D89): the MIPMap over the texels as they are (envmap_model.py: resampling, pyramid, bilinear lookup with Repeat),
projection(w), scale(w), sample_li(p) and power(). numpy only: neither the library nor the oracle."""
import numpy as np

import envmap_model as em

PROJECTION, GONIOMETRIC = 5, 6
HITHER = 1e-3


def gentle_map(h, w, seed=0):
    """smooth texels in [0.5, 2] with tens of per cent of contrast along both axes; no two rows or columns alike"""
    t, s = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 0.8 + 0.7 * s / max(w - 1, 1) + 0.35 * t / max(h - 1, 1)
    rgb = np.stack([base, 0.6 + 0.9 * (base - 0.8), 1.9 - 0.8 * (base - 0.8) + 0.02 * np.sin(s + seed)], axis=-1)
    return np.clip(rgb, 0.5, 2.0).astype(np.float32)


def rigid(axis, deg, translate):
    """light_to_world: a rotation about `axis` and a translation, float32 (what the library receives)"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    m[:3, 3] = translate
    return m.astype(np.float32)


def screen_bounds(rgb):
    """(min.x, min.y, max.x, max.y): projection.rs:57-69; aspect = width / height of the map as passed, 1 without one"""
    aspect = 1.0 if rgb is None else rgb.shape[1] / rgb.shape[0]
    if aspect > 1.0:
        return np.array([-aspect, -1.0, aspect, 1.0])
    return np.array([-1.0, -1.0 / aspect, 1.0, 1.0 / aspect])


class LightMapModel:
    def __init__(self, kind, light_to_world=None, intensity=(1.0, 1.0, 1.0), fov=0.0, rgb=None):
        self.kind = kind
        m = np.eye(4) if light_to_world is None else np.asarray(light_to_world, np.float32).astype(np.float64).reshape(4, 4)
        # what the library receives: p_light and the inverse upper 3x3, rounded once
        self.p_light = m[:3, 3].astype(np.float32).astype(np.float64)
        self.w2l = np.linalg.inv(m[:3, :3]).astype(np.float32).astype(np.float64)
        self.I = np.asarray(intensity, np.float32).astype(np.float64)
        self.rgb = None if rgb is None else np.asarray(rgb, np.float32)
        self.l0 = None if rgb is None else em.level0(self.rgb, (1.0, 1.0, 1.0))
        self.pyr = None if rgb is None else em.pyramid(self.l0)
        if kind == PROJECTION:
            self.sb = screen_bounds(self.rgb)
            self.inv_tan = 1.0 / np.tan(np.radians(float(np.float32(fov))) / 2.0)
            corner = np.array([self.sb[2] / self.inv_tan, self.sb[3] / self.inv_tan, 1.0])  # screen_to_light * (max.x, max.y, 0)
            self.cos_total_width = (corner / np.linalg.norm(corner))[2]

    def lookup_half(self):
        """lookup((0.5, 0.5), 0.5); 1 without a map"""
        return np.ones(3) if self.pyr is None else em.power(self.pyr)

    # ---- ProjectionLight::projection (projection.rs:90-106) ----
    def screen_point(self, w):
        """light-space wl (not normalised) and the projected p = perspective(fov, 1e-3, 1e30) * wl as a point"""
        wl = np.asarray(w, np.float64) @ self.w2l.T
        with np.errstate(divide="ignore", invalid="ignore"):
            p = self.inv_tan * wl[..., :2] / wl[..., 2:3]
        return wl, p

    def projection(self, w):
        wl, p = self.screen_point(w)
        lit = (wl[..., 2] >= HITHER) & (p[..., 0] >= self.sb[0]) & (p[..., 0] <= self.sb[2]) & (p[..., 1] >= self.sb[1]) & \
            (p[..., 1] <= self.sb[3])
        out = np.zeros(np.shape(w)[:-1] + (3,))
        if self.l0 is None:
            out[lit] = 1.0
            return out
        s = (p[lit, 0] - self.sb[0]) / (self.sb[2] - self.sb[0])  # Bounds2::offset
        t = (p[lit, 1] - self.sb[1]) / (self.sb[3] - self.sb[1])
        out[lit] = em.triangle(self.l0, s, t)
        return out

    # ---- GonioPhotometricLight::scale (goniometric.rs:65-76) ----
    def gonio_st(self, w):
        wl = np.asarray(w, np.float64) @ self.w2l.T
        wl = wl / np.linalg.norm(wl, axis=-1, keepdims=True)
        x, y, z = wl[..., 0], wl[..., 2], wl[..., 1]  # y and z swapped
        theta = np.arccos(np.clip(z, -1, 1))
        phi = np.arctan2(y, x)
        phi = np.where(phi < 0, phi + 2 * np.pi, phi)
        return phi / (2 * np.pi), theta / np.pi

    def scale(self, w):
        if self.l0 is None:
            return np.ones(np.shape(w)[:-1] + (3,))
        s, t = self.gonio_st(w)
        return em.triangle(self.l0, s, t)

    def map_value(self, w):
        return self.projection(w) if self.kind == PROJECTION else self.scale(w)

    # ---- Light::sample_li: wi, pdf, Li = I * map(-wi) / d^2 (D88: the product) ----
    def sample_li(self, p):
        d = self.p_light - np.asarray(p, np.float64)
        d2 = (d * d).sum(axis=-1, keepdims=True)
        wi = d / np.sqrt(d2)
        return wi, np.ones(len(wi)), self.I * self.map_value(-wi) / d2

    # ---- Light::power: goniometric.rs:105-113; pbrt-v3's ProjectionLight::Power (D89) ----
    def power(self):
        cone = 4.0 * np.pi if self.kind == GONIOMETRIC else 2.0 * np.pi * (1.0 - self.cos_total_width)
        return self.I * self.lookup_half() * cone
