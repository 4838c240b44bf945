"""float64 numpy model of an InfiniteAreaLight with an image map, to pbrt-v3 intent:
texels x L, MIPMap::new's Lanczos resampling and box pyramid, MIPMap::lookup / triangle with ImageWrap::Repeat and a signed
floor, and the 2W x 2H sin-weighted Distribution2D (src/lights/infinite.rs:36-151, src/core/mipmap.rs, src/core/sampling.rs).
numpy only: neither the library nor the oracle."""
import numpy as np

Y = np.array([0.212671, 0.715160, 0.072169])


def pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def lanczos(x, tau=2.0):
    x = np.abs(x)
    out = np.zeros_like(x)
    small = x < 1e-5
    mid = (~small) & (x <= 1.0)
    xm = x[mid] * np.pi
    out[mid] = np.sin(xm * tau) / (xm * tau) * np.sin(xm) / xm
    out[small] = 1.0
    return out


def resample_matrix(old, new):
    """M[new, old]: MIPMap::resample_weights (4 taps, filter width 2) with Repeat."""
    m = np.zeros((new, old))
    for i in range(new):
        center = (i + 0.5) * old / new
        first = int(np.floor(center - 2.0 + 0.5))
        pos = first + np.arange(4) + 0.5
        w = lanczos((pos - center) / 2.0)
        w = w / w.sum()
        for j in range(4):
            m[i, (first + j) % old] += w[j]
    return m


def level0(rgb, L):
    """Level 0 of the MIPMap of rgb x L: (H, W, 3) float64 holding float32 values."""
    img = (np.asarray(rgb, np.float32) * np.asarray(L, np.float32).reshape(1, 1, 3)).astype(np.float64)
    h, w = img.shape[:2]
    rw, rh = pow2(w), pow2(h)
    if (rw, rh) != (w, h):
        r1 = np.einsum("so,toc->tsc", resample_matrix(w, rw), img)
        img = np.maximum(np.einsum("to,osc->tsc", resample_matrix(h, rh), r1), 0.0)
    return img.astype(np.float32).astype(np.float64)


def pyramid(l0):
    pyr = [l0]
    n_levels = 1 + int(np.log2(max(l0.shape[0], l0.shape[1])))
    for _ in range(1, n_levels):
        p = pyr[-1]
        h, w = p.shape[:2]
        nh, nw = max(1, h // 2), max(1, w // 2)
        t, s = np.arange(nh), np.arange(nw)
        tx = lambda a, b: p[np.ix_((2 * t + b) % h, (2 * s + a) % w)]  # noqa: E731
        pyr.append((tx(0, 0) + tx(1, 0) + tx(0, 1) + tx(1, 1)) * 0.25)
    return pyr


def triangle(lvl, s, t):
    """MIPMap::triangle with a signed floor and Repeat: s, t arrays -> (n, 3)."""
    h, w = lvl.shape[:2]
    s = np.asarray(s, np.float64) * w - 0.5
    t = np.asarray(t, np.float64) * h - 0.5
    s0, t0 = np.floor(s), np.floor(t)
    ds, dt = s - s0, t - t0
    s0, t0 = s0.astype(np.int64), t0.astype(np.int64)
    tx = lambda a, b: lvl[(t0 + b) % h, (s0 + a) % w]  # noqa: E731
    return (tx(0, 0) * ((1 - ds) * (1 - dt))[..., None] + tx(0, 1) * ((1 - ds) * dt)[..., None]
            + tx(1, 0) * (ds * (1 - dt))[..., None] + tx(1, 1) * (ds * dt)[..., None])


def lookup(pyr, s, t, width):
    levels = len(pyr)
    level = levels - 1 + np.log2(max(width, 1e-8))
    if level < 0:
        return triangle(pyr[0], s, t)
    if level > levels - 1:
        return np.broadcast_to(pyr[-1][0, 0], np.shape(s) + (3,))
    il = int(np.floor(level))
    d = level - il
    return (1 - d) * triangle(pyr[il], s, t) + d * triangle(pyr[min(il + 1, levels - 1)], s, t)


def dist_func(pyr):
    h, w = pyr[0].shape[:2]
    nu, nv = 2 * w, 2 * h
    vp = (np.arange(nv) + 0.5) / nv
    up = (np.arange(nu) + 0.5) / nu
    S, T = np.meshgrid(up, vp)
    c = lookup(pyr, S, T, 0.5 / min(nu, nv))
    return (c @ Y) * np.sin(np.pi * vp)[:, None]


def power(pyr):
    return lookup(pyr, np.array([0.5]), np.array([0.5]), 0.5)[0]


class EnvModel:
    """The whole light: tables, le(world direction), pdf(world direction), integrals by quadrature."""

    def __init__(self, rgb, L=(1.0, 1.0, 1.0), light_to_world=None):
        self.l0 = level0(rgb, L)
        self.pyr = pyramid(self.l0)
        self.func = dist_func(self.pyr)
        self.nv, self.nu = self.func.shape
        self.row_int = self.func.mean(axis=1)
        self.marg_int = self.row_int.mean()
        m = np.eye(4) if light_to_world is None else np.asarray(light_to_world, np.float32).astype(np.float64).reshape(4, 4)
        self.l2w = m[:3, :3]
        self.w2l = np.linalg.inv(self.l2w)

    def uv(self, d_world):
        wl = np.asarray(d_world, np.float64) @ self.w2l.T
        wl = wl / np.linalg.norm(wl, axis=-1, keepdims=True)
        theta = np.arccos(np.clip(wl[..., 2], -1, 1))
        phi = np.arctan2(wl[..., 1], wl[..., 0])
        phi = np.where(phi < 0, phi + 2 * np.pi, phi)
        return phi / (2 * np.pi), theta / np.pi

    def le(self, d_world):
        u, v = self.uv(d_world)
        return triangle(self.l0, u, v)

    def pdf(self, d_world):
        """InfiniteAreaLight::pdf_li: solid-angle density of sampling by the Distribution2D."""
        u, v = self.uv(d_world)
        st = np.sin(v * np.pi)
        iu = np.clip((u * self.nu).astype(np.int64), 0, self.nu - 1)
        iv = np.clip((v * self.nv).astype(np.int64), 0, self.nv - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(st > 0, self.func[iv, iu] / self.marg_int / (2 * np.pi ** 2 * st), 0.0)

    def directions(self, n_theta, n_phi):
        """Midpoint quadrature over the sphere in light space: world directions (n, 3) and solid angles (n,)."""
        th = (np.arange(n_theta) + 0.5) / n_theta * np.pi
        ph = (np.arange(n_phi) + 0.5) / n_phi * 2 * np.pi
        T, P = np.meshgrid(th, ph, indexing="ij")
        wl = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
        dw = (np.sin(T) * (np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)
        return wl @ self.l2w.T, dw
