"""Maps, scenes, rays and the closed form that hold an InfiniteAreaLight with an image map to the float64 model
(envmap_model.py): shared by test_gpu_envmap.py (the device) and test_oracle_envmap.py (the CPU oracle)."""
import numpy as np

from pbrt_hip import scenes

RHO = 0.5


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    m[:3, 3] = (3.0, -1.0, 2.0)  # a translation does not move an infinite light
    return m.astype(np.float32)


def _gentle_map(h=8, w=16):
    """smooth, a few per cent of contrast, first and last columns (and rows) different"""
    t, s = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 1.0 + 0.04 * s / w + 0.02 * t / h
    return np.stack([base, base * 1.1 + 0.01 * np.sin(s), base * 0.9 + 0.01 * np.cos(t)], axis=-1).astype(np.float32)


def _sun_map(h=32, w=64, sun=(8, 11), size=2, level=2000.0, sky=0.01):
    """a 'sun' of size x size texels at row/column `sun` holding >= 99 % of the energy, over a dim sky"""
    rgb = np.full((h, w, 3), sky, np.float32) * np.array([0.6, 0.8, 1.0], np.float32)
    rgb[sun[0]:sun[0] + size, sun[1]:sun[1] + size] = np.array([1.0, 0.9, 0.7], np.float32) * level
    return rgb


def _escape_scene(light_L=(1.0, 1.0, 1.0)):
    """a small triangle off to the side and one infinite light (rays from the origin escape)"""
    return dict(positions=np.array([[5, 5, 5], [5.1, 5, 5], [5, 5.1, 5]], np.float32), indices=np.array([[0, 1, 2]], np.int32),
                tri_material=np.zeros(1, np.int32), materials=scenes._materials([(scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)]),
                tri_light=np.full(1, -1, np.int32), lights=scenes._lights([(scenes.LIGHT_INFINITE, light_L, -1, 0, 1)]))


def _escape_rays():
    rng = np.random.default_rng(7)
    d = rng.normal(size=(400, 3))
    eps = 1e-4
    special = [(1, eps, 0.1), (1, -eps, 0.1), (1, 0.0, -0.3), (1, 1e-7, 0.5), (1, -1e-7, -0.5),  # the phi seam
               (0.01, 0.02, 1), (-0.03, 0.01, 1), (0.02, -0.01, -1), (-0.01, -0.04, -1), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),  # poles
               (0.045, 0.0, 0.999), (0.0, -0.045, -0.999)]
    d = np.concatenate([d, np.asarray(special, np.float64)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[~((d[:, 0] > 0.5) & (d[:, 1] > 0.5) & (d[:, 2] > 0.5))]  # not towards the triangle
    rays = np.zeros(len(d), dtype=scenes.RAY_DTYPE)
    rays["d"] = d.astype(np.float32)
    rays["t_max"] = np.inf
    return rays


def _plane_scene(extra_zero_light=True, instanced=False):
    """a large matte quad in z = 0 (light-space +z up), the infinite light 0, and a point light of intensity 0 (so that the
    spatial strategy has two lights to choose from; it adds nothing to the expected value)"""
    e = 1000.0
    pos = np.array([[-e, -e, 0], [e, -e, 0], [e, e, 0], [-e, e, 0]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    lights = [(scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1)]
    if extra_zero_light:
        lights.append(scenes.point_light((0.0, 0.0, 5.0), (0.0, 0.0, 0.0)))
    mats = scenes._materials([(scenes.MAT_MATTE, (RHO, RHO, RHO), (0, 0, 0), 1.0)])
    if instanced:
        inst = np.zeros((1, 2, 4, 4), np.float32)
        inst[0, 0] = np.eye(4)
        inst[0, 1] = np.eye(4)
        return dict(positions=pos, indices=idx, materials=mats, instances=inst, instance_material=np.zeros(1, np.int32),
                    lights=scenes._lights(lights), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    return dict(positions=pos, indices=idx, tri_material=np.zeros(2, np.int32), materials=mats, tri_light=np.full(2, -1, np.int32),
                lights=scenes._lights(lights))


def _plane_camera(w, h):
    return scenes.orthographic_camera((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h)


def _closed_form(model):
    """rho / pi * int_{z > 0} L(w) cos(theta) dw by midpoint quadrature, 8 x 8 points per texel of level 0"""
    d, dw = model.directions(8 * model.l0.shape[0], 8 * model.l0.shape[1])
    cos = np.clip(d[:, 2], 0, None)
    return RHO / np.pi * (model.le(d) * (cos * dw)[:, None]).sum(axis=0)
