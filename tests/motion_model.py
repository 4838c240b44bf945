"""Float64 model of moving instances, written from the definitions (pbrt-v3's AnimatedTransform; the reference's
src/core/transform.rs:264-330, 870-912, 2008-2046 and src/core/quaternion.rs), independent of the library's code:

  decompose(M)            translation, rotation quaternion (x, y, z, w), the rest S = R^-1 M (polar decomposition)
  Motion(M0, M1, t0, t1)  AnimatedTransform::new: both decompositions, the end quaternion negated when r0 . r1 < 0
  Motion.interpolate(t)   the stored matrices at or beyond the ends, T(u) R(u) S(u) between them; slerp takes the normalised
                          linear interpolation above r0 . r1 = 0.9995, as the device does
  world_triangles         an instance's triangles at a time
  closest_hits            brute-force closest hit over all triangles of all instances, every ray at its own time, with the
                          margins the tests exclude rays by
  hit_normal              the geometric normal of a hit triangle in world space at the ray's time
  shading_frames          normal through (M^-1)^T, dpdu through M and the BSDF's frame at hits of one instance at one time, with the
                          frames a wrong transform would give; to_local takes world vectors into a frame
"""
import numpy as np

SLERP_LERP_ABOVE = 0.9995


def quat_to_matrix(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r = np.empty(q.shape[:-1] + (3, 3))
    r[..., 0, 0] = 1 - 2 * (y * y + z * z)
    r[..., 0, 1] = 2 * (x * y - z * w)
    r[..., 0, 2] = 2 * (x * z + y * w)
    r[..., 1, 0] = 2 * (x * y + z * w)
    r[..., 1, 1] = 1 - 2 * (x * x + z * z)
    r[..., 1, 2] = 2 * (y * z - x * w)
    r[..., 2, 0] = 2 * (x * z - y * w)
    r[..., 2, 1] = 2 * (y * z + x * w)
    r[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return r


def matrix_to_quat(m):
    """Rotation matrix -> unit quaternion (x, y, z, w), by the largest of w and the diagonal (Shepperd)."""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        q[3] = s / 2
        s = 0.5 / s
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
    else:
        i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - (m[j, j] + m[k, k]) + 1.0)
        q[i] = s / 2
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    return q


def decompose(m):
    """4x4 affine matrix -> (T (3,), quaternion (4,), S (3, 3)) with M[:3, :3] = R S: R the orthogonal polar factor, found by
    averaging with the inverse transpose until the step is below 1e-4 in the largest row sum (at most 100 steps)."""
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    t = m[:3, 3].copy()
    a = m[:3, :3]
    r = a.copy()
    for _ in range(100):
        nxt = 0.5 * (r + np.linalg.inv(r.T))
        norm = np.abs(r - nxt).sum(axis=1).max()
        r = nxt
        if norm <= 1e-4:
            break
    return t, matrix_to_quat(r), np.linalg.inv(r) @ a


def slerp(u, q0, q1):
    """u: (...,) -> quaternions (..., 4)"""
    u = np.asarray(u, dtype=np.float64)[..., None]
    c = float(np.dot(q0, q1))
    if c > SLERP_LERP_ABOVE:
        q = (1 - u) * q0 + u * q1
        return q / np.linalg.norm(q, axis=-1, keepdims=True)
    theta = np.arccos(np.clip(c, -1.0, 1.0))
    perp = q1 - q0 * c
    perp = perp / np.linalg.norm(perp)
    return q0 * np.cos(theta * u) + perp * np.sin(theta * u)


class Motion:
    """AnimatedTransform of one instance. m0 / m1: the 4x4 at t0 / t1. m1 = None: a static instance."""

    def __init__(self, m0, m1=None, t0=0.0, t1=1.0):
        self.m0 = np.asarray(m0, dtype=np.float64).reshape(4, 4)
        self.animated = m1 is not None
        if not self.animated:
            return
        self.m1 = np.asarray(m1, dtype=np.float64).reshape(4, 4)
        self.t0, self.t1 = float(t0), float(t1)
        self.T0, self.q0, self.S0 = decompose(self.m0)
        self.T1, self.q1, self.S1 = decompose(self.m1)
        if np.dot(self.q0, self.q1) < 0:
            self.q1 = -self.q1

    def compose(self, u):
        """T(u) R(u) S(u) for u (...,) in [0, 1] -> (..., 4, 4), also at the ends (where interpolate returns the stored matrices)"""
        u = np.asarray(u, dtype=np.float64)
        out = np.zeros(u.shape + (4, 4))
        out[..., 3, 3] = 1.0
        ue = u[..., None]
        out[..., :3, 3] = (1 - ue) * self.T0 + ue * self.T1
        s = (1 - ue[..., None]) * self.S0 + ue[..., None] * self.S1
        out[..., :3, :3] = quat_to_matrix(slerp(u, self.q0, self.q1)) @ s
        return out

    def interpolate(self, time):
        """time (...,) -> object-to-world matrices (..., 4, 4)"""
        time = np.asarray(time, dtype=np.float64)
        if not self.animated:
            return np.broadcast_to(self.m0, time.shape + (4, 4)).copy()
        u = np.clip((time - self.t0) / (self.t1 - self.t0), 0.0, 1.0)
        out = self.compose(u)
        out[time <= self.t0] = self.m0
        out[time >= self.t1] = self.m1
        return out


def world_triangles(motion, positions, indices, time):
    """(n_tris, 3, 3): the instance's triangles in world space at one time"""
    m = motion.interpolate(np.float64(time))
    p = np.asarray(positions, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]
    return p[np.asarray(indices)]


def _object_rays(motion, o, d, time):
    inv = np.linalg.inv(motion.interpolate(time))
    oo = np.einsum("nij,nj->ni", inv[:, :3, :3], o) + inv[:, :3, 3]
    od = np.einsum("nij,nj->ni", inv[:, :3, :3], d)
    return oo, od


def _ray_triangles(o, d, tris):
    """Rays (n, 3) against triangles (m, 3, 3) in one space -> t, b0, b1, b2 of shape (n, m); the plane hit, whatever the barycentrics"""
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pvec = np.cross(d[:, None, :], e2[None, :, :])
    det = np.einsum("mj,nmj->nm", e1, pvec)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tvec = o[:, None, :] - p0[None, :, :]
        b1 = np.einsum("nmj,nmj->nm", tvec, pvec) * inv
        qvec = np.cross(tvec, e1[None, :, :])
        b2 = np.einsum("nj,nmj->nm", d, qvec) * inv
        t = np.einsum("mj,nmj->nm", e2, qvec) * inv
    return t, 1.0 - b1 - b2, b1, b2


def closest_hits(instances, rays_o, rays_d, t_max, time, margin=1e-4):
    """instances: list of (Motion, positions, indices). Every ray is traced at its own time, in each instance's object space
    (t is the world ray's parameter there too). Returns a dict of (n,) arrays: hit (bool), t, prim, inst, b (n, 3), and
    `unsure`: rays whose outcome hangs on less than `margin` — a barycentric of the hit below it, a second candidate within it
    (relative) of the closest t, or any triangle whose plane the ray meets within it of an edge (in barycentrics, i.e. relative
    to the triangle's size)."""
    o = np.asarray(rays_o, dtype=np.float64)
    d = np.asarray(rays_d, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    n = len(o)
    ts, bs, ids = [], [], []
    for k, (motion, pos, idx) in enumerate(instances):
        oo, od = _object_rays(motion, o, d, time)
        tris = np.asarray(pos, dtype=np.float64)[np.asarray(idx)]
        t, b0, b1, b2 = _ray_triangles(oo, od, tris)
        ts.append(t)
        bs.append(np.stack([b0, b1, b2], axis=-1))
        ids += [(k, j) for j in range(len(tris))]
    t = np.concatenate(ts, axis=1)
    b = np.concatenate(bs, axis=1)
    ids = np.asarray(ids)
    bmin = b.min(axis=-1)
    in_range = np.isfinite(t) & (t > 0) & (t <= np.asarray(t_max, dtype=np.float64)[:, None])
    inside = in_range & (bmin >= 0)
    tt = np.where(inside, t, np.inf)
    best = np.argmin(tt, axis=1)
    rows = np.arange(n)
    t_best = tt[rows, best]
    hit = np.isfinite(t_best)
    near_edge = (in_range & (np.abs(bmin) < margin)).any(axis=1)
    tt2 = tt.copy()
    tt2[rows, best] = np.inf
    second = tt2.min(axis=1)
    with np.errstate(invalid="ignore"):   # misses: inf - inf
        close_pair = hit & np.isfinite(second) & ((second - t_best) <= margin * np.abs(t_best))
    return dict(hit=hit, t=np.where(hit, t_best, np.inf), inst=np.where(hit, ids[best, 0], -1), prim=np.where(hit, ids[best, 1], -1),
                b=np.where(hit[:, None], b[rows, best], 0.0), unsure=near_edge | close_pair)


FRAME_VARIANTS = ("right", "normal_through_m", "dpdu_in_object_space")


def shading_frames(motion, positions, indices, prim, time, variant="right"):
    """The shading frame of hits on triangles `prim` (n,) of one instance at one time, in world space, from M = M(time):
    n the unit normal (p0 - p2) x (p1 - p2) of the OBJECT-space triangle taken through (M^-1)^T, dpdu = p1 - p0 (the default
    parametrisation (0, 0), (1, 0), (1, 1)) taken through M, ss = dpdu normalised, ts = n x ss (BSDF::new). Returns a dict of
    (n, 3) arrays n, dpdu, ss, ts. The wrong frames a defective kernel would give: `normal_through_m` takes the normal through M
    itself, `dpdu_in_object_space` leaves dpdu untransformed."""
    m = motion.interpolate(np.float64(time))[:3, :3]
    p = np.asarray(positions, dtype=np.float64)[np.asarray(indices)[np.asarray(prim)]]
    n_obj = np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 2])
    n = n_obj @ (m.T if variant == "normal_through_m" else np.linalg.inv(m))     # rows: (M^-1)^T n = n^T M^-1
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dpdu = p[:, 1] - p[:, 0]
    if variant != "dpdu_in_object_space":
        dpdu = dpdu @ m.T
    ss = dpdu / np.linalg.norm(dpdu, axis=1, keepdims=True)
    return dict(n=n, dpdu=dpdu, ss=ss, ts=np.cross(n, ss))


def to_local(frame, v):
    """world vectors (n, 3) in the frame's (ss, ts, n) coordinates"""
    return np.stack([(v * frame["ss"]).sum(axis=1), (v * frame["ts"]).sum(axis=1), (v * frame["n"]).sum(axis=1)], axis=1)


def hit_normal(motion, positions, indices, prim, time):
    """Unit geometric normal (p0 - p2) x (p1 - p2) of triangle `prim` at `time` in world space (the library's orientation)."""
    p = world_triangles(motion, positions, indices, time)[prim]
    nrm = np.cross(p[0] - p[2], p[1] - p[2])
    return nrm / np.linalg.norm(nrm)
