"""float64 model of the quadric shapes (Sphere, Disk, Cylinder under an affine transform): numpy only, no project code.

A shape is a dict: type ("sphere" | "disk" | "cylinder"), radius, z_min, z_max (disk: z_min = z_max = height), inner_radius,
phi_max (radians), o2w (4x4 float64), reverse (bool). `from_record` makes one from a PbrtShape record (any mapping with the
header's field names), applying what the constructors apply: ordered z, the sphere's z clamped to the radius, phi_max
clamped to [0, 360] degrees.

intersect() follows the textbook definitions, not the device's operation order: roots of the quadratic in float64, the
nearer root first, each rejected by its t range, z range and sweep angle. Beside the verdict it reports `near`: some
quantity a decision rests on lies within REL = 1e-4 (relative to that quantity's natural scale) of the boundary it is
compared with, so float32 arithmetic may decide the other way. Only quantities that are actually consulted count: the
farther root's only when the nearer root was rejected.
"""
import numpy as np

REL = 1e-4
TWO_PI = 2.0 * np.pi
TYPES = ("sphere", "disk", "cylinder")  # PbrtShapeType 0, 1, 2


def from_record(rec):
    kind = TYPES[int(rec["type"])]
    r = float(rec["radius"])
    z0, z1 = float(min(rec["z_min"], rec["z_max"])), float(max(rec["z_min"], rec["z_max"]))
    if kind == "sphere":
        z0, z1 = float(np.clip(z0, -r, r)), float(np.clip(z1, -r, r))
    if kind == "disk":
        z0 = z1 = float(rec["z_min"])
    return dict(type=kind, radius=r, z_min=z0, z_max=z1, inner_radius=float(rec["inner_radius"]) if kind == "disk" else 0.0,
                phi_max=np.radians(float(np.clip(rec["phi_max"], 0.0, 360.0))),
                o2w=np.asarray(rec["to_world"], dtype=np.float64).reshape(4, 4), reverse=bool(rec["reverse_orientation"]))


def make(kind, radius, z_min, z_max, inner_radius=0.0, phi_max_deg=360.0, o2w=None, reverse=False):
    return from_record(dict(type=TYPES.index(kind), radius=radius, z_min=z_min, z_max=z_max, inner_radius=inner_radius,
                            phi_max=phi_max_deg, to_world=np.eye(4) if o2w is None else o2w, reverse_orientation=reverse))


def swaps_handedness(shape):
    return np.linalg.det(shape["o2w"][:3, :3]) < 0.0


def object_bound(shape):
    r = shape["radius"]
    return np.array([-r, -r, shape["z_min"]]), np.array([r, r, shape["z_max"]])


def world_bounds(shape):
    """object_to_world * object_bound(): the union of the eight transformed corners, in float64."""
    lo, hi = object_bound(shape)
    corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2], 1.0] for c in range(8)])
    w = corners @ shape["o2w"].T
    return w[:, :3].min(axis=0), w[:, :3].max(axis=0)


def area(shape):
    r = shape["radius"]
    if shape["type"] == "sphere":
        return shape["phi_max"] * r * (shape["z_max"] - shape["z_min"])
    if shape["type"] == "disk":
        return shape["phi_max"] * 0.5 * (r * r - shape["inner_radius"] ** 2)
    return (shape["z_max"] - shape["z_min"]) * r * shape["phi_max"]


def surface_points(shape, u, v):
    """Object-space points of the parametrisation at u, v in [0, 1] (arrays): what `area` integrates over."""
    r, phi = shape["radius"], u * shape["phi_max"]
    if shape["type"] == "sphere":
        z = shape["z_min"] + v * (shape["z_max"] - shape["z_min"])
        rho = np.sqrt(np.maximum(r * r - z * z, 0.0))
        return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=-1)
    if shape["type"] == "disk":
        rho = shape["inner_radius"] + v * (r - shape["inner_radius"])
        return np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full_like(rho, shape["z_min"])], axis=-1)
    z = shape["z_min"] + v * (shape["z_max"] - shape["z_min"])
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


def implicit_residual(shape, p):
    """0 on the (unbounded) surface the shape is cut from, relative to the radius."""
    r = shape["radius"]
    if shape["type"] == "sphere":
        return (np.sqrt((p ** 2).sum(axis=-1)) - r) / r
    if shape["type"] == "disk":
        return (p[..., 2] - shape["z_min"]) / r
    return (np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - r) / r


def _phi(p):
    phi = np.arctan2(p[..., 1], p[..., 0])
    return np.where(phi < 0.0, phi + TWO_PI, phi)


def _near_phi(shape, phi):
    near = (phi <= REL * TWO_PI) | (phi >= TWO_PI * (1.0 - REL))
    return near | (np.abs(phi - shape["phi_max"]) <= REL * TWO_PI)


def intersect(shape, o, d, t_max=np.inf):
    """o, d: (n, 3) world-space rays (d need not be normalised); t_max: scalar or (n,). Returns a dict of arrays:
    hit (bool), t, p (object-space hit point), phi, n (world-space unit normal as the shading code orients it), near.
    A ray exactly down the axis of a disk with inner_radius 0 hits its centre: p = (0, 0, height), phi = 0, not `near` on account
    of the sweep (surface_frame gives that hit the tangent of phi = 0)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n_rays = o.shape[0]
    t_max = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (n_rays,))
    w2o = np.linalg.inv(shape["o2w"])
    oo = o @ w2o[:3, :3].T + w2o[:3, 3]
    dd = d @ w2o[:3, :3].T
    r, kind = shape["radius"], shape["type"]
    t_scale = np.maximum(np.sqrt((oo ** 2).sum(axis=1)) / np.sqrt((dd ** 2).sum(axis=1)), 1e-30)  # time to travel |origin|

    def near_t(t):
        tm = np.where(np.isfinite(t_max), t_max, 0.0)
        return (np.abs(t) <= REL * np.maximum(t_scale, np.abs(t))) | \
               (np.isfinite(t_max) & (np.abs(t - tm) <= REL * np.maximum(np.abs(t), np.abs(tm))))

    hit = np.zeros(n_rays, dtype=bool)
    near = np.zeros(n_rays, dtype=bool)
    t_hit = np.full(n_rays, np.inf)
    p_hit = np.zeros((n_rays, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "disk":
            dz = dd[:, 2]
            near |= np.abs(dz) <= REL * np.sqrt((dd ** 2).sum(axis=1))
            t = (shape["z_min"] - oo[:, 2]) / dz
            ok = (dz != 0.0) & (t > 0.0) & (t < t_max)
            near |= (dz != 0.0) & near_t(t)
            p = oo + dd * np.where(ok, t, 0.0)[:, None]
            rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
            on_axis = rho <= 1e-12 * r  # a ray down the axis, up to float64's own rounding through the transform
            p[on_axis, :2], rho[on_axis] = 0.0, 0.0
            inside = (rho <= r) & (rho >= shape["inner_radius"])
            near |= ok & ((np.abs(rho - r) <= REL * r) |
                          ((shape["inner_radius"] > 0.0) & (np.abs(rho - shape["inner_radius"]) <= REL * shape["inner_radius"])))
            phi = _phi(p)
            # the centre (rho == 0: a ray down the axis) belongs to every sector and is no boundary of the sweep: the
            # hit is taken there with phi = 0, the device's too (it nudges the point to x = 1e-5 r as the sphere's pole)
            near |= ok & inside & (rho > 0.0) & _near_phi(shape, phi)
            hit = ok & inside & (phi <= shape["phi_max"])
            t_hit = np.where(hit, t, np.inf)
            p_hit = p
            p_hit[:, 2] = shape["z_min"]
        else:
            k = 3 if kind == "sphere" else 2
            a = (dd[:, :k] ** 2).sum(axis=1)
            b = 2.0 * (dd[:, :k] * oo[:, :k]).sum(axis=1)
            c = (oo[:, :k] ** 2).sum(axis=1) - r * r
            disc = b * b - 4.0 * a * c
            near |= np.abs(disc) <= REL * (b * b + np.abs(4.0 * a * c))
            real = (disc >= 0.0) & (a > 0.0)
            root = np.sqrt(np.maximum(disc, 0.0))
            q = np.where(b < 0.0, -0.5 * (b - root), -0.5 * (b + root))
            ta, tb = q / a, c / q
            t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
            pending = real.copy()
            for t in (t0, t1):
                in_range = pending & (t > 0.0) & (t <= t_max)
                near |= pending & near_t(t)
                p = oo + dd * np.where(in_range, t, 0.0)[:, None]
                if kind == "sphere":
                    p = p * (r / np.sqrt((p ** 2).sum(axis=1)))[:, None]
                    z_ok = ((shape["z_min"] <= -r) | (p[:, 2] >= shape["z_min"])) & ((shape["z_max"] >= r) | (p[:, 2] <= shape["z_max"]))
                    near_z = ((shape["z_min"] > -r) & (np.abs(p[:, 2] - shape["z_min"]) <= REL * r)) | \
                             ((shape["z_max"] < r) & (np.abs(p[:, 2] - shape["z_max"]) <= REL * r))
                else:
                    p[:, :2] *= (r / np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2))[:, None]
                    z_ok = (p[:, 2] >= shape["z_min"]) & (p[:, 2] <= shape["z_max"])
                    near_z = (np.abs(p[:, 2] - shape["z_min"]) <= REL * r) | (np.abs(p[:, 2] - shape["z_max"]) <= REL * r)
                phi = _phi(p)
                near |= in_range & (near_z | _near_phi(shape, phi))
                accept = in_range & z_ok & (phi <= shape["phi_max"])
                t_hit = np.where(accept, t, t_hit)
                p_hit = np.where(accept[:, None], p, p_hit)
                hit |= accept
                pending &= ~accept
    return dict(hit=hit, t=t_hit, p=p_hit, phi=_phi(p_hit), n=np.where(hit[:, None], normal_at(shape, p_hit), 0.0), near=near)


def normal_at(shape, p_obj):
    """The world-space unit normal at the object-space points p_obj (n, 3) as the shading code orients it:
    normalize(dpdu x dpdv) points outward for the sphere and the cylinder, along +z for the disk; flipped by
    reverse_orientation ^ transform_swaps_handedness; to world space by the inverse transpose."""
    p_obj = np.asarray(p_obj, dtype=np.float64)
    r, kind = shape["radius"], shape["type"]
    if kind == "sphere":
        n_obj = p_obj / r
    elif kind == "cylinder":
        n_obj = np.stack([p_obj[:, 0], p_obj[:, 1], np.zeros(len(p_obj))], axis=1) / r
    else:
        n_obj = np.tile(np.array([0.0, 0.0, 1.0]), (len(p_obj), 1))
    if shape["reverse"] != bool(swaps_handedness(shape)):
        n_obj = -n_obj
    n_w = n_obj @ np.linalg.inv(shape["o2w"])[:3, :3]  # (M^-1)^T n
    with np.errstate(divide="ignore", invalid="ignore"):
        return n_w / np.sqrt((n_w ** 2).sum(axis=1))[:, None]


AXIS_NUDGE = 1e-5  # times the radius: where the device puts a hit on a sphere's pole or a disk's centre (phi = 0)


def surface_frame(shape, hit):
    """The shading frame at the hits of intersect() (every row; rows that missed hold zeros and NaNs). World space, float64:
    dpdu = M dpdu_obj with dpdu_obj = (-phi_max y, phi_max x, 0) at the object-space hit point (the derivative of the
    parametrisation by u: phi = u phi_max) and M the linear part of o2w; ss = dpdu / |dpdu|; ns = hit["n"] (the shading normal is
    the geometric one, face-forwarded onto itself); ts = ns x ss. On the axis (x = y = 0: the sphere's pole, the disk's centre)
    the point is taken at x = AXIS_NUDGE * radius, so dpdu has the direction of M e_y."""
    p = np.array(hit["p"], dtype=np.float64)
    on_axis = (p[:, 0] == 0.0) & (p[:, 1] == 0.0)
    p[on_axis, 0] = AXIS_NUDGE * shape["radius"]
    dpdu_obj = np.stack([-shape["phi_max"] * p[:, 1], shape["phi_max"] * p[:, 0], np.zeros(len(p))], axis=1)
    dpdu = dpdu_obj @ shape["o2w"][:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = dpdu / np.sqrt((dpdu ** 2).sum(axis=1))[:, None]
    ns = np.asarray(hit["n"], dtype=np.float64)
    return dict(dpdu=dpdu, ss=ss, ns=ns, ts=np.cross(ns, ss))


def to_local(frame, w):
    """World-space directions w (n, 3) in the frame's coordinates: (w . ss, w . ts, w . ns)."""
    w = np.asarray(w, dtype=np.float64)
    return np.stack([(w * frame["ss"]).sum(axis=-1), (w * frame["ts"]).sum(axis=-1), (w * frame["ns"]).sum(axis=-1)], axis=-1)


def world_point(shape, p_obj):
    return np.asarray(p_obj, dtype=np.float64) @ shape["o2w"][:3, :3].T + shape["o2w"][:3, 3]


def reflect_about(d, n):
    """The mirror direction of the incoming ray direction d about the normal n (either orientation of n)."""
    return d - 2.0 * (d * n).sum(axis=-1, keepdims=True) * n


def intersect_scene(shapes, o, d, t_max=np.inf):
    """Closest hit over a list of shapes: (prim index in the list or -1, t, near). `near` also flags rays whose two nearest
    candidate hits lie within REL of each other (the closer one could be either)."""
    n = len(o)
    best_t, best = np.full(n, np.inf), np.full(n, -1)
    second = np.full(n, np.inf)
    near = np.zeros(n, dtype=bool)
    for i, s in enumerate(shapes):
        r = intersect(s, o, d, t_max)
        near |= r["near"]
        closer = r["hit"] & (r["t"] < best_t)
        second = np.where(closer, best_t, np.where(r["hit"], np.minimum(second, r["t"]), second))
        best = np.where(closer, i, best)
        best_t = np.where(closer, r["t"], best_t)
    near |= np.isfinite(second) & (second - best_t <= REL * second)
    return best, best_t, near


def rays_at_unit_cube(n, seed):
    """The ray generator of the GPU tests: origins uniform on the sphere of radius 3, aimed at uniform points of [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = 3.0 * v / np.sqrt((v ** 2).sum(axis=1))[:, None]
    target = rng.uniform(-1.0, 1.0, size=(n, 3))
    d = target - o
    d /= np.sqrt((d ** 2).sum(axis=1))[:, None]
    return o.astype(np.float32), d.astype(np.float32)


# ---- the Lambert probe: a matte shape under three pairs of opposite distant lights ----
PROBE_OFFSETS = (1e-3, 1e-4)  # how far a shadow ray's origin is pushed off the surface, both tried


def occluded_from_surface(shape, p_obj, w, t_max=np.inf):
    """Does the shape block the world-space direction w (n, 3) seen from its own surface points p_obj (n, 3, object space)? The
    ray starts ON the surface: a sphere's or cylinder's quadratic has the root 0 there (the point itself, not counted) and the
    other root -b / a; a disk cannot block its own points. Returns (blocked, near), `near` as in intersect(): the other root
    within REL of 0 (a tangent ray), or its point within REL of an edge of the cut. With t_max the segment p + t w, t < t_max,
    stands for the ray (t_max = 1 and w the vector to a point light: the part of the ray beyond the light blocks nothing); a
    root within REL of t_max is `near` as well."""
    n_rays = len(p_obj)
    blocked, near = np.zeros(n_rays, dtype=bool), np.zeros(n_rays, dtype=bool)
    if shape["type"] == "disk":
        return blocked, near
    w2o = np.linalg.inv(shape["o2w"])
    dd = np.asarray(w, dtype=np.float64) @ w2o[:3, :3].T
    r = shape["radius"]
    k = 3 if shape["type"] == "sphere" else 2
    a = (dd[:, :k] ** 2).sum(axis=1)
    b = 2.0 * (dd[:, :k] * p_obj[:, :k]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(a > 0.0, -b / a, -np.inf)
        near |= (a <= 0.0) | (np.abs(t) <= REL * r / np.sqrt((dd ** 2).sum(axis=1)))
        if np.isfinite(t_max):
            near |= np.abs(t - t_max) <= REL * t_max
        ahead = (t > 0.0) & (t < t_max)
        p = p_obj + dd * np.where(ahead, t, 0.0)[:, None]
        if shape["type"] == "sphere":
            z_ok = ((shape["z_min"] <= -r) | (p[:, 2] >= shape["z_min"])) & ((shape["z_max"] >= r) | (p[:, 2] <= shape["z_max"]))
            near_z = ((shape["z_min"] > -r) & (np.abs(p[:, 2] - shape["z_min"]) <= REL * r)) | \
                     ((shape["z_max"] < r) & (np.abs(p[:, 2] - shape["z_max"]) <= REL * r))
        else:
            z_ok = (p[:, 2] >= shape["z_min"]) & (p[:, 2] <= shape["z_max"])
            near_z = (np.abs(p[:, 2] - shape["z_min"]) <= REL * r) | (np.abs(p[:, 2] - shape["z_max"]) <= REL * r)
        phi = _phi(p)
        near |= ahead & (near_z | _near_phi(shape, phi))
        blocked = ahead & z_ok & (phi <= shape["phi_max"])
    return blocked, near


def lambert_probe(shape, o, d, axes):
    """A matte shape under six distant lights along +-axes[:, k] (axes: 3x3, orthonormal columns), the pair of column k
    emitting in colour channel k alone. For the world-space rays o, d: what one surface interaction of direct lighting returns
    in channel k is rho / pi * L * expect[:, k].

    expect[:, k] = |n . a_k| when the light of pair k on the viewer's side of the surface is not shadowed by the shape itself,
    else 0 (the light on the far side never contributes to a matte surface). Shadowing: a float64 ray from the world-space hit
    point pushed along the viewer-side normal by each of PROBE_OFFSETS, and the ray from the surface point itself
    (occluded_from_surface: the device pushes its ray by a few ulps only, and between offset 0 and the smaller offset the far
    end of a slanting ray still moves by about that offset). A ray is `clear` when all three give one verdict and none is
    flagged near. Returns a dict of arrays over the rays: hit, near (of the primary hit), n (the model's world-space normal),
    expect (n, 3), shadowed (n, 3; the common verdict), keep (a hit that is not near and whose three shadow rays are clear).
    Which light of a pair is "on the viewer's side" flips where n . a_k = 0; the value is continuous through 0 there, so that
    decision excludes nothing."""
    o64, d64 = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    m = intersect(shape, o, d)
    hit = m["hit"]
    idx = np.flatnonzero(hit)
    n = m["n"][idx]
    side = np.where((n * d64[idx]).sum(axis=1) < 0.0, 1.0, -1.0)
    nv = n * side[:, None]  # the normal on the viewer's side
    p_w = m["p"][idx] @ shape["o2w"][:3, :3].T + shape["o2w"][:3, 3]
    cos = n @ axes
    toward = np.where(nv @ axes >= 0.0, 1.0, -1.0)  # which light of each pair is on the viewer's side
    expect = np.zeros((len(o64), 3))
    shadowed = np.zeros((len(o64), 3), dtype=bool)
    clear = np.ones((len(o64), 3), dtype=bool)
    for k in range(3):
        w = toward[:, k, None] * axes[:, k]
        verdicts = [intersect(shape, p_w + eps * nv, w) for eps in PROBE_OFFSETS]
        blocked, blocked_near = occluded_from_surface(shape, m["p"][idx], w)
        ok = ~blocked_near & ~verdicts[0]["near"] & ~verdicts[1]["near"] & (verdicts[0]["hit"] == blocked) & (verdicts[1]["hit"] == blocked)
        shadowed[idx, k] = blocked
        clear[idx, k] = ok
        expect[idx, k] = np.where(blocked, 0.0, np.abs(cos[:, k]))
    return dict(hit=hit, n=m["n"], expect=expect, shadowed=shadowed, keep=hit & ~m["near"] & clear.all(axis=1), near=m["near"])


# ---- closed forms of the area-light tests ----
def disk_light_floor_radiance(rho, L, R, h):
    """Radiance leaving a Lambertian floor point (albedo rho) under the centre of a disk light of radius R at height h that
    faces it: E = pi L R^2 / (h^2 + R^2), Lo = rho / pi * E."""
    return rho * L * R * R / (h * h + R * R)


def cylinder_light_centre_radiance(rho, L, R, H):
    """The same for a Lambertian patch at the centre of a cylinder of radius R, z in [-H, H], emitting inward, the patch's
    normal along the axis: the cylinder fills the hemisphere below polar angle atan(R / H) ... pi / 2, i.e.
    E = pi L (1 - sin^2(theta_0)) with tan(theta_0) = R / H, Lo = rho L H^2 / (H^2 + R^2)."""
    return rho * L * H * H / (H * H + R * R)


def partial_cylinder_light_centre_radiance(rho, L, R, H, phi_max):
    """The same under a cylinder cut to the sweep phi_max (radians): the patch's cosine does not depend on the azimuth, so every
    sector of the cylinder gives the irradiance its angle's share."""
    return cylinder_light_centre_radiance(rho, L, R, H) * phi_max / TWO_PI


def sphere_light_floor_radiance(rho, L, R, d):
    """A sphere of radius R whose centre is d > R above the floor point along the floor's normal: it fills the cone of
    sin(theta_max) = R / d about the normal, E = pi L sin^2(theta_max), Lo = rho L (R / d)^2."""
    return rho * L * (R / d) ** 2


def annulus_light_floor_radiance(rho, L, R, Ri, h):
    """disk_light_floor_radiance of the disk of radius R less that of the hole of radius Ri."""
    return disk_light_floor_radiance(rho, L, R, h) - disk_light_floor_radiance(rho, L, Ri, h)


def frame_about(n):
    """Some orthonormal frame (ss, ts, ns) with ns = n / |n|, as 3-vectors."""
    ns = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    a = np.eye(3)[np.argmin(np.abs(ns))]
    ss = np.cross(a, ns)
    ss /= np.linalg.norm(ss)
    return dict(ss=ss, ts=np.cross(ns, ss), ns=ns)


def bsdf_patch_radiance_by_quadrature(shape, p, frame, wo, f, L, cells=400, weight=None):
    """Radiance leaving the world-space point p towards wo (world space) whose BSDF is the callable f(wo_local, wi_local) ->
    (n,) or (n, 3) in the frame (ss, ts, ns as 3-vectors; to_local's coordinates), under the shape as a diffuse emitter of
    radiance L that nothing shadows: L * integral of f(wo, wi) |cos_p| |cos_s| / r^2 dA by the midpoint rule over cells x cells
    cells of the shape's parametrisation (surface_points), through its transform. weight(wi_local, r2, cos_s) -> (n,), if given,
    multiplies the integrand (cos_s: the unit cosine at the emitter; what a pdf over its area needs). Returns (value, |value -
    value at cells / 2|): the second is the estimate of the quadrature's error."""
    wo_l = to_local(frame, np.asarray(wo, dtype=np.float64)[None, :])

    def at(cells):
        u = (np.arange(cells) + 0.5) / cells
        uu, vv = np.meshgrid(u, u, indexing="ij")
        m, h = shape["o2w"], 1e-6

        def world(a, b):
            return surface_points(shape, a, b) @ m[:3, :3].T + m[:3, 3]

        q = world(uu, vv)
        normal_da = np.cross((world(uu + h, vv) - world(uu - h, vv)) / (2 * h), (world(uu, vv + h) - world(uu, vv - h)) / (2 * h))
        w = (q - np.asarray(p, dtype=np.float64)).reshape(-1, 3)
        r2 = (w ** 2).sum(axis=-1)
        wi = w / np.sqrt(r2)[:, None]
        wi_l = to_local(frame, wi)
        normal_da = normal_da.reshape(-1, 3)
        cos_s_da = np.abs((wi * normal_da).sum(axis=-1))
        fv = np.asarray(f(np.broadcast_to(wo_l, wi_l.shape), wi_l), dtype=np.float64)
        g = np.abs(wi_l[:, 2]) * cos_s_da / r2
        if weight is not None:
            g = g * weight(wi_l, r2, cos_s_da / np.sqrt((normal_da ** 2).sum(axis=-1)))
        return L * (fv * (g[:, None] if fv.ndim == 2 else g)).mean(axis=0)

    fine = at(cells)
    return fine, np.abs(fine - at(cells // 2))


def patch_radiance_by_quadrature(shape, p, n_p, rho, L, cells=400):
    """Radiance leaving a Lambertian patch (albedo rho) at the world-space point p with normal n_p under the shape as a
    two-sided diffuse emitter of radiance L that nothing shadows: rho / pi * L * integral of max(0, cos_p) |cos_s| / r^2 dA: the
    Lambertian case of bsdf_patch_radiance_by_quadrature (f = rho / pi above the patch, 0 below it; seen from above)."""
    frame = frame_about(n_p)
    value, _ = bsdf_patch_radiance_by_quadrature(shape, p, frame, frame["ns"], lambda wo, wi: np.where(wi[:, 2] > 0.0, rho / np.pi, 0.0), L, cells)
    return value
