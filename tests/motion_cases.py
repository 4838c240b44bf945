"""Scenes, rays and expected values of the moving-instance tests, CPU only (numpy, tests/motion_model.py and the scene helpers
of pbrt_hip.scenes): shared by test_gpu_motion.py, test_gpu_motion_paths.py (the device held to them) and
test_motion_cases_model.py (the builders held to the model, and every cap and floor below checked without a GPU).

  the helpers of test_gpu_motion.py    make_scene, rot / tr / sc, rays_at, some_times, model_hits, check_ids, FIVE, the blur scene
  path_time_case                       specular chains under a sliding black occluder: which static scene every ray must equal
  ROW_INSTANCES, lambert_case,         scale and shear at the shaded hit: Lambert's law, anisotropic rows under a point light
  aniso_case, shadow_start_case        (with the wrong frames), the shadow of a scaled box on a plane
  depth_instances                      64 instances from a seeded generator, by kind of motion
  end_times, static_at                 the ends of the time range
  scrambled_radical_inverse            the Halton sampler's time dimension
  level_scenes                         plastic / metal, set_material and Disney rows on an all-static scene

Caps and floors (the values test_motion_cases_model.py measures are in its docstring):
  EDGE = 1e-3        a chain that passes within it of the occluder's edge is excluded            MAX_EXCLUDED = 2 % of the rays
  MIN_SWITCHED = 100 rays per class covered at their own time but not at the start, and the other way round
  ANISO_FLOOR = 1e-3 the model's largest channel below it: the ray is not compared              MIN_KEPT = 800 rays per material
  MIN_KIND_HITS = 50 hits on negated-quaternion, normalised-lerp and scaled instances each
"""
import itertools

import numpy as np

import disney_model as dm
import microfacet_model as mfm
import motion_model as mm
from glossy_cases import ETA, K
from pbrt_hip import scenes

T0, T1 = 0.25, 1.75
N_RAYS = 4096
QUAD = (np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], dtype=np.float32),
        np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
_c = np.array([[x, y, z] for z in (-0.25, 0.25) for y in (-0.3, 0.3) for x in (-0.4, 0.4)], dtype=np.float32)
BOX = (_c, np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                     [1, 3, 5], [3, 7, 5]], dtype=np.int32))
OBJECTS = (QUAD, BOX)
KD, LIGHT_L = 0.5, 3.0


def rot(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = np.radians(degrees) / 2
    m = np.eye(4)
    m[:3, :3] = mm.quat_to_matrix(np.concatenate([a * np.sin(h), [np.cos(h)]]))
    return m


def tr(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def sc(x, y, z):
    return np.diag([x, y, z, 1.0])


def f32(m):
    return np.asarray(m, dtype=np.float32).astype(np.float64)


# (object, start matrix, end matrix or None): translation, 170 degree rotation, rotation + translation + non-uniform scale, the
# normalised-lerp branch, and a static box
FIVE = [(0, tr(-2, 0, 0) @ rot((0, 1, 0), 20), tr(-2, 1, 0.5) @ rot((0, 1, 0), 20)),
        (1, rot((0.3, 1.0, 0.2), 5), rot((0.3, 1.0, 0.2), 175)),
        (1, tr(2, 0, 0) @ rot((1, 0.2, -0.4), -30) @ sc(1.0, 0.7, 1.3), tr(2.3, 0.6, 0.2) @ rot((0.1, 1, 0.5), 75) @ sc(1.6, 0.5, 0.9)),
        (0, tr(0, -2, 0) @ rot((0, 0, 1), 10), tr(0.2, -2, 0) @ rot((0, 0, 1), 13)),
        (1, tr(0, 2, 0) @ rot((1, 1, 0), 35), None)]
CENTRES = np.array([[-2, 0.5, 0.25], [0, 0, 0], [2.15, 0.3, 0.1], [0.1, -2, 0], [0, 2, 0]], dtype=np.float64)


MATERIALS = [(scenes.MAT_MATTE, (KD, KD, KD), (0, 0, 0), 1.0), (scenes.MAT_GLASS, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5),
             (scenes.MAT_MIRROR, (0.9, 0.9, 0.9), (0, 0, 0), 1.0)]


def make_scene(instances, world=None, lights=(), moving=True, objects=OBJECTS, instance_material=None):
    """A general two-level scene of `objects`. instances: (object, m0, m1 or None). moving=False: no "instance_motion" entry at all
    (pbrt_hip_scene_create_two_level), every instance at m0. One object and no world triangles: the traversal kernels' INST = 1
    builds; otherwise INST = 2."""
    n = len(instances)
    inst = np.zeros((n, 2, 4, 4), dtype=np.float32)
    motion = {}
    for i, (_, m0, m1) in enumerate(instances):
        inst[i, 0] = np.asarray(m0, dtype=np.float32)
        inst[i, 1] = np.linalg.inv(f32(m0)).astype(np.float32)
        if m1 is not None:
            motion[i] = scenes.instance_motion(m1, T0, T1)
    inst[:, :, 3, :] = (0, 0, 0, 1)
    if world is None:
        world = dict(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.int32), tri_material=np.zeros(0, np.int32),
                     tri_light=np.zeros(0, np.int32))
    out = dict(objects=[dict(positions=p, indices=i, tri_material=np.zeros(len(i), np.int32)) for p, i in objects], instances=inst,
               instance_object=np.array([k for k, _, _ in instances], dtype=np.int32), instance_material=np.full(n, -1, np.int32) if instance_material is None else np.asarray(instance_material, dtype=np.int32),
               world=world, materials=scenes._materials(MATERIALS), lights=scenes._lights(list(lights)))
    if moving:
        out["instance_motion"] = motion
    return out


def model_instances(instances, objects=OBJECTS, t0=T0, t1=T1):
    return [(mm.Motion(f32(m0), None if m1 is None else f32(m1), t0, t1), *objects[k]) for k, m0, m1 in instances]


def rays_at(centres, seed, times, spread=0.6, radius=6.0):
    """N_RAYS rays from a sphere of `radius` towards points around the centres, each at one of `times`; no zero direction component"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(N_RAYS, 3))
    o = radius * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = centres[rng.integers(0, len(centres), N_RAYS)] + rng.uniform(-spread, spread, size=(N_RAYS, 3))
    rays = np.zeros(N_RAYS, dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"] = o, target - o
    rays["t_max"] = np.inf
    rays["time"] = np.asarray(times, dtype=np.float32)[rng.integers(0, len(times), N_RAYS)]
    assert np.all(rays["d"] != 0)
    return rays


def some_times(seed):
    """8 times: six inside (T0, T1), one before the start, one after the end"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(T0, T1, 6), [T0 - 0.4, T1 + 0.3]]).astype(np.float32)


def model_hits(instances, rays, objects=OBJECTS):
    return mm.closest_hits(model_instances(instances, objects), rays["o"], rays["d"], rays["t_max"], rays["time"].astype(np.float64))


def check_ids(name, hits, m):
    keep = ~m["unsure"]
    print(f"{name}: {m['hit'].sum()} model hits, {(~keep).sum()} of {len(keep)} rays excluded")
    assert 1.0 - keep.mean() <= 0.02, name
    assert np.array_equal((hits["prim_id"] >= 0)[keep], m["hit"][keep]), name
    assert np.array_equal(hits["prim_id"][keep], m["prim"][keep]), name
    assert np.array_equal(hits["instance_id"][keep], m["inst"][keep]), name
    sel = keep & m["hit"]
    return sel, np.abs(hits["t"][sel].astype(np.float64) - m["t"][sel]) / m["t"][sel]


FLOOR = dict(positions=np.array([[-6, -6, -3], [6, -6, -3], [6, 6, -3], [-6, 6, -3]], dtype=np.float32),
             indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
SUN = (scenes.distant_light((0.2, 0.3, 1.0), (LIGHT_L, LIGHT_L, LIGHT_L)),)

# the tolerance of tests/test_gpu_shapes.py's Lambert test: N_FACTOR * NORMAL_PROBE_SPHERE_PATH_WORST * cond_2 of the transform's
# linear part, which is 1 for a rotation
NORMAL_TOL = 4.0 * 4.9379e-05

RES, SPP = 64, 64
BLUR_START, BLUR_SHIFT = (-0.73, 0.02, 0.0), 1.5


def blur_scene():
    x, y, z = BLUR_START
    scene = make_scene([(0, tr(x, y, z), tr(x + BLUR_SHIFT, y, z))], lights=(scenes.distant_light((0, 0, 1.0), (LIGHT_L, LIGHT_L, LIGHT_L)),),
                       objects=(QUAD,))
    scene["instance_motion"] = {0: scenes.instance_motion(tr(x + BLUR_SHIFT, y, z), 0.0, 1.0)}
    return scene


# ---------------------------------------------------------------------------------------------------------------------
# shared by the new cases
# ---------------------------------------------------------------------------------------------------------------------
EDGE = 1e-3
MAX_EXCLUDED = 0.02
FAR = 12.0


def with_far_triangles(world, far=FAR):
    """`world` plus two small triangles far out at opposite corners: every scene that holds them has the same world bound,
    wherever its instances stand inside it"""
    f = np.float32(far)
    pts = np.array([[-f, -f, -f], [-f, 0.1 - f, -f], [0.1 - f, -f, -f], [f, f, f], [f, f - 0.1, f], [f - 0.1, f, f]], dtype=np.float32)
    n = len(world["positions"])
    return dict(positions=np.concatenate([world["positions"], pts]).astype(np.float32),
                indices=np.concatenate([world["indices"], [[n, n + 1, n + 2], [n + 3, n + 4, n + 5]]]).astype(np.int32),
                tri_material=np.concatenate([world["tri_material"], [0, 0]]).astype(np.int32),
                tri_light=np.concatenate([world["tri_light"], [-1, -1]]).astype(np.int32))


def frozen(instances, objects, time):
    """the instances as static ones at the model's matrices of `time` (rounded to float by make_scene)"""
    return [(k, mo.interpolate(np.float64(time)), None) for (k, _, _), (mo, _, _) in zip(instances, model_instances(instances, objects))]


def static_at(scene, which):
    """`scene` (of make_scene) with every animated instance's rows replaced by its END matrix and that matrix's inverse, computed
    in double and rounded once, -0 written as +0 as the library stores it (`which` = "end"); "start": the scene as it is. No
    "instance_motion" entry either way: the old creation call."""
    out = {k: v for k, v in scene.items() if k != "instance_motion"}
    if which == "start":
        return out
    inst = scene["instances"].copy()
    for i, rec in scene["instance_motion"].items():
        m = rec["end_to_world"].astype(np.float64).reshape(4, 4)
        inst[i, 0] = m.astype(np.float32)
        inst[i, 1] = (np.linalg.inv(m) + 0.0).astype(np.float32)
    inst[:, :, 3, :] = (0, 0, 0, 1)
    out["instances"] = inst
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. time stays with its path
# ---------------------------------------------------------------------------------------------------------------------
# Horizontal rectangles (x0, x1, y0, y1, z, faces up?, material row, Le): all the light comes from the two emitters, seen
# through specular chains; every surface that is not specular is black (Kd = 0), so a path adds nothing but exact zeros at or
# after a matte hit, wherever that hit lies.
PATH_MATERIALS = [(scenes.MAT_MATTE, (0.0, 0.0, 0.0), (0, 0, 0), 1.0), (scenes.MAT_MIRROR, (0.9, 0.9, 0.9), (0, 0, 0), 1.0),
                  (scenes.MAT_GLASS, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5)]
GLASS_ETA = 1.5
PATH_RECTS = dict(floor_mirror=(-4.0, 4.0, -3.0, 0.9, 0.0, True, 1, None),
                  low_mirror=(-4.0, 4.0, -0.9, 0.1, 2.5, False, 1, None),
                  pane=(-4.0, 4.0, 1.2, 2.8, 1.5, False, 2, None),
                  emitter=(-5.0, 5.0, -4.0, 4.0, 4.0, False, 0, (5.0, 4.0, 3.0)),
                  second_emitter=(-3.5, 3.5, 1.1, 2.9, 0.2, True, 0, (0.5, 1.0, 1.5)))
OCC_Z, OCC_SIZE = 3.0, (1.2, 7.0)
OCC_X0, OCC_X1 = -1.0, 1.0
OCCLUDER = [(0, tr(OCC_X0, 0, OCC_Z) @ sc(OCC_SIZE[0], OCC_SIZE[1], 1), tr(OCC_X1, 0, OCC_Z) @ sc(OCC_SIZE[0], OCC_SIZE[1], 1))]
# the static scenes: the same quad, large enough to cover every chain / out of every chain's way
OCCLUDER_COVERS = [(0, tr(0, 0, OCC_Z) @ sc(9.0, 7.0, 1), None)]
OCCLUDER_AWAY = [(0, tr(9.0, 0, OCC_Z) @ sc(OCC_SIZE[0], OCC_SIZE[1], 1), None)]
CLASSES = ("miss", "mirror", "two_mirrors", "pane")
MIN_SWITCHED = 100


def _rect_world(rects):
    pos, idx, mat, light, lights = [], [], [], [], []
    for x0, x1, y0, y1, z, up, m, le in rects:
        corners = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]     # counter-clockwise from above: the normal is +z
        if not up:
            corners = corners[::-1]
        base = len(pos)
        pos += corners
        for tri in ((0, 1, 2), (0, 2, 3)):
            if le is not None:
                light.append(len(lights))
                lights.append((scenes.LIGHT_DIFFUSE_AREA, le, len(idx), 0, 1))
            else:
                light.append(-1)
            idx.append([base + tri[0], base + tri[1], base + tri[2]])
            mat.append(m)
    world = dict(positions=np.asarray(pos, dtype=np.float32), indices=np.asarray(idx, dtype=np.int32),
                 tri_material=np.asarray(mat, dtype=np.int32), tri_light=np.asarray(light, dtype=np.int32))
    return world, lights


def path_time_scene(instances, moving):
    world, lights = _rect_world(PATH_RECTS.values())
    scene = make_scene(instances, world=with_far_triangles(world), lights=lights, moving=moving, objects=(QUAD,))
    scene["materials"] = scenes._materials(PATH_MATERIALS)
    return scene


def path_time_rays(seed=31):
    """N_RAYS rays of the four classes in random order, over some_times(seed + 1). Returns (rays, class index per ray)."""
    rng = np.random.default_rng(seed)
    times = some_times(seed + 1)
    cls = rng.choice(4, size=N_RAYS, p=[0.07, 0.31, 0.31, 0.31])
    n = N_RAYS
    x_cross = rng.uniform(-2.0, 2.0, n)                          # about where the chain passes the occluder's plane
    dx = rng.uniform(0.05, 0.25, n) * rng.choice([-1.0, 1.0], n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    # miss: from above the emitter, upwards
    s = cls == 0
    o[s] = np.column_stack([x_cross[s], rng.uniform(-3, 3, s.sum()), np.full(s.sum(), 5.0)])
    d[s] = np.column_stack([dx[s], rng.uniform(0.02, 0.08, s.sum()), np.ones(s.sum())])
    # mirror: down from z = 2 on the floor mirror, up past the occluder's plane (5 units of z)
    s = cls == 1
    o[s] = np.column_stack([x_cross[s] - 5.0 * dx[s], rng.uniform(-2.9, -2.0, s.sum()), np.full(s.sum(), 2.0)])
    d[s] = np.column_stack([dx[s], rng.uniform(0.02, 0.08, s.sum()), -np.ones(s.sum())])
    # two mirrors: up from z = 1 on the low mirror (faces down), down on the floor mirror, up beside the low mirror (7 units)
    s = cls == 2
    o[s] = np.column_stack([x_cross[s] - 7.0 * dx[s], rng.uniform(-1.0, -0.3, s.sum()), np.full(s.sum(), 1.0)])
    d[s] = np.column_stack([dx[s], rng.uniform(0.19, 0.21, s.sum()), np.ones(s.sum())])
    # pane: up from z = 0.5 on the glass sheet at z = 1.5; reflected down on the second emitter, transmitted up (about 2 units)
    s = cls == 3
    o[s] = np.column_stack([x_cross[s] - 2.0 * dx[s], rng.uniform(1.5, 2.5, s.sum()), np.full(s.sum(), 0.5)])
    d[s] = np.column_stack([dx[s], rng.uniform(0.02, 0.08, s.sum()) * rng.choice([-1.0, 1.0], s.sum()), np.ones(s.sum())])
    # unit directions: the library hands wo = -d on as it is given at a world-space triangle (as the reference does), and a
    # specular lobe refracts by the cosine it reads off wo
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=scenes.RAY_DTYPE)
    rays["o"], rays["d"], rays["t_max"] = o, d, np.inf
    rays["time"] = times[rng.integers(0, len(times), n)]
    assert np.all(rays["d"] != 0)
    return rays, cls


def _occluder_crossing(motion, o, d, time):
    """Where the rays meet the occluder's plane at their own times: t (inf: never, or behind), inside the quad?, within EDGE of
    its edge? (world units: the instance is a translation of a scale)"""
    oo, od = mm._object_rays(motion, o, d, time)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -oo[:, 2] / od[:, 2]
    t = np.where(np.isfinite(t) & (t > 1e-9), t, np.inf)
    p = oo + od * np.where(np.isfinite(t), t, 0.0)[:, None]
    m = motion.interpolate(time)
    size = np.stack([m[:, 0, 0], m[:, 1, 1]], axis=1)
    out_by = (np.abs(p[:, :2]) - 0.5) * size                      # > 0: outside along that axis, by so much
    inside = np.all(out_by < 0.0, axis=1) & np.isfinite(t)
    near = np.all(out_by < EDGE, axis=1) & ~np.all(out_by < -EDGE, axis=1) & np.isfinite(t)
    return t, inside, near


def trace_chain(o, d, time, occluder=None, pane_branch="transmit", max_hits=6):
    """The specular chain of every ray in float64: the closest of the rectangles and the occluder (a mm.Motion of QUAD, None:
    left out) at the ray's time; a mirror reflects, the pane refracts (`transmit`, eta 1.5, entering from the side its normal
    faces) or reflects. Returns (hits: list per ray of surface names, near: the chain passed within EDGE of the occluder's edge)."""
    o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    time = np.asarray(time, dtype=np.float64)
    n = len(o)
    names = list(PATH_RECTS)
    hits = [[] for _ in range(n)]
    near_any = np.zeros(n, bool)
    alive = np.ones(n, bool)
    for _ in range(max_hits):
        best_t, best = np.full(n, np.inf), np.full(n, -1)
        for k, (x0, x1, y0, y1, z, _, _, _) in enumerate(PATH_RECTS.values()):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (z - o[:, 2]) / d[:, 2]
            p = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
            ok = np.isfinite(t) & (t > 1e-9) & (p[:, 0] > x0) & (p[:, 0] < x1) & (p[:, 1] > y0) & (p[:, 1] < y1) & (t < best_t)
            best_t, best = np.where(ok, t, best_t), np.where(ok, k, best)
        if occluder is not None:
            t, inside, near = _occluder_crossing(occluder, o, d, time)
            near_any |= alive & near & (t < best_t)
            ok = inside & (t < best_t)
            best_t, best = np.where(ok, t, best_t), np.where(ok, len(names), best)
        for i in np.flatnonzero(alive):
            hits[i].append("nothing" if best[i] < 0 else "occluder" if best[i] == len(names) else names[best[i]])
        kind = np.array([PATH_RECTS[names[b]][6] if 0 <= b < len(names) else 0 for b in best])
        go_on = alive & (best >= 0) & (best < len(names)) & (kind != 0)
        o = o + d * np.where(np.isfinite(best_t), best_t, 0.0)[:, None]
        refract = go_on & (kind == 2) & (pane_branch == "transmit")
        mirror = go_on & ~refract
        nd = d.copy()
        nd[mirror, 2] = -d[mirror, 2]
        if refract.any():
            up = np.array([PATH_RECTS[names[b]][5] if 0 <= b < len(names) else True for b in best])
            nz = np.where(up, 1.0, -1.0)                          # the geometric normal's z
            entering = d[:, 2] * nz < 0.0                         # wo = -d on the normal's side
            eta = np.where(entering, 1.0 / GLASS_ETA, GLASS_ETA)
            cos_i = np.abs(d[:, 2])
            sin2_t = eta ** 2 * (1.0 - cos_i ** 2)
            assert np.all(sin2_t[refract] < 1.0)                  # no total internal reflection in this scene
            cos_t = np.sqrt(np.clip(1.0 - sin2_t, 0.0, None))
            face_z = -np.sign(d[:, 2])                            # the normal turned against the ray
            rd = eta[:, None] * d
            rd[:, 2] += (eta * cos_i - cos_t) * face_z
            nd[refract] = rd[refract]
        d = nd / np.linalg.norm(nd, axis=1, keepdims=True)
        alive = go_on
    return hits, near_any


_PATH_CACHE = {}
CHAIN_PREFIX = {0: [], 1: ["floor_mirror"], 2: ["low_mirror", "floor_mirror"], 3: ["pane"]}


def path_time_case():
    """dict: rays, cls, moving / covers / away (scene dicts), covered (the model: the deciding chain ends on the occluder at the
    ray's own time), covered_at_start (... if the occluder stood at its start position), keep (not within EDGE of its edge),
    chains (the deciding chain's surface names), reflected (the pane's reflect branch)."""
    if "case" in _PATH_CACHE:
        return _PATH_CACHE["case"]
    rays, cls = path_time_rays()
    o, d, time = rays["o"].astype(np.float64), rays["d"].astype(np.float64), rays["time"].astype(np.float64)
    motion = model_instances(OCCLUDER, (QUAD,))[0][0]
    chains, near = trace_chain(o, d, time, motion)
    start_chains, start_near = trace_chain(o, d, np.full(len(o), T0), motion)
    reflected, _ = trace_chain(o, d, time, motion, pane_branch="reflect")
    case = dict(rays=rays, cls=cls, chains=chains, reflected=reflected, keep=~near, keep_at_start=~start_near,
                covered=np.array([c[-1] == "occluder" for c in chains]), covered_at_start=np.array([c[-1] == "occluder" for c in start_chains]),
                moving=path_time_scene(OCCLUDER, True), covers=path_time_scene(OCCLUDER_COVERS, False), away=path_time_scene(OCCLUDER_AWAY, False))
    _PATH_CACHE["case"] = case
    return case


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows under scale and shear at the shaded hit
# ---------------------------------------------------------------------------------------------------------------------
def shear(xy, xz, yz):
    m = np.eye(4)
    m[0, 1], m[0, 2], m[1, 2] = xy, xz, yz
    return m


# a box like FIVE[2]; a quad with rotation about different axes, translation and changing non-uniform scale; a box whose shear
# changes. The first two are turned before they are scaled: under a scale along an object's own axes a face normal of the box
# (or the quad's) keeps its direction whether it goes through M or through (M^-1)^T, and only the shear would tell the two apart.
# 4 units apart: none shadows another from ROW_WI or ROW_LIGHT_P (aniso_case checks it on the model).
_TURN_A, _TURN_B = rot((1, 1, 0.3), 40), rot((0.4, -1, 1), 55)
ROW_INSTANCES = [(1, tr(-4, 0, 0) @ rot((1, 0.2, -0.4), -30) @ sc(1.0, 0.7, 1.3) @ _TURN_A,
                  tr(-3.7, 0.6, 0.2) @ rot((0.1, 1, 0.5), 75) @ sc(1.6, 0.5, 0.9) @ _TURN_A),
                 (0, tr(0, 0, 0) @ rot((0.2, 1, 0.1), 25) @ sc(1.4, 0.8, 1.0) @ _TURN_B,
                  tr(0.3, -0.4, 0.3) @ rot((1, 0.3, 0.2), -50) @ sc(0.9, 1.7, 0.6) @ _TURN_B),
                 (1, tr(4, 0, 0) @ rot((0.3, -0.2, 1), 15) @ shear(0.1, 0.0, 0.2) @ sc(1.2, 1.0, 0.8),
                  tr(4.2, 0.3, -0.2) @ rot((0.5, 1, -0.3), 80) @ shear(0.6, -0.3, 0.1) @ sc(0.8, 1.3, 1.1))]
ROW_CENTRES = np.array([[-3.85, 0.3, 0.1], [0.15, -0.2, 0.15], [4.1, 0.15, -0.1]])
ROW_WI = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
ROW_LIGHT_P = np.array([1.0, -6.0, 5.0])
ROW_LIGHT_I = np.array([40.0, 60.0, 80.0])
AU, AV = 0.15, 0.6
DISNEY_DESC = scenes.disney((0.8, 0.5, 0.3), metallic=1.0, anisotropic=0.8, roughness=0.5)
ANISO_ROWS = {"metal": dict(model=mfm.Material.metal(ETA, K, AU, AV, remap=False), f=mfm.bsdf_f),
              "disney": dict(model=dm.Disney(DISNEY_DESC), f=dm.bsdf_f)}
ANISO_FLOOR = 1e-3
MIN_KEPT = 800
# worst relative error of the STATIC path (instances frozen at the model's matrices) against the model, as
# test_gpu_motion_paths.py::test_anisotropic_rows_under_scale_and_shear measured it on gfx950 (MI355X), with half as much again
# for another compiler's rounding: the
# sensitivity checks of test_motion_cases_model.py take 4 times these as the allowance, as the GPU test takes 4 times what it
# measures
ANISO_BASELINE_RECORDED = {"metal": 3.6e-6, "disney": 4.5e-6}   # 1.5 times the measured 2.364840e-06 and 2.961105e-06


def row_scene(instances, moving, lights, material=None):
    """ROW_INSTANCES (or frozen ones) under `lights`; material: None matte, "metal" / "disney": that row on every instance
    (scene["set_roughness"] = (row, u, v) is for Scene.set_material_roughness after creation)"""
    scene = make_scene(instances, lights=lights, moving=moving)
    if material == "metal":
        scene["materials"] = scenes._materials(MATERIALS + [scenes.metal(ETA, K, 0.01)])
        scene["instance_material"] = np.full(len(instances), 3, np.int32)
        scene["set_roughness"] = (3, AU, AV)
    elif material == "disney":
        scene["materials"] = scenes._materials(MATERIALS + [MATERIALS[0]])
        scene["instance_material"] = np.full(len(instances), 3, np.int32)
        scene["disney_descs"] = {3: DISNEY_DESC}
    return scene


def row_rays(seed=41):
    return rays_at(ROW_CENTRES, seed, some_times(seed + 1), spread=0.45)


def _per_time_frames(rays, m, variant="right"):
    """model frames at the model's hits (dict of (n, 3) arrays, zeros where the ray misses) and cond_2 of M(t)'s linear part"""
    n = len(rays)
    fr = {k: np.zeros((n, 3)) for k in ("n", "dpdu", "ss", "ts")}
    cond = np.ones(n)
    insts = model_instances(ROW_INSTANCES)
    for t in np.unique(rays["time"]):
        for i, (motion, pos, idx) in enumerate(insts):
            sel = m["hit"] & (rays["time"] == t) & (m["inst"] == i)
            if not sel.any():
                continue
            f = mm.shading_frames(motion, pos, idx, m["prim"][sel], t, variant)
            for k in fr:
                fr[k][sel] = f[k]
            cond[sel] = np.linalg.cond(motion.interpolate(np.float64(t))[:3, :3], 2)
    return fr, cond


def lambert_case(variant="right"):
    """dict: rays, m (model hits), expect (n,) = max(0, n . wi) with n turned towards the viewer, tol (n,) = NORMAL_TOL cond_2(M(t))"""
    rays = row_rays()
    m = model_hits(ROW_INSTANCES, rays)
    fr, cond = _per_time_frames(rays, m, variant)
    nrm = fr["n"]
    nrm = np.where(((nrm * -rays["d"].astype(np.float64)).sum(axis=1) < 0)[:, None], -nrm, nrm)
    return dict(rays=rays, m=m, expect=np.where(m["hit"], np.maximum(0.0, nrm @ ROW_WI), 0.0), tol=NORMAL_TOL * cond)


_ANISO_CACHE = {}


def aniso_case(name, variant="right"):
    """dict: rays, m, ref (n, 3) = f(wo, wi) I |n . wi| / r^2 in the model's frame at the model's hit, keep: the model hits, is
    sure of it, nothing stands between the point and the light, and ref's largest channel is at least ANISO_FLOOR"""
    if (name, variant) in _ANISO_CACHE:
        return _ANISO_CACHE[(name, variant)]
    if "shared" not in _ANISO_CACHE:
        rays = row_rays()
        m = model_hits(ROW_INSTANCES, rays)
        o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
        p = o + d * np.where(m["hit"], m["t"], 1.0)[:, None]
        to_light = ROW_LIGHT_P - p
        # anything between the point and the light, from a little way off the surface (the own, convex, body cannot be)
        sh = mm.closest_hits(model_instances(ROW_INSTANCES), p + 1e-4 * to_light, to_light, np.full(len(p), 1.0 - 2e-4), rays["time"].astype(np.float64))
        _ANISO_CACHE["shared"] = (rays, m, p, to_light, sh["hit"] | sh["unsure"])
    rays, m, p, to_light, blocked = _ANISO_CACHE["shared"]
    fr, _ = _per_time_frames(rays, m, variant)
    r2 = (to_light ** 2).sum(axis=1)
    wi = to_light / np.sqrt(r2)[:, None]
    wo = -rays["d"].astype(np.float64)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    hit = m["hit"]
    wo_l, wi_l = mm.to_local(fr, wo), mm.to_local(fr, wi)
    row = ANISO_ROWS[name]
    ref = np.zeros((len(rays), 3))
    with np.errstate(all="ignore"):
        ref[hit] = row["f"](row["model"], wo_l[hit], wi_l[hit]) * ROW_LIGHT_I * (np.abs(wi_l[hit, 2]) / r2[hit])[:, None]
    ref = np.where(np.isfinite(ref), ref, 0.0)
    keep = hit & ~m["unsure"] & ~blocked & (ref.max(axis=1) >= ANISO_FLOOR)
    out = dict(rays=rays, m=m, ref=ref, keep=keep)
    _ANISO_CACHE[(name, variant)] = out
    return out


def aniso_error(got, ref, keep):
    """per kept ray: the largest |got - ref| / ref over the channels at or above the floor"""
    sel = ref[keep] >= ANISO_FLOOR
    rel = np.where(sel, np.abs(np.asarray(got, np.float64)[keep] - ref[keep]) / np.where(sel, ref[keep], 1.0), 0.0)
    return rel.max(axis=1)


# the shadow of the scaled moving box on a static plane: the box turns about z, so its underside stays parallel to the plane just
# below it
STAND_BOX = [(1, tr(-0.8, 0, 0) @ rot((0, 0, 1), 10) @ sc(1.0, 0.7, 1.3), tr(0.8, 0.3, 0) @ rot((0, 0, 1), 70) @ sc(1.6, 0.5, 0.9))]
STAND_Z = -0.33
STAND_WI = np.array([1.0, 0.4, 0.6]) / np.linalg.norm([1.0, 0.4, 0.6])   # a low sun: the shadow reaches well beyond the box


def stand_scene():
    plane = dict(FLOOR, positions=(FLOOR["positions"] * np.float32([1, 1, 0]) + np.float32([0, 0, STAND_Z])).astype(np.float32))
    return make_scene(STAND_BOX, world=plane, lights=(scenes.distant_light(STAND_WI, (LIGHT_L, LIGHT_L, LIGHT_L)),))


def shadow_start_case(seed=51):
    """dict: rays (straight-ish down on the plane and the box), on_plane / on_box (the model's first hit), dark (on_plane: the
    ray from the point towards the light meets the box at the ray's time), lambert (on_box: max(0, n . wi) towards the viewer),
    tol (on_box), keep (the model is sure of both the first hit and the shadow ray)"""
    rng = np.random.default_rng(seed)
    times = some_times(seed + 1)
    rays = np.zeros(N_RAYS, dtype=scenes.RAY_DTYPE)
    rays["o"] = np.column_stack([rng.uniform(-2.2, 1.2, N_RAYS), rng.uniform(-1.1, 0.9, N_RAYS), np.full(N_RAYS, 2.0)])
    rays["d"] = (0.1, 0.05, -1.0)
    rays["t_max"] = np.inf
    rays["time"] = times[rng.integers(0, len(times), N_RAYS)]
    o, d, time = rays["o"].astype(np.float64), rays["d"].astype(np.float64), rays["time"].astype(np.float64)
    insts = model_instances(STAND_BOX)
    m = mm.closest_hits(insts, o, d, rays["t_max"], time)
    t_plane = (STAND_Z - o[:, 2]) / d[:, 2]
    on_box = m["hit"] & (m["t"] < t_plane)
    on_plane = ~on_box
    p = o + d * t_plane[:, None]
    sh = mm.closest_hits(insts, p, np.broadcast_to(STAND_WI, p.shape), np.full(N_RAYS, np.inf), time)
    motion, pos, idx = insts[0]
    lambert, tol = np.zeros(N_RAYS), np.zeros(N_RAYS)
    for t in np.unique(rays["time"]):
        sel = on_box & (rays["time"] == t)
        f = mm.shading_frames(motion, pos, idx, m["prim"][sel], t)
        nrm = np.where(((f["n"] * -d[sel]).sum(axis=1) < 0)[:, None], -f["n"], f["n"])
        lambert[sel] = np.maximum(0.0, nrm @ STAND_WI)
        tol[sel] = NORMAL_TOL * np.linalg.cond(motion.interpolate(np.float64(t))[:3, :3], 2)
    # a ray that passes the box within the model's margin is unsure of its first hit; on the plane the shadow ray decides
    keep = ~m["unsure"] & ~(on_plane & sh["unsure"]) & ~(m["hit"] & (np.abs(m["t"] - t_plane) < 1e-3))
    return dict(rays=rays, on_box=on_box, on_plane=on_plane, dark=on_plane & sh["hit"], lambert=lambert, tol=tol, keep=keep)


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth, counting and the bound
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("negated", "nlerp", "scaled", "static", "general")
MIN_KIND_HITS = 50


def quat_dot(m0, m1):
    """r0 . r1 of the two decompositions, before AnimatedTransform::new negates r1"""
    return float(np.dot(mm.decompose(f32(m0))[1], mm.decompose(f32(m1))[1]))


def depth_instances(n_objects, seed=61):
    """64 instances from a seeded generator, their centres within 1.5 of the origin so that the boxes overlap. Eight whose
    quaternions have r0 . r1 < 0 (a turn of 200 to 300 degrees), eight on slerp's normalised-lerp branch (1.5 to 3 degrees),
    eight with changing non-uniform scale, eight static, 32 with a turn of up to 170 degrees; all but the static ones are
    translated as well. n_objects = 2: quad and box in turn; 1: object 0 throughout. Returns (instances, kind per instance)."""
    rng = np.random.default_rng(seed)

    def axis():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    def base():
        return tr(*rng.uniform(-1.5, 1.5, 3)) @ rot(axis(), rng.uniform(0.0, 360.0))

    def shift():
        return tr(*rng.uniform(-0.5, 0.5, 3))

    kinds = list(rng.permutation(np.repeat(np.arange(5), [8, 8, 8, 8, 32])))
    out = []
    for i, kind in enumerate(kinds):
        k = i % n_objects
        b = base()
        if kind == 0:
            while True:
                m1 = shift() @ b @ rot(axis(), rng.uniform(200.0, 300.0))
                if quat_dot(b, m1) < -0.05:
                    break
            out.append((k, b, m1))
        elif kind == 1:
            out.append((k, b, shift() @ b @ rot(axis(), rng.uniform(1.5, 3.0))))
        elif kind == 2:
            s0, s1 = (rng.permutation([rng.uniform(0.6, 0.8), rng.uniform(0.9, 1.1), rng.uniform(1.3, 1.6)]) for _ in range(2))
            out.append((k, b @ sc(*s0), shift() @ b @ rot(axis(), rng.uniform(10.0, 120.0)) @ sc(*s1)))
        elif kind == 3:
            out.append((k, b, None))
        else:
            out.append((k, b, shift() @ b @ rot(axis(), rng.uniform(5.0, 170.0))))
    return out, np.array(kinds)


DEPTH_OBJECTS = {2: OBJECTS, 1: (BOX,)}
NO_WORLD = dict(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.int32), tri_material=np.zeros(0, np.int32),
                tri_light=np.zeros(0, np.int32))
_DEPTH_CACHE = {}


def depth_case(n_objects):
    """dict: instances, kinds, objects, world (the two-object scene: two small triangles far out, which no ray meets, make it a
    scene with world triangles, the kernels' INST = 2; None: INST = 1), times, rays, m (mm.closest_hits: brute force over all
    triangles)"""
    if n_objects not in _DEPTH_CACHE:
        instances, kinds = depth_instances(n_objects, seed=61 + n_objects)
        objects = DEPTH_OBJECTS[n_objects]
        times = some_times(70 + n_objects)
        mid = np.array([mo.interpolate(np.float64(0.5 * (T0 + T1)))[:3, 3] for mo, _, _ in model_instances(instances, objects)])
        rays = rays_at(mid, 80 + n_objects, times, spread=0.4)
        _DEPTH_CACHE[n_objects] = dict(instances=instances, kinds=kinds, objects=objects, world=with_far_triangles(NO_WORLD) if n_objects == 2 else None,
                                       times=times, rays=rays, m=model_hits(instances, rays, objects))
    return _DEPTH_CACHE[n_objects]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the ends of the range
# ---------------------------------------------------------------------------------------------------------------------
def end_times():
    """exactly T0 and T1 (as the float the library holds) and their neighbours on both sides"""
    a, b = np.float32(T0), np.float32(T1)
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    return np.array([np.nextafter(a, lo), a, np.nextafter(a, hi), np.nextafter(b, lo), b, np.nextafter(b, hi)], dtype=np.float32)


END_MATERIAL = [1, -1, 2, -1, -1]   # of FIVE: a glass quad, a matte box, a mirror box, a matte quad, a matte box


def end_scene(which):
    """FIVE over the floor under the sun and a dim sky, with the far triangles: "moving", or static at the "start" / "end" rows"""
    lights = SUN + ((scenes.LIGHT_INFINITE, (0.2, 0.25, 0.3), -1, 0, 1),)
    scene = make_scene(FIVE, world=with_far_triangles(FLOOR), lights=lights, instance_material=END_MATERIAL)
    return scene if which == "moving" else static_at(scene, which)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Halton sampler's time dimension
# ---------------------------------------------------------------------------------------------------------------------
def scrambled_radical_inverse(base, perm, i):
    """ScrambledRadicalInverse in float64: the digits of i, least significant first, each through `perm`, mirrored about the
    radix point; the endless zeros after them contribute perm[0] each (lowdiscrepancy.rs, pbrt-v3 ScrambledRadicalInverseSpecialized)"""
    i = np.asarray(i, dtype=np.int64).copy()
    perm = np.asarray(perm)
    out, scale = np.zeros(i.shape, dtype=np.float64), np.ones(i.shape, dtype=np.float64)
    while np.any(i > 0):
        more = i > 0
        scale = np.where(more, scale / base, scale)
        out += np.where(more, perm[i % base] * scale, 0.0)
        i //= base
    return out + perm[0] * scale / (base - 1)


def halton_time_permutation(idx, u):
    """The digit permutations of base 5 (the sampler's third dimension) under which the scrambled radical inverse of the sample
    indices `idx` is `u` to 2e-7: the list of those that fit (exactly one for a right sampler)"""
    return [p for p in itertools.permutations(range(5))
            if np.abs(scrambled_radical_inverse(5, p, idx) - u).max() <= 2e-7]


# ---------------------------------------------------------------------------------------------------------------------
# 6. material levels through the moving builds
# ---------------------------------------------------------------------------------------------------------------------
LEVEL_ROWS = MATERIALS + [scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2), scenes.metal(ETA, K, 0.1), MATERIALS[0], MATERIALS[0], MATERIALS[0]]
LEVEL_DESCS = {5: scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.4), 0.15, 0.4), 6: scenes.rough_glass((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5, 0.2, 0.1)}
LEVEL_DISNEY = {7: scenes.disney((0.8, 0.5, 0.3), metallic=0.3, anisotropic=0.5, roughness=0.4, sheen=0.5, clearcoat=0.5)}


def level_scenes(level):
    """(old, new): FIVE, all static, over the floor under the sun and a dim sky, through pbrt_hip_scene_create_two_level and
    through pbrt_hip_scene_create_two_level_moving. Level 1 adds a plastic and a metal row, 2 a substrate and a rough-glass
    descriptor, 3 a Disney row, each on instances of their own and the newest on the floor as well."""
    static = [(k, m0, None) for k, m0, _ in FIVE]
    rows = {1: [3, 4, 2, 3, 1], 2: [3, 5, 6, 4, 5], 3: [7, 5, 6, 4, 3]}[level]
    floor = dict(FLOOR, tri_material=np.full(2, {1: 3, 2: 5, 3: 7}[level], np.int32))
    lights = SUN + ((scenes.LIGHT_INFINITE, (0.2, 0.25, 0.3), -1, 0, 1),)
    out = []
    for moving in (False, True):
        scene = make_scene(static, world=floor, lights=lights, moving=moving, instance_material=rows)
        scene["materials"] = scenes._materials(LEVEL_ROWS)
        if level >= 2:
            scene["material_descs"] = dict(LEVEL_DESCS)
        if level >= 3:
            scene["disney_descs"] = dict(LEVEL_DISNEY)
        out.append(scene)
    return tuple(out)
