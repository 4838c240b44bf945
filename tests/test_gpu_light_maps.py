"""ProjectionLight and GonioPhotometricLight on the device (PBRT_LIGHT_PROJECTION / PBRT_LIGHT_GONIOMETRIC):
Light::sample_li pinned to the float64 model (light_map_model.py) through pbrt_hip_light_sample_li, the closed form of a matte
plane through the three integrators and on the other scene kinds, a map-less goniometric light against the point light it is,
the power and spatial light distributions, and a setter and a creation that refuse without changing anything."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import light_map_model as lm

pytestmark = pytest.mark.gpu

KD = np.array([0.5, 0.4, 0.3])
I = np.array([2.0, 3.0, 4.0])
P_LIGHT = (0.3, -0.2, 1.5)
FOV = 60.0
DOWN = lm.rigid((1.0, 0.0, 0.0), 180.0, P_LIGHT)          # light-space +z looks down at the plane z = 0
TILTED = lm.rigid((1.0, 0.15, -0.1), 168.0, P_LIGHT)
PROJ_MAP = lm.gentle_map(3, 5)   # 5 wide x 3 high: resampled to 8 x 4 on the way to the device, aspect > 1
GONIO_MAP = lm.gentle_map(4, 8)  # 8 x 4
MATTE = (scenes.MAT_MATTE, tuple(KD), (0, 0, 0), 1.0)
INTEGRATORS = [pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED]


def _light(kind, l2w, intensity=I):
    return scenes.projection_light(l2w, intensity, FOV) if kind == lm.PROJECTION else scenes.goniometric_light(l2w, intensity)


def _map_of(kind):
    return PROJ_MAP if kind == lm.PROJECTION else GONIO_MAP


def _plane_scene(lights, light_maps=None, half=10.0):
    positions, indices = scenes._plane_z0(half)
    sc = dict(positions=positions, indices=indices, tri_material=np.zeros(2, dtype=np.int32), materials=scenes._materials([MATTE]),
              tri_light=np.full(2, -1, dtype=np.int32), lights=scenes._lights(list(lights)))
    if light_maps:
        sc["light_maps"] = light_maps
    return sc


def _plane_rays(n_side=9, o=(0.1, 0.2, 3.0)):
    o = np.asarray(o, np.float64)
    xs = np.linspace(-2.5, 2.5, n_side)
    pts = np.array([(x, y, 0.0) for x in xs for y in xs])
    d = pts - o
    rays = np.zeros(len(d), dtype=scenes.RAY_DTYPE)
    rays["o"] = o.astype(np.float32)
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["t_max"] = np.inf
    return rays


def _hit_points(rays):
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    return o + (-o[:, 2] / d[:, 2])[:, None] * d


def _assert_margins(model, p):
    """every point is away from the model's discontinuities (float64, from the float32 points the device gets)"""
    wi, _, _ = model.sample_li(p)
    if model.kind == lm.GONIOMETRIC:
        wl = -wi @ model.w2l.T
        wl /= np.linalg.norm(wl, axis=1, keepdims=True)
        assert np.all(np.arctan2(np.hypot(wl[:, 0], wl[:, 2]), np.abs(wl[:, 1])) > 1e-3)  # off the light-space +-y axis
        return
    wl, q = model.screen_point(-wi)
    assert np.all(np.abs(wl[:, 2] - lm.HITHER) > 1e-4)
    front = wl[:, 2] > lm.HITHER
    sb = model.sb
    inside = np.minimum.reduce([q[:, 0] - sb[0], sb[2] - q[:, 0], q[:, 1] - sb[1], sb[3] - q[:, 1]])  # > 0 inside the window
    assert np.all(np.abs(inside[front]) >= 1e-3)


def _plane_closed_form(model, p, n=(0.0, 0.0, 1.0)):
    """Li = Kd / pi * I * map(-wi) * |cos theta| / r^2 from the hit points p of a matte plane with normal n"""
    wi, _, li = model.sample_li(p)
    return KD / np.pi * li * np.abs(wi @ np.asarray(n))[:, None]


# ---- 1. the query against the model ----
def _projection_points(model, n, seed):
    """wl = (px z / inv_tan, py z / inv_tan, z) projects to (px, py): a quarter well inside the window, a quarter outside it, a
    quarter behind the projector on lines that would project inside, a quarter in front but grazing (far outside the window)"""
    rng = np.random.default_rng(seed)
    k = n // 4
    x0, y0, x1, y1 = model.sb
    m = 2e-3
    inside = np.stack([x0 + m + rng.random(2 * k) * (x1 - x0 - 2 * m), y0 + m + rng.random(2 * k) * (y1 - y0 - 2 * m)], axis=1)
    out_x = np.stack([(x1 + m + rng.random(k // 2) * 1.5) * rng.choice([-1.0, 1.0], k // 2), (rng.random(k // 2) * 2 - 1) * 1.5 * y1], axis=1)
    out_y = np.stack([(rng.random(k - k // 2) * 2 - 1) * 1.5 * x1, (y1 + m + rng.random(k - k // 2) * 1.5) * rng.choice([-1.0, 1.0], k - k // 2)], axis=1)
    q = np.concatenate([inside[:k], out_x, out_y, inside[k:]])
    z = 0.5 + 2.5 * rng.random(len(q))
    z[3 * k - k:3 * k] *= -1.0  # the second `inside` quarter: behind
    wl = np.concatenate([q * (z / model.inv_tan)[:, None], z[:, None]], axis=1)
    c = (3e-3 + 0.02 * rng.random(n - len(q)))  # grazing: the unit direction's z just above hither
    phi = rng.random(len(c)) * 2 * np.pi
    graze = np.stack([np.sqrt(1 - c * c) * np.cos(phi), np.sqrt(1 - c * c) * np.sin(phi), c], axis=1) * (0.5 + rng.random(len(c)))[:, None]
    return np.concatenate([wl, graze])


def _gonio_points(n, seed):
    rng = np.random.default_rng(seed)
    theta = np.arccos(rng.random(n) * 2 - 1)
    theta[:64] = np.linspace(2e-3, 2e-2, 64)           # next to light-space +y
    theta[64:128] = np.pi - np.linspace(2e-3, 2e-2, 64)  # ... and -y
    theta = np.clip(theta, 2e-3, np.pi - 2e-3)
    phi = rng.random(n) * 2 * np.pi
    phi[128:160] = np.linspace(-1e-4, 1e-4, 32) % (2 * np.pi)  # across the seam
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=1)  # theta from +y, phi from +x to +z
    return d * (0.5 + 2.5 * rng.random(n))[:, None]


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "no-map"])
@pytest.mark.parametrize("l2w", [None, TILTED], ids=["identity", "rotated"])
@pytest.mark.parametrize("kind", [lm.PROJECTION, lm.GONIOMETRIC], ids=["projection", "goniometric"])
def test_sample_li_matches_model(hip_ctx, kind, l2w, with_map):
    n = 4096
    rgb = _map_of(kind) if with_map else None
    model = lm.LightMapModel(kind, l2w, I, FOV, rgb)
    p_point, p_spot = np.array([0.5, 0.25, 2.0]), np.array([-1.0, 0.5, 2.5])
    spot = scenes.spot_light(p_spot, (0.0, 0.0, 0.0), (5.0, 6.0, 7.0), 30.0, 20.0)
    scene = pbrt_hip.Scene(hip_ctx, _plane_scene([_light(kind, l2w), scenes.point_light(p_point, (3.0, 2.0, 1.0)), spot],
                                                 {0: rgb} if with_map else None))
    wl = _projection_points(model, n, 5) if kind == lm.PROJECTION else _gonio_points(n, 6)
    p = (model.p_light + wl @ np.linalg.inv(model.w2l).T).astype(np.float32)
    assert len(p) == n
    _assert_margins(model, p)
    wi, pdf, li = scene.light_sample_li(0, p)
    wi_ref, _, li_ref = model.sample_li(p)
    dark = ~li_ref.any(axis=1)
    print(f"li worst rel {np.abs(li[~dark] / li_ref[~dark] - 1).max():.3g}, wi worst abs {np.abs(wi - wi_ref).max():.3g}")
    # wi is a unit vector: 1e-4 of its length on every component
    assert np.abs(wi - wi_ref).max() <= 1e-4
    assert np.all(pdf == 1.0)
    if kind == lm.PROJECTION:
        assert n // 4 <= (~dark).sum() <= n // 4 + 8 and dark.sum() >= 3 * (n // 4) - 8
    else:
        assert not dark.any()
    assert np.all(li[dark] == 0.0)  # behind the projector, outside its window: exactly 0
    np.testing.assert_allclose(li[~dark], li_ref[~dark], rtol=1e-4)
    if not with_map:
        lit = np.broadcast_to(I, li_ref.shape)[~dark] / ((model.p_light - p.astype(np.float64)) ** 2).sum(axis=1)[~dark, None]
        np.testing.assert_allclose(li[~dark], lit, rtol=1e-6)  # a filtered 1 is not multiplied in: I / d^2
    # the probe on lights that were there before: the point light's and the spot light's closed forms
    q = (np.random.default_rng(9).random((512, 3)) * [4.0, 4.0, 1.5] - [2.0, 2.0, 0.0]).astype(np.float32)
    q64 = q.astype(np.float64)
    wi, pdf, li = scene.light_sample_li(1, q)
    d = p_point - q64
    np.testing.assert_allclose(li, np.array([3.0, 2.0, 1.0]) / (d * d).sum(axis=1, keepdims=True), rtol=1e-4)
    assert np.abs(wi - d / np.linalg.norm(d, axis=1, keepdims=True)).max() <= 1e-4 and np.all(pdf == 1.0)
    # spot: points at chosen angles from its axis: full cone, the falloff's middle, outside (SpotLight::falloff, spot.rs:49-62)
    axis = -p_spot / np.linalg.norm(p_spot)
    side = np.cross(axis, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    ang = np.radians(np.concatenate([np.linspace(0.0, 19.0, 32), np.linspace(21.0, 27.0, 32), np.linspace(31.0, 80.0, 32)]))
    q = (p_spot + (np.cos(ang)[:, None] * axis + np.sin(ang)[:, None] * side) * np.linspace(0.5, 2.0, 96)[:, None]).astype(np.float32)
    wi, pdf, li = scene.light_sample_li(2, q)
    d = p_spot - q.astype(np.float64)
    cos_t = -(d / np.linalg.norm(d, axis=1, keepdims=True)) @ axis
    ct, cf = np.cos(np.radians(30.0)), np.cos(np.radians(20.0))
    fall = np.where(cos_t < ct, 0.0, np.where(cos_t >= cf, 1.0, ((cos_t - ct) / (cf - ct)) ** 4))
    assert (fall == 0).sum() == 32 and (fall == 1).sum() == 32
    np.testing.assert_allclose(li, np.array([5.0, 6.0, 7.0]) * fall[:, None] / (d * d).sum(axis=1, keepdims=True), rtol=1e-4)
    scene.close()


# ---- 2. closed form through the integrators ----
def _li_plane(scene, integrator, rays):
    keys = np.arange(len(rays), dtype=np.uint64) * 7919 + 3
    rgb, _ = scene.li(rays, keys, integrator=integrator, max_depth=1, light_strategy=0)
    return rgb


def _check_plane(rgb, model, rays, n=(0.0, 0.0, 1.0)):
    p = _hit_points(rays)
    _assert_margins(model, p.astype(np.float32))
    ref = _plane_closed_form(model, p, n)
    dark = ~ref.any(axis=1)
    if model.kind == lm.PROJECTION:
        assert 4 <= (~dark).sum() and dark.sum() >= 4  # rays land inside and outside the projector's window
    assert np.all(rgb[dark] == 0.0)
    print(f"worst rel {np.abs(rgb[~dark] / ref[~dark] - 1).max():.3g} over {(~dark).sum()} lit points")
    np.testing.assert_allclose(rgb[~dark], ref[~dark], rtol=1e-4)


@pytest.mark.parametrize("with_map", [True, False], ids=["map", "no-map"])
@pytest.mark.parametrize("kind", [lm.PROJECTION, lm.GONIOMETRIC], ids=["projection", "goniometric"])
@pytest.mark.parametrize("integrator", INTEGRATORS, ids=["path", "direct", "whitted"])
def test_plane_closed_form(hip_ctx, integrator, kind, with_map):
    rgb_map = _map_of(kind) if with_map else None
    scene = pbrt_hip.Scene(hip_ctx, _plane_scene([_light(kind, DOWN)], {0: rgb_map} if with_map else None))
    rays = _plane_rays()
    rgb = _li_plane(scene, integrator, rays)
    scene.close()
    _check_plane(rgb, lm.LightMapModel(kind, DOWN, I, FOV, rgb_map), rays)


# ---- 3. a map-less goniometric light is a point light ----
def test_mapless_goniometric_light_is_the_point_light_bit_for_bit(hip_ctx):
    w = h = 32
    delta = scenes.cornell_delta_lights()
    gonio = list(delta)
    t = np.eye(4, dtype=np.float32)
    t[:3, 3] = delta[0]["pos"]
    gonio[0] = scenes.goniometric_light(t, delta[0]["L"])
    cam = scenes.cornell_camera(w, h)
    films = []
    for lights in (delta, gonio):
        scene = pbrt_hip.Scene(hip_ctx, scenes.with_lights(scenes.cornell_box(), lights))
        out = [scene.render(cam, w, h, 4, max_depth=5, light_strategy=s, seed=17)[0] for s in (0, 1, 2)]
        out.append(scene.render(cam, w, h, 4, integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=3, light_strategy=0, seed=17)[0])
        films.append(out)
        scene.close()
    for a, b in zip(*films):
        assert a[..., :3].mean() > 0.01
        assert np.array_equal(a, b)


# ---- 4. power and spatial distributions ----
def _mean_check(scene, strategy, rays, n_keys, ref):
    rep = np.repeat(rays, n_keys)
    keys = np.arange(len(rep), dtype=np.uint64) * 104729 + 11
    rgb, _ = scene.li(rep, keys, integrator=pbrt_hip.INTEGRATOR_PATH, max_depth=1, light_strategy=strategy)
    x = rgb.astype(np.float64).reshape(len(rays), n_keys, 3)
    mean, sigma = x.mean(axis=1), x.std(axis=1, ddof=1) / np.sqrt(n_keys)
    excess = np.abs(mean - ref) - (4 * sigma + 1e-4 * ref)
    print(f"strategy {strategy}: worst |mean - ref| - bound = {excess.max():.3g}, worst |mean / ref - 1| = {np.abs(mean / ref - 1).max():.3g}")
    assert np.all(excess <= 0)


def test_power_and_spatial_distributions(hip_ctx):
    p_point, i_point = np.array([-0.8, 0.6, 1.0]), np.array([0.6, 0.5, 0.4])
    scene = pbrt_hip.Scene(hip_ctx, _plane_scene([_light(lm.PROJECTION, DOWN), scenes.point_light(p_point, i_point)], {0: PROJ_MAP}, half=3.0))
    rays = _plane_rays(8)
    p = _hit_points(rays)

    def ref_for(rgb_map):
        model = lm.LightMapModel(lm.PROJECTION, DOWN, I, FOV, rgb_map)
        _assert_margins(model, p.astype(np.float32))
        d = p_point - p
        r2 = (d * d).sum(axis=1, keepdims=True)
        point = KD / np.pi * i_point / r2 * np.abs(d[:, 2:3]) / np.sqrt(r2)
        proj = _plane_closed_form(model, p)
        assert 4 <= proj.any(axis=1).sum() <= len(p) - 4
        return proj + point

    for strategy in (0, 1, 2):
        _mean_check(scene, strategy, rays, 256, ref_for(PROJ_MAP))
    scene.set_light_map(0, PROJ_MAP * 4.0)  # four times as bright: the spatial table is built again
    _mean_check(scene, 2, rays, 256, ref_for(PROJ_MAP * 4.0))
    scene.close()


# ---- 5. the setter ----
def test_set_light_map_twice_and_refusals(hip_ctx):
    scene = pbrt_hip.Scene(hip_ctx, _plane_scene([_light(lm.PROJECTION, DOWN), scenes.point_light((0.0, 0.0, 2.0), (0.1, 0.1, 0.1)),
                                                  (scenes.LIGHT_INFINITE, (0.0, 0.0, 0.0), -1, 0, 1)], {0: PROJ_MAP}))
    second = lm.gentle_map(4, 4, seed=3)[::-1].copy() * 0.7  # another size (square: the window changes too) and other texels
    scene.set_light_map(0, second)
    rays = _plane_rays()
    alone = pbrt_hip.Scene(hip_ctx, _plane_scene([_light(lm.PROJECTION, DOWN)], {0: PROJ_MAP}))
    alone.set_light_map(0, second)  # the plane's closed form holds against the second map
    for integrator in INTEGRATORS:
        _check_plane(_li_plane(alone, integrator, rays), lm.LightMapModel(lm.PROJECTION, DOWN, I, FOV, second), rays)
    alone.close()
    p = _hit_points(rays)
    model = lm.LightMapModel(lm.PROJECTION, DOWN, I, FOV, second)
    _assert_margins(model, p.astype(np.float32))
    wi, _, li = scene.light_sample_li(0, p)
    ref = model.sample_li(p)[2]
    dark = ~ref.any(axis=1)
    assert 4 <= dark.sum() <= len(p) - 4 and np.all(li[dark] == 0.0)
    np.testing.assert_allclose(li[~dark], ref[~dark], rtol=1e-4)
    keys = np.arange(len(rays), dtype=np.uint64) * 31 + 5
    before = [scene.li(rays, keys, max_depth=1, light_strategy=s)[0] for s in (0, 1, 2)]
    L = pbrt_hip.lib()
    ok = np.ones((4, 4, 3), np.float32)
    nan, neg = ok.copy(), ok.copy()
    nan[1, 2, 0], neg[3, 3, 2] = np.nan, -1.0
    refusals = [(7, ok, 4, 4, "light index"), (-1, ok, 4, 4, "light index"), (1, ok, 4, 4, "is not PBRT_LIGHT_PROJECTION"),
                (2, ok, 4, 4, "is not PBRT_LIGHT_PROJECTION"), (0, None, 4, 4, "null pointer"), (0, nan, 4, 4, "texels must be finite"),
                (0, neg, 4, 4, "texels must be finite"), (0, ok, 0, 4, "width and height"), (0, ok, 4, -2, "width and height"),
                (0, ok, 1 << 14, 1 << 14, "2^28 texels")]
    for light, rgb, w, h, reason in refusals:
        rc = L.pbrt_hip_scene_set_light_map(scene.h, light, None if rgb is None else rgb.ctypes.data, w, h)
        why = L.pbrt_hip_last_error(hip_ctx.h).decode()
        assert rc == 1 and reason in why, (light, w, h, rc, why)  # PBRT_HIP_ERR_INVALID
        after = [scene.li(rays, keys, max_depth=1, light_strategy=s)[0] for s in (0, 1, 2)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), reason
    with pytest.raises(pbrt_hip.PbrtHipError, match="PBRT_LIGHT_INFINITE"):
        scene.set_environment_map(0, ok)  # the environment-map setter keeps refusing these lights
    scene.close()


def test_creation_refusals_leave_the_context_usable(hip_ctx):
    def bad(field, index, value, kind=lm.PROJECTION):
        l = _light(kind, DOWN).copy()
        if index is None:
            l[field] = value
        else:
            l[field][index] = value
        return l
    cases = [(bad("pos", 1, np.nan), "pos and L"), (bad("L", 0, np.inf), "pos and L"), (bad("world_to_light", 4, np.nan, lm.GONIOMETRIC), "world_to_light"),
             (bad("pos", 2, -np.inf, lm.GONIOMETRIC), "pos and L"), (bad("fov", None, 0.0), "fov"), (bad("fov", None, 180.0), "fov"),
             (bad("fov", None, np.nan), "fov"), (bad("fov", None, -20.0), "fov"), (bad("type", None, 7), "unknown light type")]
    for light, reason in cases:
        with pytest.raises(pbrt_hip.PbrtHipError, match=reason) as e:
            pbrt_hip.Scene(hip_ctx, _plane_scene([light]))
        assert "(1)" in str(e.value)  # PBRT_HIP_ERR_INVALID
    # a goniometric light ignores fov; and the context still creates and renders
    scene = pbrt_hip.Scene(hip_ctx, _plane_scene([bad("fov", None, np.nan, lm.GONIOMETRIC)]))
    rays = _plane_rays()
    _check_plane(_li_plane(scene, pbrt_hip.INTEGRATOR_PATH, rays), lm.LightMapModel(lm.GONIOMETRIC, DOWN, I, FOV, None), rays)
    scene.close()


# ---- 6. other scene kinds ----
@pytest.mark.parametrize("kind", [lm.PROJECTION, lm.GONIOMETRIC], ids=["projection", "goniometric"])
@pytest.mark.parametrize("integrator", INTEGRATORS, ids=["path", "direct", "whitted"])
def test_plane_inside_an_instance(hip_ctx, integrator, kind):
    """two levels: the plane at z = -1 in object space under an instance that lifts it to z = 0; the light is a world-space light"""
    positions, indices = scenes._plane_z0(10.0)
    positions[:, 2] = -1.0
    inst = np.zeros((1, 2, 4, 4), np.float32)
    inst[0, 0] = inst[0, 1] = np.eye(4)
    inst[0, 0][2, 3], inst[0, 1][2, 3] = 1.0, -1.0
    sc = dict(positions=positions, indices=indices, tri_material=np.zeros(2, np.int32), materials=scenes._materials([MATTE]),
              tri_light=np.full(2, -1, np.int32), instances=inst, instance_material=np.full(1, -1, np.int32),
              lights=scenes._lights([_light(kind, DOWN)]), light_maps={0: _map_of(kind)})
    scene = pbrt_hip.Scene(hip_ctx, sc)
    rays = _plane_rays()
    rgb = _li_plane(scene, integrator, rays)
    scene.close()
    _check_plane(rgb, lm.LightMapModel(kind, DOWN, I, FOV, _map_of(kind)), rays)


@pytest.mark.parametrize("kind", [lm.PROJECTION, lm.GONIOMETRIC], ids=["projection", "goniometric"])
@pytest.mark.parametrize("integrator", INTEGRATORS, ids=["path", "direct", "whitted"])
def test_disk_in_a_shapes_scene(hip_ctx, integrator, kind):
    """a Disk of radius 10 at z = 0 in place of the plane: the kernels for scenes with general shapes"""
    speck = np.array([[50.0, 50.0, 50.0], [50.001, 50.0, 50.0], [50.0, 50.001, 50.0]], dtype=np.float32)  # a scene needs a triangle
    sc = dict(positions=speck, indices=np.array([[0, 1, 2]], np.int32), tri_material=np.zeros(1, np.int32), tri_light=np.full(1, -1, np.int32),
              materials=scenes._materials([MATTE]), lights=scenes._lights([_light(kind, DOWN)]), shapes=scenes.shapes(scenes.disk(0.0, 10.0)),
              light_maps={0: _map_of(kind)})
    scene = pbrt_hip.Scene(hip_ctx, sc)
    rays = _plane_rays()
    rgb = _li_plane(scene, integrator, rays)
    scene.close()
    _check_plane(rgb, lm.LightMapModel(kind, DOWN, I, FOV, _map_of(kind)), rays)
