"""Camera motion blur on the GPU: PbrtCameraMotion through pbrt_hip_render_moving_camera / _camera_rays_moving_camera
(k_generate_moving_camera, pbrt-rs_amd/csrc/wf_camera_motion.h) against the static camera bit for bit where the two must agree,
against the float64 model of tests/motion_model.py where the device interpolates, and against closed forms.

Held shutters: a ray's time is (1 - u) open + u close as the device evaluates it; with open == close == a that is exactly a only
where both products are exact, so every held time below is 0 or a power of two (tests/test_gpu_motion_paths.py:
test_camera_rays_return_the_samplers_first_1d_draw_as_the_time), and the time ranges are chosen around such times.

test_rays_against_the_model, measured on gfx950 (MI355X), worst absolute deviation over the six times, animated path / baseline
(the static camera holding the model's matrix rounded to float); the bound is 4 x the baseline, the ratio
test_gpu_motion.py::test_hits_against_the_model uses for the same comparison:
                                        origin                        direction
  perspective + lens, slerp             4.034573e-07 / 4.034573e-07   8.492752e-08 / 8.094592e-08
  perspective + lens, normalised lerp   3.442721e-07 / 3.442721e-07   9.059490e-08 / 8.666165e-08
  orthographic + lens, slerp            6.819371e-07 / 5.876307e-07   8.119965e-08 / 8.119965e-08
  orthographic + lens, normalised lerp  6.318680e-07 / 5.839982e-07   8.757813e-08 / 8.757813e-08
  environment, slerp                    3.060018e-07 / 2.900446e-07   1.066869e-07 / 9.662014e-08
  environment, normalised lerp          3.041245e-07 / 2.919220e-07   1.006325e-07 / 1.054007e-07
(the origins' deviation is mostly the step along the ray that covers the transform's rounding error, which both paths take).
"""
import os
import subprocess

import numpy as np
import pytest

import motion_model as mm
import pbrt_hip
from motion_cases import BLUR_SHIFT, FIVE, KD, LIGHT_L, MATERIALS, QUAD, RES, SPP, f32, make_scene, rot, tr
from pbrt_hip import scenes
from test_cpp_example import _build as build_cpp
from test_gpu_motion import overlap, pixel_edges

pytestmark = pytest.mark.gpu

W = H = 48
INTEGRATORS = {"path": pbrt_hip.INTEGRATOR_PATH, "direct": pbrt_hip.INTEGRATOR_DIRECT, "whitted": pbrt_hip.INTEGRATOR_WHITTED,
               "ao": pbrt_hip.INTEGRATOR_AO}
KW = dict(max_depth=3, ao_samples=4, seed=5)
R = KD / np.pi * LIGHT_L


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _quad(x0, x1, y0, y1, z, tilt=0.0):
    return [[x0, y0, z - tilt], [x1, y0, z + tilt], [x1, y1, z + tilt], [x0, y1, z - tilt]]


def one_level_scene():
    """Triangles only, in front of a camera that looks along +z from around the origin: a back wall, a tilted matte quad, a mirror,
    a glass pane; a point and a distant light. One level, no shapes: the 4-wide records."""
    quads = [(_quad(-5, 5, -5, 5, 7.0), 0), (_quad(-1.5, 0.25, -1.0, 0.75, 4.0, 0.5), 0), (_quad(0.5, 2.0, -0.5, 1.5, 5.0, -0.4), 2),
             (_quad(-0.5, 0.75, -1.75, -0.25, 3.0, 0.1), 1)]
    pos = np.array([p for q, _ in quads for p in q], dtype=np.float32)
    idx = np.array([[4 * i + a, 4 * i + b, 4 * i + c] for i in range(len(quads)) for a, b, c in ((0, 1, 2), (0, 2, 3))], dtype=np.int32)
    mat = np.array([m for _, m in quads for _ in range(2)], dtype=np.int32)
    return dict(positions=pos, indices=idx, tri_material=mat, materials=scenes._materials(MATERIALS), tri_light=np.full(len(idx), -1, np.int32),
                lights=scenes._lights([scenes.point_light((0.5, 2.0, 1.0), (30.0, 28.0, 25.0)), scenes.distant_light((0.2, 0.3, -1.0), (LIGHT_L,) * 3)]))


def moving_scene():
    """tests/motion_cases.py's five instances (four of them moving over [0.25, 1.75]), five units down the z axis, before a wall"""
    ahead = [(k, tr(0, 0, 5) @ m0, None if m1 is None else tr(0, 0, 5) @ m1) for k, m0, m1 in FIVE]
    wall = dict(positions=np.array(_quad(-6, 6, -6, 6, 8.0), dtype=np.float32), indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32),
                tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    return make_scene(ahead, world=wall, lights=(scenes.distant_light((0.2, 0.3, -1.0), (LIGHT_L,) * 3), scenes.point_light((0.5, 2.0, 1.0), (30.0, 28.0, 25.0))))


def shapes_scene():
    sc = {k: v for k, v in scenes.sphere_scene().items() if k != "spheres"}
    return dict(sc, shapes=scenes.shapes(scenes.sphere_shape(1.0, material=0), scenes.disk(-1.0, 2.0, material=0)))


@pytest.fixture(scope="module")
def one(hip_ctx):
    g = pbrt_hip.Scene(hip_ctx, one_level_scene())
    assert g.wide_records()[0] != -1          # the 4-wide records are there: an animated camera keeps them
    yield g
    g.close()


@pytest.fixture(scope="module")
def moving(hip_ctx):
    g = pbrt_hip.Scene(hip_ctx, moving_scene())
    assert g.wide_records() == (-1, "scene with moving instances")
    yield g
    g.close()


def general_camera(w=W, h=H, **kw):
    return scenes.perspective_camera((1.0, -1.0, -1.0), (0.0, 0.0, 5.0), (0.0, 1.0, 0.0), 50.0, w, h, **kw)


def with_matrix(cam, m):
    out = cam.copy()
    out["camera_to_world"] = np.asarray(m, dtype=np.float32).reshape(16)
    return out


def held(cam, t):
    out = cam.copy()
    out["shutter_open"] = out["shutter_close"] = t
    return out


def same_rays(a, b, time=True):
    """camera_rays outputs equal byte for byte; time=False: all but the rays' time (which a static camera on a static scene leaves 0)"""
    (ra, ka, fa, pa), (rb, kb, fb, pb_) = a, b
    for f in ("o", "d", "t_max") + (("time",) if time else ()):
        assert np.array_equal(bits(ra[f]), bits(rb[f])), f
    assert np.array_equal(ka, kb) and np.array_equal(bits(fa), bits(fb)) and np.array_equal(pa, pb_)


# a general motion: look_at matrices 40 degrees apart, plus a translation; over [0.5, 2] (see the module docstring)
G0 = f32(scenes.look_at((1.0, -1.0, -1.0), (0.0, 0.0, 5.0), (0.0, 1.0, 0.0)))
G1 = f32(tr(0.5, 0.25, -0.5) @ rot((0.0, 1.0, 0.0), 40) @ scenes.look_at((1.0, -1.0, -1.0), (0.0, 0.0, 5.0), (0.0, 1.0, 0.0)))
GT0, GT1 = 0.5, 2.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. the static camera is the old code
# ---------------------------------------------------------------------------------------------------------------------
def test_static_is_the_old_code(hip_ctx, one, moving):
    off = scenes.camera_motion(G1, GT0, GT1)
    off["animated"], off["end_time"] = 0, off["start_time"]            # not read for a static camera
    spheres, shapes = pbrt_hip.Scene(hip_ctx, scenes.sphere_scene()), pbrt_hip.Scene(hip_ctx, shapes_scene())
    cases = [("one-level", one, general_camera(), list(INTEGRATORS)), ("spheres", spheres, scenes.sphere_camera(W, H), ["path"]),
             ("shapes", shapes, scenes.sphere_camera(W, H), ["path"]), ("moving", moving, general_camera(), list(INTEGRATORS))]
    for name, g, cam, integrators in cases:
        cam["shutter_open"], cam["shutter_close"] = 0.25, 1.75
        for i in integrators:
            old, _ = g.render(cam, W, H, 4, integrator=INTEGRATORS[i], **KW)                   # pbrt_hip_render: a NULL motion
            new, _ = g.render(cam, W, H, 4, integrator=INTEGRATORS[i], camera_motion=off, **KW)
            assert np.array_equal(bits(old), bits(new)), (name, i)
            assert pbrt_hip.film_to_rgb(old).max() > 0.0, (name, i)
        same_rays(g.camera_rays(cam, W, H, 4, seed=5), g.camera_rays(cam, W, H, 4, seed=5, camera_motion=off))
    spheres.close()
    shapes.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. at and beyond the ends of the time range: the stored matrices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "moving"])
def test_the_ends(one, moving, which):
    g = one if which == "one" else moving
    cam, motion = with_matrix(general_camera(), G0), scenes.camera_motion(G1, GT0, GT1)
    films = {}
    for t, m in ((GT0, G0), (0.25, G0), (GT1, G1), (4.0, G1)):
        a, s = held(cam, t), held(with_matrix(cam, m), t)
        rays = g.camera_rays(a, W, H, 4, seed=5, camera_motion=motion)
        same_rays(rays, g.camera_rays(s, W, H, 4, seed=5), time=which == "moving")
        assert np.array_equal(rays[0]["time"][rays[3][:, 0] >= 0], np.full((rays[3][:, 0] >= 0).sum(), t, np.float32))
        films[t], _ = g.render(a, W, H, 4, camera_motion=motion, **KW)
        want, _ = g.render(s, W, H, 4, **KW)
        assert np.array_equal(bits(films[t]), bits(want)), t
    assert not np.array_equal(bits(films[GT0]), bits(films[GT1]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. a motion whose interpolation is exact in float32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "moving"])
def test_exact_interpolation(one, moving, which):
    """translate(-1, 0.5, 0.25) -> translate(1, 1.5, 0.75) over [0, 2], the shutter held at 1: u = 0.5, the identity rotation and
    powers of two make every product and sum of T(u) R(u) S(u) exact, so the camera IS the static one at translate(0, 1, 0.5)."""
    g = one if which == "one" else moving
    base = scenes.perspective_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 60.0, W, H)
    start, motion = with_matrix(base, tr(-1, 0.5, 0.25)), scenes.camera_motion(tr(1, 1.5, 0.75), 0.0, 2.0)
    middle = with_matrix(base, tr(0, 1, 0.5))
    same_rays(g.camera_rays(held(start, 1.0), W, H, 4, seed=5, camera_motion=motion), g.camera_rays(held(middle, 1.0), W, H, 4, seed=5),
              time=which == "moving")
    for name, i in INTEGRATORS.items():
        got, _ = g.render(held(start, 1.0), W, H, 4, integrator=i, camera_motion=motion, **KW)
        want, _ = g.render(held(middle, 1.0), W, H, 4, integrator=i, **KW)
        at_start, _ = g.render(held(start, 0.0), W, H, 4, integrator=i, camera_motion=motion, **KW)
        assert np.array_equal(bits(got), bits(want)), name
        assert pbrt_hip.film_to_rgb(got).max() > 0.0 and not np.array_equal(bits(got), bits(at_start)), name


# ---------------------------------------------------------------------------------------------------------------------
# 4. interior times: the rays against the float64 model
# ---------------------------------------------------------------------------------------------------------------------
MODEL_T0, MODEL_T1 = 0.0625, 8.0
MODEL_TIMES = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0)      # powers of two inside the range: u from 0.008 to 0.496
MODEL_MOTIONS = {"slerp": (G0, G1),                   # 40 degrees apart: r0 . r1 = cos(20 degrees) < 0.9995
                 "normalised_lerp": (G0, f32(tr(0.5, 0.25, -0.5) @ rot((0.0, 1.0, 0.0), 3) @ G0))}
MODEL_CAMERAS = {"perspective_lens": lambda: general_camera(16, 16, lens_radius=0.05, focal_distance=5.0),
                 "orthographic_lens": lambda: scenes.orthographic_camera((1.0, -1.0, -1.0), (0.0, 0.0, 5.0), (0.0, 1.0, 0.0), 2.0, 16, 16, lens_radius=0.05, focal_distance=5.0),
                 "environment": lambda: scenes.environment_camera((1.0, -1.0, -1.0), (0.0, 0.0, 5.0), (0.0, 1.0, 0.0))}


@pytest.mark.parametrize("motion_name", list(MODEL_MOTIONS))
@pytest.mark.parametrize("camera_name", list(MODEL_CAMERAS))
def test_rays_against_the_model(one, camera_name, motion_name):
    """Expected ray: the camera-space ray (the same call with an identity camera_to_world: same sampler and seed, same samples)
    through the model's float64 interpolate(time). Baseline: the static camera holding that matrix rounded to float. The animated
    path adds the float32 roundings of slerp and compose and is allowed 4 times the baseline's worst absolute deviation."""
    m0, m1 = MODEL_MOTIONS[motion_name]
    model = mm.Motion(m0, m1, MODEL_T0, MODEL_T1)
    assert (np.dot(model.q0, model.q1) > mm.SLERP_LERP_ABOVE) == (motion_name == "normalised_lerp")
    cam, motion = with_matrix(MODEL_CAMERAS[camera_name](), m0), scenes.camera_motion(m1, MODEL_T0, MODEL_T1)
    worst = dict(o=[0.0, 0.0], d=[0.0, 0.0])
    for t in MODEL_TIMES:
        local, _, _, pix = one.camera_rays(held(with_matrix(cam, np.eye(4)), t), 16, 16, 4, seed=9)
        ok = pix[:, 0] >= 0
        assert ok.sum() == 16 * 16 * 4
        m = model.interpolate(np.float64(t))
        want_o = local["o"][ok].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        want_d = local["d"][ok].astype(np.float64) @ m[:3, :3].T
        got, _, _, _ = one.camera_rays(held(cam, t), 16, 16, 4, seed=9, camera_motion=motion)
        base, _, _, _ = one.camera_rays(held(with_matrix(cam, m), t), 16, 16, 4, seed=9)
        assert np.array_equal(got["time"][ok], np.full(ok.sum(), t, np.float32))        # the held shutter time, bit for bit
        for k, (rays, want) in enumerate(((got, (want_o, want_d)), (base, (want_o, want_d)))):
            worst["o"][k] = max(worst["o"][k], float(np.abs(rays["o"][ok] - want[0]).max()))
            worst["d"][k] = max(worst["d"][k], float(np.abs(rays["d"][ok] - want[1]).max()))
        assert np.abs(got["d"][ok]).max() > 0.1
    print(f"{camera_name} / {motion_name}: origin animated {worst['o'][0]:.6e} baseline {worst['o'][1]:.6e}; "
          f"direction animated {worst['d'][0]:.6e} baseline {worst['d'][1]:.6e}")
    assert worst["o"][0] <= 4 * worst["o"][1] and worst["d"][0] <= 4 * worst["d"][1]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the time is the sampler's first 1D draw
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [None, ("stratified", 4, 4, True, 3), ("zerotwo", 3), ("halton",)], ids=["random", "stratified", "zerotwo", "halton"])
def test_the_time_draw(one, moving, sampler):
    """an open shutter on a STATIC scene: the animated camera's rays carry the times the old entry point returns for a scene with
    moving instances (k_generate_moving) at the same film, sampler and seed"""
    cam = with_matrix(general_camera(16, 16), G0)
    cam["shutter_open"], cam["shutter_close"] = 0.25, 1.75
    new = one.camera_rays(cam, 16, 16, 16, seed=7, sampler=sampler, camera_motion=scenes.camera_motion(G1, GT0, GT1))
    old = moving.camera_rays(cam, 16, 16, 16, seed=7, sampler=sampler)
    ok = old[3][:, 0] >= 0
    assert ok.sum() == 16 * 16 * 16 and np.array_equal(new[3], old[3])
    assert np.array_equal(bits(new[0]["time"]), bits(old[0]["time"]))
    t = old[0]["time"][ok]
    assert t.min() >= 0.25 and t.max() <= 1.75 and len(np.unique(t)) > 16
    # and without a motion the static scene's rays carry none (DESIGN D96): the time above is the animated camera's doing
    assert not one.camera_rays(cam, 16, 16, 16, seed=7, sampler=sampler)[0]["time"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a pan over a static quad is the coverage trapezoid
# ---------------------------------------------------------------------------------------------------------------------
PAN_X0, PAN_Y0 = 0.77, 0.02         # examples/render_camera_pan.cpp: the same quad, light, camera, pan, integrator and seed
PAN_KW = dict(integrator=pbrt_hip.INTEGRATOR_DIRECT, max_depth=1, light_strategy=0, seed=3)


def pan_scene():
    pos = QUAD[0] + np.array([PAN_X0, PAN_Y0, 0.0], dtype=np.float32)
    return dict(positions=pos.astype(np.float32), indices=QUAD[1], tri_material=np.zeros(2, np.int32), materials=scenes._materials(MATERIALS[:1]),
                tri_light=np.full(2, -1, np.int32), lights=scenes._lights([scenes.distant_light((0, 0, 1.0), (LIGHT_L,) * 3)]))


def pan_camera(shift=BLUR_SHIFT):
    cam = scenes.orthographic_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 2.0, RES, RES)
    return cam, scenes.camera_motion(tr(shift, 0, 0) @ cam["camera_to_world"].astype(np.float64).reshape(4, 4), 0.0, 1.0)


def trapezoid(xs, shift, x0, rows):
    """per column: rows x the fraction of u in [0, 1] with |x + shift u - x0| <= 0.5, by the midpoint rule over the column's width"""
    sub = (np.arange(2048) + 0.5) / 2048
    expect = np.zeros(RES)
    for c in range(RES):
        x = xs[c] + (xs[c + 1] - xs[c]) * sub
        lo, hi = (x0 - 0.5 - x) / shift, (x0 + 0.5 - x) / shift
        expect[c] = rows * np.clip(np.minimum(hi, 1.0) - np.maximum(lo, 0.0), 0.0, None).mean()
    return expect


@pytest.fixture(scope="module")
def pan(hip_ctx):
    g = pbrt_hip.Scene(hip_ctx, pan_scene())
    assert g.wide_records()[0] != -1
    yield g
    g.close()


def test_a_pan_is_the_coverage_trapezoid(pan):
    cam, motion = pan_camera()
    film, _ = pan.render(cam, RES, RES, SPP, camera_motion=motion, **PAN_KW)
    film_still, _ = pan.render(held(cam, 0.0), RES, RES, SPP, camera_motion=motion, **PAN_KW)
    xs, ys = pixel_edges(cam)
    col = pbrt_hip.film_to_rgb(film)[:, :, 1].astype(np.float64).mean(axis=0) / R
    expect = trapezoid(xs, BLUR_SHIFT, PAN_X0, overlap(ys, PAN_Y0 - 0.5, PAN_Y0 + 0.5).mean())
    sigma = np.sqrt(expect * (1.0 - expect) / (RES * SPP))
    print(f"camera pan: largest column mean {col.max():.4f} (expected {expect.max():.4f}), worst deviation / sigma "
          f"{np.max(np.abs(col - expect)[sigma > 0] / sigma[sigma > 0]):.2f}")
    assert expect.max() > 0.15 and (expect == 0).sum() > 10
    assert (col[expect == 0] == 0.0).all()
    assert np.all(np.abs(col - expect) <= 5 * sigma + 1e-6)   # 1e-6: the midpoint rule
    assert np.abs(col - pbrt_hip.film_to_rgb(film_still)[:, :, 1].mean(axis=0) / R).max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# 7. a tracking shot: the tracked quad is sharp, the static one blurred
# ---------------------------------------------------------------------------------------------------------------------
def test_tracking_shot(hip_ctx):
    shift = 1.0                                    # a power of two: camera and instance translate by the same float32 sums
    tracked, fixed = (-1.23, 1.02), (0.77, -0.98)  # the tracked quad in the rows above y = 0, the static one below
    sc = make_scene([(0, tr(*tracked, 0), tr(tracked[0] + shift, tracked[1], 0)), (0, tr(*fixed, 0), None)], objects=(QUAD,),
                    lights=(scenes.distant_light((0, 0, 1.0), (LIGHT_L,) * 3),))
    sc["instance_motion"] = {0: scenes.instance_motion(tr(tracked[0] + shift, tracked[1], 0), 0.0, 1.0)}
    g = pbrt_hip.Scene(hip_ctx, sc)
    cam, motion = pan_camera(shift)
    film, _ = g.render(cam, RES, RES, SPP, camera_motion=motion, **PAN_KW)
    g.close()
    rgb = pbrt_hip.film_to_rgb(film)[:, :, 1].astype(np.float64)
    xs, ys = pixel_edges(cam)
    top = np.maximum(ys[:-1], ys[1:]) > 0.0 + 1e-9
    assert top.sum() == RES // 2
    # the tracked quad, in the camera's frame of time 0, where it stays
    cover = overlap(ys, tracked[1] - 0.5, tracked[1] + 0.5)[:, None] * overlap(xs, tracked[0] - 0.5, tracked[0] + 0.5)[None, :]
    assert (cover == 1.0).sum() > 150
    assert np.allclose(rgb[cover == 1.0], R, rtol=1e-4, atol=0.0)
    assert (rgb[top][cover[top] == 0.0] == 0.0).all() and (cover[top] == 0.0).sum() > 1500
    # the static quad's rows: the trapezoid of the pan
    col = rgb[~top].mean(axis=0) / R
    expect = trapezoid(xs, shift, fixed[0], overlap(ys[RES // 2:], fixed[1] - 0.5, fixed[1] + 0.5).mean())
    sigma = np.sqrt(expect * (1.0 - expect) / (RES // 2 * SPP))
    print(f"tracking shot: static quad, largest column mean {col.max():.4f} (expected {expect.max():.4f}), worst deviation / sigma "
          f"{np.max(np.abs(col - expect)[sigma > 0] / sigma[sigma > 0]):.2f}")
    assert expect.max() > 0.15 and (expect == 0).sum() > 10
    assert (col[expect == 0] == 0.0).all()
    assert np.all(np.abs(col - expect) <= 5 * sigma + 1e-6)
    partly = (col > 0.02) & (col < 0.9 * col.max())
    assert partly.sum() >= 10          # blurred: columns covered for a part of the shutter only


# ---------------------------------------------------------------------------------------------------------------------
# 8. li over camera_rays is render
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,integrator", [("one", "path"), ("moving", "whitted")])
def test_li_over_camera_rays_is_render(one, moving, which, integrator):
    g = one if which == "one" else moving
    cam, motion = with_matrix(general_camera(), G0), scenes.camera_motion(G1, GT0, GT1)
    cam["shutter_open"], cam["shutter_close"] = 0.25, 2.5      # times before, inside and after the camera's range
    spp = 4
    kw = dict(integrator=INTEGRATORS[integrator], max_depth=3, light_strategy=1)
    film, st = g.render(cam, W, H, spp, seed=5, camera_motion=motion, **kw)
    rays, keys, pfilm, pix = g.camera_rays(cam, W, H, spp, seed=5, camera_motion=motion)
    valid = pix[:, 0] >= 0
    assert valid.sum() == W * H * spp
    t = rays["time"][valid]
    assert (t < GT0).sum() > 100 and (t > GT1).sum() > 100 and ((t > GT0) & (t < GT1)).sum() > 1000
    x, y, s = (pix[valid, k].astype(np.int64) for k in range(3))
    rgb, st_li = g.li(rays[valid], keys[valid], draws_before_li=5, **kw)
    assert st_li["rays_closest"] + st_li["rays_shadow"] == st["rays_closest"] + st["rays_shadow"]
    f4 = np.float32
    acc = np.zeros((H, W, 3), dtype=np.float32)
    order = np.lexsort((s, x, y))
    for k in range(spp):            # the k-th sample of every pixel at once: per pixel the additions stay in sample order
        sel = order[k::spp]
        assert np.array_equal(s[sel], np.full(len(sel), k))
        acc[y[sel], x[sel]] += rgb[sel]
    xyz = np.stack([f4(0.412453) * acc[..., 0] + f4(0.357580) * acc[..., 1] + f4(0.180423) * acc[..., 2],
                    f4(0.212671) * acc[..., 0] + f4(0.715160) * acc[..., 1] + f4(0.072169) * acc[..., 2],
                    f4(0.019334) * acc[..., 0] + f4(0.119193) * acc[..., 1] + f4(0.950227) * acc[..., 2]], axis=-1)
    assert np.array_equal(film[..., 3], np.full((H, W), spp, dtype=np.float32))
    assert xyz.astype(np.float32).tobytes() == np.ascontiguousarray(film[..., :3]).tobytes()
    assert acc.max() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 9. tile shares, and the C++ surface
# ---------------------------------------------------------------------------------------------------------------------
def test_tile_shares_add_up(one, moving):
    cam, motion = with_matrix(general_camera(), G0), scenes.camera_motion(G1, GT0, GT1)
    cam["shutter_open"], cam["shutter_close"] = 0.25, 2.5
    for g in (one, moving):
        whole, _ = g.render(cam, W, H, 4, camera_motion=motion, **KW)
        assert pbrt_hip.film_to_rgb(whole).max() > 0.0
        for order in (0, 1):
            parts = [g.render(cam, W, H, 4, tile_rank=r, tile_world=2, tile_order=order, camera_motion=motion, **KW)[0] for r in (0, 1)]
            assert all(p[..., 3].max() > 0.0 for p in parts)
            assert not ((parts[0][..., 3] > 0.0) & (parts[1][..., 3] > 0.0)).any()
            assert np.array_equal(bits(parts[0] + parts[1]), bits(whole)), order


def test_cpp_camera_pan_is_the_python_job(pan, tmp_path):
    exe = build_cpp(tmp_path, "render_camera_pan.cpp")
    cam, motion = pan_camera()
    for args, kw in (([], {}), (["1", "2"], dict(tile_rank=1, tile_world=2))):
        out = tmp_path / "film.raw"
        r = subprocess.run([exe, str(out), str(RES), str(SPP)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want, st = pan.render(cam, RES, RES, SPP, camera_motion=motion, **PAN_KW, **kw)
        assert f"camera pan: {st['camera_samples']} camera samples, {st['rays_closest']} closest-hit + {st['rays_shadow']} shadow rays" in r.stdout, r.stdout
        got = np.fromfile(out, dtype=np.float32).reshape(RES, RES, 4)
        assert np.array_equal(bits(got), bits(want)) and got[..., :3].max() > 0.0
        os.remove(out)


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals on the device path: each leaves the context usable
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx, one):
    cam, motion = with_matrix(general_camera(), G0), scenes.camera_motion(G1, GT0, GT1)
    cam["shutter_open"], cam["shutter_close"] = 0.25, 2.5
    first, _ = one.render(cam, W, H, 4, camera_motion=motion, **KW)
    singular, not_affine, nan = G1.copy(), G1.copy(), G1.copy()
    singular[:3, 2] = singular[:3, 1]
    not_affine[3] = (0, 0, 0.1, 1)
    nan[1, 2] = np.nan
    cases = [(G0, nan, GT0, GT1, "a non-finite matrix entry"), (G0, not_affine, GT0, GT1, "not affine"), (not_affine, G1, GT0, GT1, "not affine"),
             (G0, singular, GT0, GT1, "a singular matrix"), (singular, G1, GT0, GT1, "a singular matrix"),
             (G0, G1, 1.0, 1.0, "end_time <= start_time"), (G0, G1, 2.0, 0.5, "end_time <= start_time")]
    for a, b, t0, t1, why in cases:
        with pytest.raises(pbrt_hip.PbrtHipError, match="camera motion: .*" + why):
            one.render(with_matrix(cam, a), W, H, 4, camera_motion=scenes.camera_motion(b, t0, t1), **KW)
        with pytest.raises(pbrt_hip.PbrtHipError, match="camera motion: .*" + why):
            one.camera_rays(with_matrix(cam, a), W, H, 4, camera_motion=scenes.camera_motion(b, t0, t1))
        again, _ = one.render(cam, W, H, 4, camera_motion=motion, **KW)     # the next valid render on the same context
        assert np.array_equal(bits(again), bits(first)), why
    fresh_ctx = pbrt_hip.Context(0)
    fresh = pbrt_hip.Scene(fresh_ctx, one_level_scene())
    want, _ = fresh.render(cam, W, H, 4, camera_motion=motion, **KW)
    fresh.close()
    fresh_ctx.close()
    assert np.array_equal(bits(first), bits(want))
    # a camera with scale is accepted
    scaled, _ = one.render(cam, W, H, 4, camera_motion=scenes.camera_motion(f32(G1 @ np.diag([2.0, 2.0, 2.0, 1.0])), GT0, GT1), **KW)
    assert np.isfinite(scaled).all()
