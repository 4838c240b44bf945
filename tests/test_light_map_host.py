"""ProjectionLight's and GonioPhotometricLight's tables on the host (pbrt_hip_light_map_tables) against the float64 model of
light_map_model.py: level 0, lookup((0.5, 0.5), 0.5), the projector's window, cos_total_width and the power;
the refusals; PbrtLight's layout; the model against itself; the C++ surface compiles. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import envmap_model as em
import light_map_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.dirname(pbrt_hip.LIB_PATH)
FOV = 50.0


def _map(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 3.0, size=(h, w, 3)).astype(np.float32)


# (h, w): 4x4; 5 wide x 3 high (resampled, aspect > 1); 3 wide x 5 high (aspect < 1); 1x1; no map
SIZES = [(4, 4), (3, 5), (5, 3), (1, 1), None]


@pytest.mark.parametrize("kind", [lm.PROJECTION, lm.GONIOMETRIC])
@pytest.mark.parametrize("size", SIZES)
def test_tables_match_the_model(kind, size):
    rgb = None if size is None else _map(size[0], size[1], 11)
    t = pbrt_hip.light_map_tables(kind, rgb, fov=FOV)
    model = lm.LightMapModel(kind, None, (1.0, 1.0, 1.0), FOV, rgb)
    if rgb is None:
        assert t["level0"] is None
        assert np.array_equal(t["lookup"], np.ones(3, np.float32))  # exactly 1 without a map
    else:
        ref = model.l0
        assert t["level0"].shape == ref.shape == (em.pow2(size[0]), em.pow2(size[1]), 3)
        if ref.shape[:2] == tuple(size):
            assert np.array_equal(t["level0"], rgb)  # the texels as they are: I is not multiplied in
        # the tolerances test_envmap_host.py holds the same quantities to
        np.testing.assert_allclose(t["level0"], ref, rtol=1e-5, atol=1e-6 * ref.max())
        np.testing.assert_allclose(t["lookup"], model.lookup_half(), rtol=1e-6)
    if kind == lm.PROJECTION:
        assert np.array_equal(t["screen_bounds"], model.sb.astype(np.float32))  # exactly
        np.testing.assert_allclose(t["cos_total_width"], model.cos_total_width, rtol=1e-6)
    else:
        assert np.array_equal(t["screen_bounds"], np.zeros(4, np.float32)) and t["cos_total_width"] == -1.0
    np.testing.assert_allclose(t["power"], model.power(), rtol=1e-6)


def test_window_follows_the_aspect_of_the_map_as_passed():
    wide = pbrt_hip.light_map_tables(lm.PROJECTION, _map(3, 5, 1), fov=FOV)["screen_bounds"]
    tall = pbrt_hip.light_map_tables(lm.PROJECTION, _map(5, 3, 1), fov=FOV)["screen_bounds"]
    none = pbrt_hip.light_map_tables(lm.PROJECTION, None, fov=FOV)["screen_bounds"]
    assert np.array_equal(wide, np.array([-5 / 3, -1, 5 / 3, 1], np.float32))  # 5 / 3, not the resampled 8 / 4
    assert np.array_equal(tall, np.array([-1, -5 / 3, 1, 5 / 3], np.float32))
    assert np.array_equal(none, np.array([-1, -1, 1, 1], np.float32))


def test_power_without_a_map_is_the_closed_form():
    g = pbrt_hip.light_map_tables(lm.GONIOMETRIC)
    np.testing.assert_allclose(g["power"], 4 * np.pi, rtol=1e-6)
    p = pbrt_hip.light_map_tables(lm.PROJECTION, fov=90.0)
    # fov 90: inv_tan = 1, the corner direction is (1, 1, 1) / sqrt(3)
    np.testing.assert_allclose(p["cos_total_width"], 1 / np.sqrt(3), rtol=1e-6)
    np.testing.assert_allclose(p["power"], 2 * np.pi * (1 - 1 / np.sqrt(3)), rtol=1e-6)


def _tables_rc(kind, fov, rgb, w, h, res=True):
    rw, rh, why, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_char_p(), ctypes.c_float()
    out = np.zeros(3, np.float32)
    rc = pbrt_hip.lib().pbrt_hip_light_map_tables(kind, fov, None if rgb is None else rgb.ctypes.data, w, h, ctypes.byref(rw) if res else None,
                                                  ctypes.byref(rh) if res else None, None, out.ctypes.data, None, ctypes.byref(c),
                                                  out.ctypes.data, ctypes.byref(why))
    return rc, (why.value or b"").decode()


def test_refusals_are_invalid_with_a_reason():
    ok = np.ones((4, 4, 3), np.float32)
    cases = [((scenes.LIGHT_POINT, FOV, ok, 4, 4), "light type"), ((7, FOV, ok, 4, 4), "light type"),
             ((lm.PROJECTION, 0.0, ok, 4, 4), "fov"), ((lm.PROJECTION, 180.0, ok, 4, 4), "fov"), ((lm.PROJECTION, -3.0, ok, 4, 4), "fov"),
             ((lm.PROJECTION, float("nan"), ok, 4, 4), "fov"), ((lm.PROJECTION, float("inf"), None, 0, 0), "fov"),
             ((lm.GONIOMETRIC, 0.0, ok, 0, 4), "width and height must be >= 1"), ((lm.PROJECTION, FOV, ok, 4, -1), "width and height must be >= 1"),
             ((lm.GONIOMETRIC, 0.0, ok, 1 << 14, 1 << 14), "2^28 texels")]   # refused before a texel is read
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        t = ok.copy()
        t[2, 3, 1] = bad
        cases.append(((lm.GONIOMETRIC, 0.0, t, 4, 4), "texels must be finite and >= 0"))
        cases.append(((lm.PROJECTION, FOV, t, 4, 4), "texels must be finite and >= 0"))
    for args, reason in cases:
        rc, why = _tables_rc(*args)
        assert rc == 1 and reason in why, (args[:2], args[3:], rc, why)  # PBRT_HIP_ERR_INVALID
    rc, why = _tables_rc(lm.GONIOMETRIC, 0.0, ok, 4, 4, res=False)
    assert rc == 1 and "null pointer" in why
    assert _tables_rc(lm.GONIOMETRIC, 0.0, ok, 4, 4)[0] == 0 and _tables_rc(lm.PROJECTION, 179.0, None, 0, 0)[0] == 0


def test_light_record_layout(tmp_path):
    """PbrtLight keeps its 96 bytes; fov sits where pad2[0] was"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d\\n", '
                   'sizeof(PbrtLight), offsetof(PbrtLight, fov), offsetof(PbrtLight, world_to_light), offsetof(PbrtLight, pos), '
                   '(int)PBRT_LIGHT_PROJECTION, (int)PBRT_LIGHT_GONIOMETRIC); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    D = scenes.LIGHT_DTYPE
    assert got[:2] == [96, 88]
    assert D.itemsize == 96
    assert got == [D.itemsize, D.fields["fov"][1], D.fields["world_to_light"][1], D.fields["pos"][1], scenes.LIGHT_PROJECTION,
                   scenes.LIGHT_GONIOMETRIC]


def test_light_constructors_round_once():
    m = lm.rigid((1.0, 2.0, -0.5), 37.0, (0.3, -0.2, 1.5))
    p = scenes.projection_light(m, (2.0, 3.0, 4.0), 40.0)
    g = scenes.goniometric_light(m, (2.0, 3.0, 4.0))
    m64 = m.astype(np.float64)
    for l, kind in ((p, scenes.LIGHT_PROJECTION), (g, scenes.LIGHT_GONIOMETRIC)):
        assert l["type"] == kind and l["n_samples"] == 1 and l["prim"] == -1
        assert np.array_equal(l["pos"], m[:3, 3])
        assert np.array_equal(l["world_to_light"], np.linalg.inv(m64[:3, :3]).astype(np.float32).reshape(9))
    assert p["fov"] == np.float32(40.0) and g["fov"] == 0.0
    ident = scenes.goniometric_light(None, (1, 1, 1))
    assert np.array_equal(ident["world_to_light"], np.eye(3, dtype=np.float32).reshape(9)) and not ident["pos"].any()


# ---- the model against itself ----
def test_model_axis_lands_on_the_middle_of_the_map():
    for size in [(3, 5), (5, 3), (4, 4)]:
        model = lm.LightMapModel(lm.PROJECTION, lm.rigid((0.2, 1.0, 0.3), 65.0, (1, 2, 3)), (1, 1, 1), FOV, _map(*size, 3))
        axis = np.linalg.inv(model.w2l) @ np.array([0.0, 0.0, 1.0])  # light-space +z in the world
        wl, p = model.screen_point(axis[None])
        np.testing.assert_allclose(p[0], 0.0, atol=1e-6)
        st = (p[0] - model.sb[:2]) / (model.sb[2:] - model.sb[:2])
        np.testing.assert_allclose(st, (0.5, 0.5), atol=1e-6)
        np.testing.assert_allclose(model.projection(axis[None])[0], em.triangle(model.l0, np.array([0.5]), np.array([0.5]))[0], rtol=1e-5)


def test_model_corner_direction_has_cos_total_width():
    for size in [(3, 5), (5, 3), None]:
        model = lm.LightMapModel(lm.PROJECTION, None, (1, 1, 1), FOV, None if size is None else _map(*size, 3))
        corner = np.array([model.sb[2] / model.inv_tan, model.sb[3] / model.inv_tan, 1.0])
        w = corner / np.linalg.norm(corner)
        np.testing.assert_allclose(w[2], model.cos_total_width, rtol=1e-12)
        _, p = model.screen_point(w[None])
        np.testing.assert_allclose(p[0], model.sb[2:], rtol=1e-12)  # it projects onto the corner (max.x, max.y)
        # a hair inside it is lit, a hair outside it is dark
        assert model.projection((w * [1 - 1e-6, 1 - 1e-6, 1])[None]).any() and not model.projection((w * [1 + 1e-6, 1, 1])[None]).any()
        assert not model.projection(np.array([[0.0, 0.0, -1.0]])).any()  # behind the projector


def test_model_gonio_orientation_and_seam():
    rgb = lm.gentle_map(4, 8)
    model = lm.LightMapModel(lm.GONIOMETRIC, None, (1, 1, 1), 0.0, rgb)
    s, t = model.gonio_st(np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]]))
    np.testing.assert_allclose(t, [0.0, 1.0, 0.5, 0.5, 0.5], atol=1e-12)  # light-space +y is theta = 0: row 0
    np.testing.assert_allclose(s[2:], [0.0, 0.25, 0.5], atol=1e-12)       # phi = 0 at +x, growing towards +z
    # +y itself: t = 0 -> the bilinear blend of row 0 with row -1 (Repeat), weights 0.5 / 0.5
    top = model.scale(np.array([[1e-9, 1.0, 0.0]]))[0]
    np.testing.assert_allclose(top, 0.5 * (0.5 * (rgb[0, 0] + rgb[0, -1])) + 0.5 * (0.5 * (rgb[-1, 0] + rgb[-1, -1])), rtol=1e-6)
    # the seam: phi -> 0+ and phi -> 2 pi- give the same value
    eps = 1e-7
    a = model.scale(np.array([[1.0, 0.3, eps]]))[0]
    b = model.scale(np.array([[1.0, 0.3, -eps]]))[0]
    np.testing.assert_allclose(a, b, rtol=1e-6)
    assert abs(model.gonio_st(np.array([[1.0, 0.3, -eps]]))[0][0] - 1.0) < 1e-6  # ... from the other end of s


def test_model_sample_li_is_the_product():
    """D88: I * projection / d^2, not I / projection"""
    rgb = lm.gentle_map(3, 5)
    I = (2.0, 3.0, 4.0)
    model = lm.LightMapModel(lm.PROJECTION, None, I, FOV, rgb)
    p = np.array([[0.1, -0.05, 2.0]])
    wi, pdf, li = model.sample_li(p)
    v = model.projection(-wi)[0]
    np.testing.assert_allclose(li[0], np.array(I) * v / (p[0] @ p[0]), rtol=1e-12)
    assert pdf[0] == 1.0 and v.min() > 0.4


_CPP = r"""
#include <cstdio>
#include <vector>
#include "pbrt_hip.hpp"
int main() {
    const double l2w[16] = {1, 0, 0, 0.5, 0, 0, -1, 2.0, 0, 1, 0, -1.0, 0, 0, 0, 1};
    const float I[3] = {2.0f, 3.0f, 4.0f};
    const PbrtLight p = pbrt::projection_light(l2w, I, 45.0f), g = pbrt::goniometric_light(l2w, I);
    std::printf("%d %d %g %g %g %g %g %g %g\n", p.type, g.type, p.fov, p.pos[0], p.pos[1], p.pos[2], g.world_to_light[5], g.world_to_light[7], g.L[1]);
    void (pbrt::Scene::*set)(int32_t, const std::vector<float>&, int32_t, int32_t) = &pbrt::Scene::set_light_map;
    return set ? 0 : 1;
}
"""


def test_cpp_surface_compiles_pedantic(tmp_path):
    src = tmp_path / "lights.cpp"
    src.write_text(_CPP)
    exe = str(tmp_path / "lights_cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L" + LIB_DIR, "-lpbrt_hip", "-Wl,-rpath," + LIB_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    # the inverse of the rotation (rows y <-> -z) and the translation column as p_light
    assert out.stdout.split() == ["5", "6", "45", "0.5", "2", "-1", "1", "-1", "3"]
