"""Moving instances on the host (pbrt-rs_amd/csrc/host_motion.cpp), no GPU: the float64 model is consistent with itself,
pbrt_hip_instance_motion_bounds holds the model's motion and is as tight as its construction says, and it refuses what the
header says it refuses.

The bound: a corner p moves on c(u) = T(u) + R(u) S(u) p with speed at most
L = |T1 - T0| + w max(|S0 p|, |S1 p|) + |(S1 - S0) p|, w = 2 theta on the slerp branch and 4 tan(theta / 2) on the normalised-lerp
branch; the box of the corner's positions at the ends of 32 segments, grown by L / 64, then padded by 16 * 2^-24 * max|coordinate|
and rounded outward to float."""
import os
import subprocess

import numpy as np
import pytest

import motion_model as mm
import pbrt_hip
from pbrt_hip import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ_MIN = np.array([-0.5, -0.3, -0.2], dtype=np.float32)
OBJ_MAX = np.array([0.6, 0.4, 0.3], dtype=np.float32)
N_TIMES = 4096


def rotation(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = np.radians(degrees) / 2
    m = np.eye(4)
    m[:3, :3] = mm.quat_to_matrix(np.concatenate([a * np.sin(h), [np.cos(h)]]))
    return m


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def scaling(x, y, z):
    return np.diag([x, y, z, 1.0])


def f32(m):
    return np.asarray(m, dtype=np.float32).astype(np.float64)


# name -> (start matrix, end matrix, rotates); the matrices are what the library is given: float32 values
CASES = {
    "translation": (f32(translation(0.2, -0.1, 0.3)), f32(translation(1.5, 0.7, -0.4)), False),
    # the same upper 3x3 at both ends: the two decompositions are the same numbers, r0 == r1 exactly
    "translation_of_rotated": (f32(rotation((1, 2, 3), 40) @ scaling(1.0, 0.5, 2.0)) + translation(0.2, -0.1, 0.3) - np.eye(4),
                               f32(rotation((1, 2, 3), 40) @ scaling(1.0, 0.5, 2.0)) + translation(-0.75, 0.5, 0.125) - np.eye(4), False),
    # a scale that changes under a fixed rotation: the two polar factors agree to rounding only, so this is a rotating case
    # for the library (on the normalised-lerp branch, with an angle of a few ulps)
    "scale_change": (f32(translation(0.2, -0.1, 0.3) @ rotation((1, 2, 3), 40) @ scaling(1.0, 0.5, 2.0)),
                     f32(translation(-0.3, 0.4, 0.1) @ rotation((1, 2, 3), 40) @ scaling(1.5, 0.75, 1.0)), None),
    "rotation_170": (f32(rotation((0.3, 1.0, 0.2), 10)), f32(rotation((0.3, 1.0, 0.2), 180)), True),
    "rotation_translation_scale": (f32(translation(0.5, 0.0, -0.2) @ rotation((1, 0.2, -0.4), -30) @ scaling(1.0, 0.7, 1.3)),
                                   f32(translation(-0.4, 0.9, 0.3) @ rotation((0.1, 1, 0.5), 75) @ scaling(1.6, 0.5, 0.9)), True),
    "normalised_lerp": (f32(translation(0.1, 0.2, 0.3) @ rotation((0, 0, 1), 10)), f32(translation(0.1, 0.2, 0.3) @ rotation((0, 0, 1), 13)), True),
}
T0, T1 = 0.25, 1.75


def instance_record(m0):
    inst = np.zeros(1, dtype=scenes.INSTANCE_DTYPE)
    inst["to_world"] = np.asarray(m0, dtype=np.float32).reshape(1, 16)
    inst["to_object"] = np.linalg.inv(np.asarray(m0, dtype=np.float64)).astype(np.float32).reshape(1, 16)
    inst["to_object"][0, 12:] = (0, 0, 0, 1)
    inst["material"] = -1
    return inst


def motion_record(m1, t0=T0, t1=T1):
    return np.array([scenes.instance_motion(m1, t0, t1)], dtype=scenes.INSTANCE_MOTION_DTYPE)


def corners():
    return np.array([[(OBJ_MAX if c & 1 else OBJ_MIN)[0], (OBJ_MAX if c & 2 else OBJ_MIN)[1], (OBJ_MAX if c & 4 else OBJ_MIN)[2]]
                     for c in range(8)], dtype=np.float64)


def sampled_corners(motion):
    """(N_TIMES, 8, 3): the model's corners at N_TIMES times over [T0, T1], both ends included"""
    times = np.linspace(T0, T1, N_TIMES)
    m = motion.interpolate(times)
    return np.einsum("nij,cj->nci", m[:, :3, :3], corners()) + m[:, None, :3, 3]


def speed_bound(motion):
    """max over the corners of L, from the model's own decomposition"""
    c = float(np.clip(np.dot(motion.q0, motion.q1), -1.0, 1.0))
    theta = np.arccos(c)
    omega = 4 * np.tan(theta / 2) if c > mm.SLERP_LERP_ABOVE else 2 * theta
    p = corners()
    s0, s1 = p @ motion.S0.T, p @ motion.S1.T
    L = (np.linalg.norm(motion.T1 - motion.T0) + omega * np.maximum(np.linalg.norm(s0, axis=1), np.linalg.norm(s1, axis=1)) +
         np.linalg.norm(s1 - s0, axis=1))
    return float(L.max())


@pytest.mark.parametrize("name", list(CASES))
def test_model_is_consistent(name):
    m0, m1, _ = CASES[name]
    motion = mm.Motion(m0, m1, T0, T1)
    # interpolate returns the stored matrices at and beyond the ends ...
    got = motion.interpolate(np.array([T0 - 1.0, T0, T1, T1 + 1.0]))
    assert np.array_equal(got[0], m0) and np.array_equal(got[1], m0) and np.array_equal(got[2], m1) and np.array_equal(got[3], m1)
    # ... and decompose-then-recompose gives the matrix back: T R S at u = 0 and u = 1
    # (the polar iteration converges quadratically and stops after a step of at most 1e-4: what is left of the rotation's
    # non-orthogonality, and with it of the round trip through the quaternion, is of the order of that step squared)
    tol = 10 * (1e-4) ** 2
    assert np.abs(motion.compose(np.float64(0.0)) - m0).max() < tol
    assert np.abs(motion.compose(np.float64(1.0)) - m1).max() < tol
    for q, s, m in ((motion.q0, motion.S0, m0), (motion.q1, motion.S1, m1)):
        r = mm.quat_to_matrix(q)
        assert abs(np.linalg.norm(q) - 1.0) < tol and np.abs(r @ r.T - np.eye(3)).max() < 4 * tol
        assert np.abs(r @ s - m[:3, :3]).max() < tol
    assert np.dot(motion.q0, motion.q1) >= 0.0
    # which slerp branch the case is on
    assert (np.dot(motion.q0, motion.q1) > mm.SLERP_LERP_ABOVE) == (name in ("translation", "translation_of_rotated", "scale_change", "normalised_lerp"))


@pytest.mark.parametrize("name", list(CASES))
def test_bounds_contain_the_motion(name):
    m0, m1, _ = CASES[name]
    lo, hi = pbrt_hip.instance_motion_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0), motion_record(m1))
    pts = sampled_corners(mm.Motion(m0, m1, T0, T1)).reshape(-1, 3)
    # Without rotation the bound is the union of the two pbrt_hip_instance_bounds boxes, whose corners are float32 sums of
    # three products and a translation (gamma_4 of the terms' magnitudes, each at most the box's largest coordinate): the
    # float64 corners may stand that far outside. With rotation the bound is padded and holds them outright.
    eps = 0.0 if CASES[name][2] is not False else 4 * 4 * 2.0 ** -24 * float(max(np.abs(lo).max(), np.abs(hi).max()))
    assert np.all(lo[0].astype(np.float64) <= pts.min(axis=0) + eps), (lo, pts.min(axis=0))
    assert np.all(hi[0].astype(np.float64) >= pts.max(axis=0) - eps), (hi, pts.max(axis=0))


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[2]])
def test_bounds_are_tight(name):
    m0, m1, _ = CASES[name]
    motion = mm.Motion(m0, m1, T0, T1)
    lo, hi = pbrt_hip.instance_motion_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0), motion_record(m1))
    pts = sampled_corners(motion).reshape(-1, 3)
    big = max(np.abs(lo).max(), np.abs(hi).max())
    # L / 64 from the construction (plus what 4096 samples can miss of the hull, L / 8190) is within L / 32; the padding is
    # 16 * 2^-24 * big and the outward rounding at most one more ulp (2^-23 * big)
    slack = speed_bound(motion) / 32 + 18 * 2.0 ** -24 * float(big)
    assert np.all(pts.min(axis=0) - lo[0] <= slack), (pts.min(axis=0) - lo[0], slack)
    assert np.all(hi[0] - pts.max(axis=0) <= slack), (hi[0] - pts.max(axis=0), slack)
    assert speed_bound(motion) > 0.03   # the case does move: the test above is not vacuous


@pytest.mark.parametrize("name", ["translation", "translation_of_rotated"])
def test_no_rotation_is_the_union_of_the_end_boxes(name):
    m0, m1, _ = CASES[name]
    motion = mm.Motion(m0, m1, T0, T1)
    lo, hi = pbrt_hip.instance_motion_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0), motion_record(m1))
    lo0, hi0 = pbrt_hip.instance_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0))
    lo1, hi1 = pbrt_hip.instance_bounds(OBJ_MIN, OBJ_MAX, instance_record(m1))
    if not np.array_equal(motion.q0, motion.q1):
        pytest.fail("the case's two rotations do not decompose to the same quaternion: it is not a no-rotation case")
    assert np.array_equal(lo, np.minimum(lo0, lo1)) and np.array_equal(hi, np.maximum(hi0, hi1))


def test_static_instance_is_instance_bounds():
    m0, m1, _ = CASES["rotation_170"]
    rec = motion_record(m1)
    rec["animated"] = 0
    rec["end_time"] = rec["start_time"]   # not read for a static instance
    lo, hi = pbrt_hip.instance_motion_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0), rec)
    lo0, hi0 = pbrt_hip.instance_bounds(OBJ_MIN, OBJ_MAX, instance_record(m0))
    assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0)


def test_refusals():
    m0, m1, _ = CASES["rotation_translation_scale"]
    ok = lambda inst, rec: pbrt_hip.instance_motion_bounds(OBJ_MIN, OBJ_MAX, inst, rec)
    ok(instance_record(m0), motion_record(m1))
    bad = m1.copy()
    bad[1, 2] = np.nan
    with pytest.raises(pbrt_hip.PbrtHipError):
        ok(instance_record(m0), motion_record(bad))
    bad = m1.copy()
    bad[0, 3] = np.inf
    with pytest.raises(pbrt_hip.PbrtHipError):
        ok(instance_record(m0), motion_record(bad))
    bad = m1.copy()
    bad[3] = (0, 0, 0.1, 1)
    with pytest.raises(pbrt_hip.PbrtHipError):
        ok(instance_record(m0), motion_record(bad))
    for t0, t1 in ((1.0, 1.0), (1.0, 0.5), (0.0, np.nan)):
        with pytest.raises(pbrt_hip.PbrtHipError):
            ok(instance_record(m0), motion_record(m1, t0, t1))
    singular = m1.copy()
    singular[:3, 2] = singular[:3, 1]   # two equal columns
    with pytest.raises(pbrt_hip.PbrtHipError):
        ok(instance_record(m0), motion_record(singular))
    inst = instance_record(m0)
    inst["to_world"] = singular.astype(np.float32).reshape(1, 16)
    with pytest.raises(pbrt_hip.PbrtHipError):
        ok(inst, motion_record(m1))
    with pytest.raises(pbrt_hip.PbrtHipError):   # one record per instance
        ok(instance_record(m0), np.zeros(2, dtype=scenes.INSTANCE_MOTION_DTYPE))


def test_struct_layout(tmp_path):
    d = scenes.INSTANCE_MOTION_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbrt_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(PbrtInstanceMotion), offsetof(PbrtInstanceMotion, end_to_world), offsetof(PbrtInstanceMotion, start_time), '
                   'offsetof(PbrtInstanceMotion, end_time), offsetof(PbrtInstanceMotion, animated), offsetof(PbrtInstanceMotion, pad)); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [d.itemsize] + [d.fields[k][1] for k in ("end_to_world", "start_time", "end_time", "animated", "pad")] == [80, 0, 64, 68, 72, 76]
    rec = scenes.instance_motion(np.eye(4), 0.5, 2.0)
    assert rec["animated"] == 1 and rec["start_time"] == 0.5 and rec["end_time"] == 2.0 and rec["end_to_world"][15] == 1.0


def test_gpu_ray_sets_stay_within_the_exclusion_cap():
    """The ray sets of tests/test_gpu_motion.py, through the model alone: at most 2 % of the rays hang on a margin of 1e-4 and are
    left out there, and every instance keeps enough hits."""
    import test_gpu_motion as g
    rays = g.rays_at(g.CENTRES, 7, g.some_times(6))
    m = g.model_hits(g.FIVE, rays)
    assert m["unsure"].mean() <= 0.02
    for i in range(5):
        assert ((m["inst"] == i) & ~m["unsure"]).sum() > 200, i
    spin = [(0, g.rot((0.2, 0.1, 1.0), 0), g.rot((0.2, 0.1, 1.0), 120))]
    m = g.model_hits(spin, g.rays_at(np.zeros((1, 3)), 8, g.some_times(9), spread=0.35), objects=(g.BOX,))
    assert m["unsure"].mean() <= 0.02 and (m["hit"] & ~m["unsure"]).sum() > 2000
