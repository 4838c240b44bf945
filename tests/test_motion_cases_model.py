"""tests/motion_cases.py held to the float64 model, without a GPU: what test_gpu_motion_paths.py expects of the device is itself
what the model says, every case exercises what it is there for, and every cap and floor holds.

Measured here (numpy, float64):
  path_time_case       4 of 4096 rays within 1e-3 of the occluder's edge (cap 2 %); covered at their own time but not at the start /
                       the other way round: mirror 250 / 248, two mirrors 283 / 232, pane 260 / 257 (floor 100 each)
  lambert_case         1 of 4096 rays excluded (cap 2 %), 1250 lit hits; the normal through M moves all 1250 by more than the allowance
  aniso_case           kept metal 1198, disney 1153 (floor 800; model value >= 1e-3); the normal through M and dpdu left in object
                       space each move 100 % of them by more than 4 times the recorded baseline (1.4e-5 and 1.8e-5)
  shadow_start_case    0 of 4096 rays excluded (cap 2 %); 471 dark and 3403 lit points of the plane, 202 lit hits on the box
  depth_case           26 (two objects) and 30 (one object) of 4096 rays excluded (cap 2 %); hits on negated-quaternion /
                       normalised-lerp / scaled instances 530 / 591 / 509 and 430 / 484 / 533 (floor 50 each)
"""
import numpy as np
import pytest

import closed_forms_samplers as cs
import motion_cases as mc
import motion_model as mm
import pbrt_hip


# ---------------------------------------------------------------------------------------------------------------------
# 1. time stays with its path
# ---------------------------------------------------------------------------------------------------------------------
def test_path_time_chains_are_the_classes_they_are_meant_to_be():
    case = mc.path_time_case()
    cls, chains = case["cls"], case["chains"]
    for i, chain in enumerate(chains):
        prefix = mc.CHAIN_PREFIX[cls[i]]
        assert chain[:-1] == prefix, (i, cls[i], chain)
        assert chain[-1] == ("nothing" if cls[i] == 0 else "occluder" if case["covered"][i] else "emitter"), (i, chain)
    # the pane's reflect branch ends on the second emitter whatever the time: only the transmit branch depends on it
    for i in np.flatnonzero(cls == 3):
        assert case["reflected"][i] == ["pane", "second_emitter"], (i, case["reflected"][i])
    excluded = 1.0 - case["keep"].mean()
    print(f"path_time_case: {(~case['keep']).sum()} of {len(cls)} rays within {mc.EDGE} of the occluder's edge")
    assert excluded <= mc.MAX_EXCLUDED
    assert len(np.unique(case["rays"]["time"])) == 8
    for k in (1, 2, 3):
        sure = (cls == k) & case["keep"] & case["keep_at_start"]
        on, off = (sure & case["covered"] & ~case["covered_at_start"]).sum(), (sure & ~case["covered"] & case["covered_at_start"]).sum()
        print(f"    {mc.CLASSES[k]}: covered at their own time but not at the start {on}, the other way round {off}")
        assert on >= mc.MIN_SWITCHED and off >= mc.MIN_SWITCHED, (k, on, off)
    # the classes are interleaved: no run of one class longer than a wave
    runs = np.diff(np.flatnonzero(np.diff(cls) != 0))
    assert runs.max() < 32


def test_path_time_static_scenes_cover_every_chain_or_none():
    """the chains traced against the two static occluders: covered for every ray that reaches the plane / for none"""
    case = mc.path_time_case()
    rays = case["rays"]
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    reach = case["cls"] != 0
    for name, want in (("covers", True), ("away", False)):
        inst = mc.OCCLUDER_COVERS if name == "covers" else mc.OCCLUDER_AWAY
        chains, near = mc.trace_chain(o, d, np.zeros(len(o)), mc.model_instances(inst, (mc.QUAD,))[0][0])
        assert not near.any()
        assert np.array_equal(np.array([c[-1] == "occluder" for c in chains]), reach & want), name


def test_path_time_scenes_share_one_world_bound():
    case = mc.path_time_case()
    roots = [pbrt_hip.build_general_two_level(case[k])[2][0] for k in ("moving", "covers", "away")]
    for r in roots[1:]:
        assert np.array_equal(r["bmin"], roots[0]["bmin"]) and np.array_equal(r["bmax"], roots[0]["bmax"])
    assert np.array_equal(roots[0]["bmin"], np.full(3, -mc.FAR, np.float32)) and np.array_equal(roots[0]["bmax"], np.full(3, mc.FAR, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. rows under scale and shear
# ---------------------------------------------------------------------------------------------------------------------
def test_row_instances_scale_shear_and_turn():
    for k, m0, m1 in mc.ROW_INSTANCES:
        for m in (m0, m1):
            a = m[:3, :3]
            assert not np.allclose(a @ a.T, np.eye(3) * (a @ a.T)[0, 0], atol=1e-3)   # no rotation times a uniform scale
    # the third one shears: its polar factor S is not diagonal
    s0, s1 = mm.decompose(mc.ROW_INSTANCES[2][1])[2], mm.decompose(mc.ROW_INSTANCES[2][2])[2]
    assert np.abs(s0 - np.diag(np.diag(s0))).max() > 0.05 and np.abs(s1 - np.diag(np.diag(s1))).max() > 0.05
    assert {k for k, _, _ in mc.ROW_INSTANCES} == {0, 1}


def test_lambert_case_tells_the_inverse_transpose_from_the_matrix():
    case = mc.lambert_case()
    keep = ~case["m"]["unsure"]
    lit = keep & (case["expect"] > 0.05)
    wrong = mc.lambert_case("normal_through_m")
    moved = np.abs(wrong["expect"] - case["expect"]) > case["tol"]
    print(f"lambert_case: {(~keep).sum()} of {len(keep)} rays excluded, {lit.sum()} lit hits, {(moved & lit).sum()} moved by the normal through M")
    assert 1.0 - keep.mean() <= mc.MAX_EXCLUDED
    assert lit.sum() > 800
    for i in range(3):
        assert (lit & (case["m"]["inst"] == i)).sum() > 100, i
    assert (moved & lit).sum() > 0.5 * lit.sum()
    assert case["tol"].max() < 10 * mc.NORMAL_TOL and case["tol"][case["m"]["hit"]].min() > 1.2 * mc.NORMAL_TOL


@pytest.mark.parametrize("name", list(mc.ANISO_ROWS))
def test_aniso_case_keeps_enough_rays_and_reads_both_sets_of_rows(name):
    case = mc.aniso_case(name)
    keep, ref = case["keep"], case["ref"]
    allow = 4.0 * mc.ANISO_BASELINE_RECORDED[name]
    print(f"aniso_case {name}: {keep.sum()} rays kept (floor {mc.MIN_KEPT}), model value >= {mc.ANISO_FLOOR}")
    assert keep.sum() >= mc.MIN_KEPT
    assert (ref[keep].max(axis=1) >= mc.ANISO_FLOOR).all()
    for variant in mm.FRAME_VARIANTS[1:]:
        wrong = mc.aniso_case(name, variant)["ref"]
        moved = mc.aniso_error(wrong, ref, keep) > allow
        print(f"    {variant}: moves {moved.mean():.0%} of the kept rays by more than {allow:.1e}")
        assert moved.mean() > 0.5, variant


def test_shadow_start_case():
    case = mc.shadow_start_case()
    keep = case["keep"]
    dark, lit_plane = keep & case["dark"], keep & case["on_plane"] & ~case["dark"]
    lit_box = keep & case["on_box"] & (case["lambert"] > 0.05)
    print(f"shadow_start_case: {(~keep).sum()} of {len(keep)} rays excluded; {dark.sum()} dark and {lit_plane.sum()} lit points of the "
          f"plane, {lit_box.sum()} lit hits on the box")
    assert 1.0 - keep.mean() <= mc.MAX_EXCLUDED
    assert dark.sum() > 300 and lit_plane.sum() > 1500 and lit_box.sum() > 150
    # the shadow does move: points that are dark at their time and would be lit with the box at its start, and the other way round
    rays = case["rays"]
    at_start = mm.closest_hits(mc.model_instances(mc.STAND_BOX), rays["o"].astype(np.float64) + rays["d"].astype(np.float64) *
                               ((mc.STAND_Z - rays["o"][:, 2].astype(np.float64)) / rays["d"][:, 2].astype(np.float64))[:, None],
                               np.broadcast_to(mc.STAND_WI, (len(rays), 3)), np.full(len(rays), np.inf), np.full(len(rays), mc.T0))
    assert (dark & ~at_start["hit"]).sum() > 100 and (lit_plane & at_start["hit"]).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", [2, 1])
def test_depth_case(n_objects):
    case = mc.depth_case(n_objects)
    inst, kinds, m = case["instances"], case["kinds"], case["m"]
    assert len(inst) == 64 and [int((kinds == k).sum()) for k in range(5)] == [8, 8, 8, 8, 32]
    assert {k for k, _, _ in inst} == set(range(n_objects))
    for (k, m0, m1), kind in zip(inst, kinds):
        if kind == 3:
            assert m1 is None
            continue
        dot = mc.quat_dot(m0, m1)
        if kind == 0:
            assert dot < -0.05                                    # negated by the host (and by mm.Motion)
        elif kind == 1:
            assert abs(dot) > mm.SLERP_LERP_ABOVE + 1e-4          # the normalised-lerp branch (after the negation), in float32 as well
        else:
            assert 0.05 < abs(dot) < mm.SLERP_LERP_ABOVE - 1e-4   # the sign is matrix_to_quat's choice of root: either way slerp proper
        if kind == 2:
            s0, s1 = np.linalg.svd(m0[:3, :3])[1], np.linalg.svd(m1[:3, :3])[1]
            assert s0.max() / s0.min() > 1.5 and s1.max() / s1.min() > 1.5
    keep = ~m["unsure"]
    sel = keep & m["hit"]
    counts = [int((kinds[m["inst"][sel]] == k).sum()) for k in range(3)]
    print(f"depth_case({n_objects}): {(~keep).sum()} of {len(keep)} rays excluded, hits on negated / nlerp / scaled instances {counts}")
    assert 1.0 - keep.mean() <= mc.MAX_EXCLUDED
    assert min(counts) >= mc.MIN_KIND_HITS
    # the boxes overlap: most rays meet the bounds of several instances (here: of the model's motion at the ray's time)
    o, d = case["rays"]["o"].astype(np.float64), case["rays"]["d"].astype(np.float64)
    entered = np.zeros(len(o), int)
    for mo, pos, _ in mc.model_instances(inst, case["objects"]):
        oo, od = mm._object_rays(mo, o, d, case["rays"]["time"].astype(np.float64))
        lo, hi = np.asarray(pos, np.float64).min(axis=0), np.asarray(pos, np.float64).max(axis=0)
        hi = np.maximum(hi, lo + 1e-6)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - oo) / od, (hi - oo) / od
        entered += np.minimum(t0, t1).max(axis=1) <= np.maximum(t0, t1).min(axis=1)
    assert np.median(entered) >= 3
    # no ray meets the world triangles that make the two-object scene one with world triangles
    if case["world"] is not None:
        w = case["world"]
        far = mm.closest_hits([(mm.Motion(np.eye(4)), w["positions"], w["indices"])], o, d, case["rays"]["t_max"], case["rays"]["time"].astype(np.float64))
        assert len(w["indices"]) == 2 and not far["hit"].any() and not far["unsure"].any()
    # a top-level tree of at least five levels
    tree = pbrt_hip.build_general_two_level(mc.make_scene(inst, world=case["world"], objects=case["objects"]))[2]

    def depth(i):
        return 1 if tree[i]["n_primitives"] else 1 + max(depth(i + 1), depth(int(tree[i]["offset"])))
    assert depth(0) >= 5


# ---------------------------------------------------------------------------------------------------------------------
# 4. the ends
# ---------------------------------------------------------------------------------------------------------------------
def test_end_times_and_static_rows():
    t = mc.end_times()
    assert t[0] < t[1] == np.float32(mc.T0) < t[2] and t[3] < t[4] == np.float32(mc.T1) < t[5]
    assert len(np.unique(t)) == 6
    moving, start, end = (mc.end_scene(k) for k in ("moving", "start", "end"))
    assert "instance_motion" not in start and "instance_motion" not in end
    assert np.array_equal(start["instances"], moving["instances"])
    for i, (_, m0, m1) in enumerate(mc.FIVE):
        want = m0 if m1 is None else m1
        assert np.array_equal(end["instances"][i, 0], np.asarray(want, np.float32))
        assert np.allclose(end["instances"][i, 1].astype(np.float64) @ mc.f32(want), np.eye(4), atol=1e-6)
        assert not np.signbit(end["instances"][i][end["instances"][i] == 0]).any()
    roots = [pbrt_hip.build_general_two_level(s)[2][0] for s in (moving, start, end)]
    for r in roots[1:]:
        assert np.array_equal(r["bmin"], roots[0]["bmin"]) and np.array_equal(r["bmax"], roots[0]["bmax"])
    # the model returns the stored matrices at the ends and has no jump just inside them
    for mo, _, _ in mc.model_instances(mc.FIVE):
        if not mo.animated:
            continue
        a = mo.interpolate(t.astype(np.float64))
        assert np.array_equal(a[0], mo.m0) and np.array_equal(a[1], mo.m0) and np.array_equal(a[4], mo.m1) and np.array_equal(a[5], mo.m1)
        assert np.abs(a[2] - mo.m0).max() < 1e-5 and np.abs(a[3] - mo.m1).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Halton sampler's time dimension
# ---------------------------------------------------------------------------------------------------------------------
def test_scrambled_radical_inverse():
    i = np.arange(3000)
    assert np.allclose(mc.scrambled_radical_inverse(5, range(5), i), cs.radical_inverse(5, i), atol=1e-15)   # perm[0] = 0: the plain one
    # by hand: 7 = 12 in base 5, digits 2 then 1, then zeros for ever: perm[2] / 5 + perm[1] / 25 + perm[0] (1 / 125 + 1 / 625 + ...)
    assert abs(mc.scrambled_radical_inverse(5, (2, 0, 4, 1, 3), np.array([7]))[0] - (4 / 5 + 0 / 25 + 2 / 100)) < 1e-15
    rng = np.random.default_rng(5)
    for _ in range(4):
        p = rng.permutation(5)
        u = mc.scrambled_radical_inverse(5, p, i)
        assert np.all(u >= 0.0) and np.all(u <= 1.0)
        assert mc.halton_time_permutation(i, u) == [tuple(p)]


# ---------------------------------------------------------------------------------------------------------------------
# 6. material levels
# ---------------------------------------------------------------------------------------------------------------------
def test_level_scenes_add_one_level_at_a_time():
    for level in (1, 2, 3):
        old, new = mc.level_scenes(level)
        assert "instance_motion" not in old and new["instance_motion"] == {}
        used = set(old["instance_material"]) | set(old["world"]["tri_material"])
        types = {int(old["materials"][r]["type"]) for r in used}
        assert {mc.scenes.MAT_PLASTIC, mc.scenes.MAT_METAL} & types
        assert ("material_descs" in old) == (level >= 2) and ("disney_descs" in old) == (level >= 3)
        for key in ("material_descs", "disney_descs"):
            assert set(old.get(key, {})) <= used, (level, key)
            assert old.get(key) == new.get(key)
        assert np.array_equal(old["instance_material"], new["instance_material"])
