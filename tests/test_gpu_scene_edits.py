"""The pbrt_hip_scene_set_* entry points as edits of a live scene, on an 8 x 8 film over a two-triangle floor: a refused
environment map leaves the render bit for bit as it was, a second map on a light gives the render of a fresh scene that was given
only that map (with and without the spatial light table built in between, which the edit drops), and every setter changes what
is rendered. The refused edits of the other five setters are held by test_gpu_glossy.py::test_roughness_refusals_leave_the_scene_unchanged,
test_gpu_bxdfs.py, test_gpu_disney.py and test_gpu_lobe_materials.py::test_refusals_leave_the_scene_unchanged, and
test_gpu_light_maps.py::test_set_light_map_twice_and_refusals.

edit_outputs() is what a comparison of two builds of the library dumps (PBRT_HIP_LIB names the build): the render and 64
BSDF queries after each of the six setters, and the hits of a two-level, a moving two-level and an instanced scene."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
import light_map_model as lm
import motion_cases as mc

W = H = 8
SPP = 4
MATTE = (scenes.MAT_MATTE, (0.5, 0.4, 0.3), (0, 0, 0), 1.0)
PLASTIC = scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.2)
SKY = (scenes.LIGHT_INFINITE, (1.0, 0.9, 0.8), -1, 0, 1)
LAMP_AT = lm.rigid((1.0, 0.0, 0.0), 180.0, (0.3, -0.2, 1.5))   # light-space +z looks down at the floor
_t, _s = np.meshgrid(np.arange(2), np.arange(4), indexing="ij")
MAP_A = np.stack([0.2 + 0.3 * _s, 1.5 - 0.25 * _s + 0.5 * _t, 0.4 + 0.8 * _t], axis=-1).astype(np.float32)   # 4 x 2 texels
MAP_B = np.ascontiguousarray(MAP_A[::-1, ::-1] * np.float32(2.5) + np.float32(0.1))
KINDS = ["environment", "projection", "goniometric"]


def _floor(light, rows=(MATTE,)):
    """the floor under `light` and a dim point light: two lights for the power and spatial distributions to choose from"""
    positions, indices = scenes._plane_z0(2.0)
    return dict(positions=positions, indices=indices, tri_material=np.zeros(2, np.int32), materials=scenes._materials(list(rows)),
                tri_light=np.full(2, -1, np.int32), lights=scenes._lights([light, scenes.point_light((0.5, 0.5, 2.0), (0.3, 0.3, 0.3))]))


def _lit_scene(kind):
    if kind == "environment":
        return _floor(SKY)
    return _floor(scenes.projection_light(LAMP_AT, (2.0, 3.0, 4.0), 60.0) if kind == "projection" else scenes.goniometric_light(LAMP_AT, (2.0, 3.0, 4.0)))


def _set_map(scene, kind, rgb):
    scene.set_environment_map(0, rgb) if kind == "environment" else scene.set_light_map(0, rgb)


def _render(scene, light_strategy=1):
    film, _ = scene.render(scenes.orthographic_camera((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, W, H), W, H, SPP, max_depth=2,
                           light_strategy=light_strategy, seed=5)
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    return film


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_refused_environment_map_leaves_the_render_unchanged(hip_ctx):
    scene = pbrt_hip.Scene(hip_ctx, _lit_scene("environment"))
    singular, bent, nan_map = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), MAP_B.copy()
    singular[2, :3] = singular[0, :3]
    bent[3, 2] = 0.5
    nan_map[1, 2, 1] = np.nan
    refused = [(1, MAP_B, None, "is not PBRT_LIGHT_INFINITE"), (2, MAP_B, None, "light index out of range"), (-1, MAP_B, None, "light index out of range"),
               (0, MAP_B, singular, "light_to_world is singular"), (0, MAP_B, bent, "last row"), (0, MAP_B, np.full((4, 4), np.nan, np.float32), "is not finite"),
               (0, nan_map, None, "texels must be finite"), (0, -MAP_B, None, "texels must be finite")]
    for mapped in (False, True):   # the constant light, then a light that has a map
        if mapped:
            scene.set_environment_map(0, MAP_A)
        before = [_render(scene, s) for s in (1, 2)]
        for light, rgb, m, why in refused:
            with pytest.raises(pbrt_hip.PbrtHipError, match=f"\\(1\\): pbrt_hip_scene_set_environment_map: .*{why}"):
                scene.set_environment_map(light, rgb, m)
        assert all(_same(b, _render(scene, s)) for b, s in zip(before, (1, 2)))
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spatial_between", [False, True], ids=["plain", "spatial_between"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_second_map_renders_as_on_a_fresh_scene(hip_ctx, kind, spatial_between):
    strategy = 2 if spatial_between else 1   # 2: SpatialLightDistribution, whose table the second edit drops; 1: the power distribution
    scene = pbrt_hip.Scene(hip_ctx, _lit_scene(kind))
    _set_map(scene, kind, MAP_A)
    first = _render(scene, strategy) if spatial_between else None
    _set_map(scene, kind, MAP_B)
    got = _render(scene, strategy)
    scene.close()
    fresh = pbrt_hip.Scene(hip_ctx, _lit_scene(kind))
    _set_map(fresh, kind, MAP_B)
    want = _render(fresh, strategy)
    fresh.close()
    assert _same(got, want)
    assert first is None or not _same(first, want)


# ---- what two builds of the library are compared on ----
def _query(scene, row):
    rng = np.random.default_rng(64)
    wo, wi = rng.normal(size=(64, 3)), rng.normal(size=(64, 3))
    wo[:, 2] = np.abs(wo[:, 2]) + 0.05
    q = scene.bsdf_query(row, wo / np.linalg.norm(wo, axis=1, keepdims=True), wi / np.linalg.norm(wi, axis=1, keepdims=True), rng.random((64, 2)))
    return {k: q[k] for k in sorted(q)}


MATERIAL_EDITS = {
    "roughness": lambda s: s.set_material_roughness(0, 0.35),
    "material": lambda s: s.set_material(0, scenes.substrate((0.5, 0.4, 0.3), (0.3, 0.3, 0.3), 0.2, 0.3)),
    "disney": lambda s: s.set_disney_material(0, scenes.disney((0.8, 0.5, 0.3), metallic=0.3, sheen=0.5, clearcoat=0.5, spec_trans=0.2)),
    "lobes": lambda s: (s.set_lobe_material(2, scenes.uber(kd=0.25, ks=0.25, kr=0.1)), s.set_lobe_material(0, scenes.mix(1, 2, 0.3))),
}


def edit_outputs(ctx):
    """{name: array} of everything the six setters and the two-level creation calls decide on these small scenes"""
    out = {}
    for name, edit in MATERIAL_EDITS.items():
        scene = pbrt_hip.Scene(ctx, _floor(SKY, (PLASTIC, MATTE, MATTE)))
        out[f"{name}/before"] = _render(scene)
        edit(scene)
        out[f"{name}/film"] = _render(scene)
        for k, v in _query(scene, 0).items():
            out[f"{name}/query/{k}"] = v
        scene.close()
    for kind in KINDS:
        scene = pbrt_hip.Scene(ctx, _lit_scene(kind))
        out[f"{kind}/before"] = _render(scene)
        for rgb, tag in ((MAP_A, "a"), (MAP_B, "b")):
            _set_map(scene, kind, rgb)
            for strategy in (1, 2):
                out[f"{kind}/film_{tag}{strategy}"] = _render(scene, strategy)
        for k, v in _query(scene, 0).items():
            out[f"{kind}/query/{k}"] = v
        scene.close()
    # two 2-triangle objects: a static, a moving and a one-aggregate scene
    floor = dict(zip(("positions", "indices"), scenes._plane_z0(3.0)), tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32))
    quads = (mc.QUAD, (mc.QUAD[0] * np.float32(0.5), mc.QUAD[1][::-1].copy()))
    placed = [(0, mc.tr(-1, 0, 1) @ mc.rot((0, 1, 0), 20), mc.tr(-1, 0.5, 1.5) @ mc.rot((0, 1, 0), 20)), (1, mc.tr(1, 0, 1) @ mc.rot((1, 0, 0), 30), None)]
    rays = mc.rays_at(np.array([[-1, 0.25, 1.25], [1, 0, 1], [0, 0, 0]], np.float64), 3, mc.some_times(4), spread=0.5, radius=5.0)[:512]
    cases = {"two_level": mc.make_scene(placed, world=floor, moving=False, objects=quads),
             "two_level_moving": mc.make_scene(placed, world=floor, moving=True, objects=quads),
             "instanced": dict(positions=mc.QUAD[0], indices=mc.QUAD[1], tri_material=np.zeros(2, np.int32), tri_light=np.full(2, -1, np.int32),
                               materials=scenes._materials(mc.MATERIALS), lights=scenes._lights([]), instance_material=np.full(2, -1, np.int32),
                               instances=mc.make_scene(placed, objects=quads)["instances"])}
    for name, sc in cases.items():
        scene = pbrt_hip.Scene(ctx, sc)
        hits = scene.intersect(rays)
        assert (hits["prim_id"] >= 0).sum() > 50, name
        out[f"{name}/hits"] = hits.view(np.uint8)
        out[f"{name}/shadow"] = scene.intersect_p(rays)
        scene.close()
    return out


@pytest.mark.gpu
def test_every_setter_changes_the_render(hip_ctx):
    out = edit_outputs(hip_ctx)
    for name in MATERIAL_EDITS:
        assert not _same(out[f"{name}/before"], out[f"{name}/film"]), name
        assert all(np.isfinite(v).all() for k, v in out.items() if k.startswith(f"{name}/query/")), name
    for kind in KINDS:
        films = [out[f"{kind}/before"]] + [out[f"{kind}/film_{tag}1"] for tag in "ab"]
        assert not any(_same(a, b) for i, a in enumerate(films) for b in films[:i]), kind
    assert not np.array_equal(out["two_level/hits"], out["two_level_moving/hits"])
