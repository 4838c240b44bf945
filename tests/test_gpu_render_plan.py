"""The render's host half (host_render.cpp: plan_render) and its device half (render.hip: RenderJob) together, and the entry
points that stage host pointers, on a 33 x 17 film of the Cornell box: whatever size a pass has and however its paths are laid
out over the waves, the box-filtered film is the same bits (test_gpu_render.py::test_samples_per_wave_is_only_a_layout holds the
layouts at larger sizes and under every sampler; here the film is no multiple of the tile, the window is cropped and the last
pass is uneven), and every output is finite. What the plan computes is checked without a GPU by tests/test_render_plan_host.py.

render_outputs() is what a comparison of two builds of the library dumps (PBRT_HIP_LIB names the build): films under every
integrator and sampler, a tile share, a batch of pbrt_hip_li, the exported camera rays, the point queries and a batch of
pbrt_hip_intersect / pbrt_hip_intersect_p. The wide filter's film ("filter") is splatted with float atomics and is the one
output that may differ in its last bits between two runs of one build."""
import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
from test_gpu_curves import STRIP_CP, curve_scene

W, H = 33, 17
CROP = (5, 3, 30, 16)
PATH, DIRECT, WHITTED, AO = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED, pbrt_hip.INTEGRATOR_AO
SAMPLERS = {"random": None, "stratified": ("stratified", 2, 2, True, 4), "zerotwo": ("zerotwo", 4), "halton": ("halton",)}


def _cornell():
    """the Cornell box with a point light beside its two emitting triangles, which take 4 and 9 samples (UniformSampleAll)"""
    sc = scenes.cornell_box()
    sc["lights"] = np.concatenate([sc["lights"], scenes._lights([scenes.cornell_delta_lights()[0]])])
    sc["lights"]["n_samples"][:2] = (4, 9)
    return sc


def _directions(n, seed):
    rng = np.random.default_rng(seed)
    wo, wi = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    wo[:, 2] = np.abs(wo[:, 2]) + 0.05
    return wo / np.linalg.norm(wo, axis=1, keepdims=True), wi / np.linalg.norm(wi, axis=1, keepdims=True), rng.random((n, 2)), rng.random(n) * 2 - 1


def _valid_camera_rays(scene, cam, w, h, spp, **kw):
    """the exported camera rays of the pixels inside the bounds (a tile's other slots carry pixel (-1, -1) and nothing else)"""
    rays, keys, p_film, pixel_sample = scene.camera_rays(cam, w, h, spp, **kw)
    inside = pixel_sample[:, 0] >= 0
    return rays[inside], keys[inside], p_film[inside], pixel_sample[inside]


def render_outputs(ctx):
    """{name: array} of a fixed set of small calls through every entry point that plans a render or stages host pointers"""
    out = {}
    cam = scenes.cornell_camera(W, H)
    scene = pbrt_hip.Scene(ctx, _cornell())
    film = lambda spp, **kw: scene.render(cam, W, H, spp, **dict(dict(max_depth=3, seed=9), **kw))[0]
    for spw in (1, 4):
        out[f"path/pass3_spw{spw}"] = film(4, spp_per_pass=3, samples_per_wave=spw)
    out["path/crop"] = film(4, bounds=CROP, spp_per_pass=3)
    for name, integrator in (("path", PATH), ("direct", DIRECT), ("whitted", WHITTED), ("ao", AO)):
        out[f"{name}/film"] = film(4, integrator=integrator, ao_samples=6)
    for name, sampler in SAMPLERS.items():
        out[f"sampler/{name}"] = film(3, sampler=sampler)
        out[f"sampler/{name}/direct_all"] = film(3, sampler=sampler, integrator=DIRECT, light_strategy=0)   # arrays of 4 and 9 (or 16)
        out[f"sampler/{name}/ao"] = film(3, sampler=sampler, integrator=AO, ao_samples=6)
    out["filter"] = film(4, filter=pbrt_hip.filter_table("gaussian", 2.0, 2.0, 2.0))
    out["rank1of2"] = film(4, tile_rank=1, tile_world=2)
    for strategy in (0, 1, 2):
        out[f"path/light_strategy{strategy}"] = film(4, light_strategy=strategy)
    rays, keys, p_film, pixel_sample = _valid_camera_rays(scene, cam, W, H, 2, seed=9)
    out["camera_rays/rays"], out["camera_rays/keys"], out["camera_rays/p_film"], out["camera_rays/pixel_sample"] = rays.view(np.uint8), keys, p_film, pixel_sample
    for name, integrator in (("path", PATH), ("direct", DIRECT)):
        out[f"li/{name}"] = scene.li(rays[:300], keys[:300], integrator=integrator, max_depth=3)[0]
    batch = _valid_camera_rays(scene, scenes.cornell_camera(32, 32), 32, 32, 1, seed=3)[0][:1000]
    hits = scene.intersect(batch)
    assert len(batch) == 1000 and (hits["prim_id"] >= 0).sum() > 900
    out["intersect"], out["intersect_p"] = hits.view(np.uint8), scene.intersect_p(batch)
    # the point queries: a matte, a Disney and a lobe row; an area light with u, the point light without
    wo, wi, u, h = _directions(64, 64)
    scene.set_disney_material(1, scenes.disney((0.8, 0.5, 0.3), metallic=0.3, sheen=0.5, clearcoat=0.5, spec_trans=0.2))
    scene.set_lobe_material(2, scenes.uber(kd=0.25, ks=0.25, kr=0.1))
    for row, name in enumerate(("plain", "disney", "lobes")):
        for k, v in scene.bsdf_query(row, wo, wi, u).items():
            out[f"bsdf_query/{name}/{k}"] = v
    p = np.random.default_rng(7).random((64, 3)) * 500.0 + 20.0
    for name, q in (("area", scene.light_sample_li(0, p, u)), ("point", scene.light_sample_li(2, p))):
        out[f"light_sample_li/{name}/wi"], out[f"light_sample_li/{name}/pdf"], out[f"light_sample_li/{name}/li"] = q
    scene.close()
    grey = (scenes.MAT_MATTE, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)
    strand = curve_scene([scenes.curve(STRIP_CP, 0.5, 0.5, type="flat", material=1, split_depth=0)], materials=scenes._materials([grey, grey]))
    strand["hair_descs"] = {1: scenes.hair(eumelanin=1.3)}
    scene = pbrt_hip.Scene(ctx, strand)
    for k, v in scene.bsdf_query_hair(1, h, wo, wi, u).items():
        out[f"bsdf_query/hair/{k}"] = v
    scene.close()
    return out


@pytest.mark.gpu
def test_render_outputs_are_finite(hip_ctx):
    out = render_outputs(hip_ctx)
    for name, v in out.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), name
    for name in ("path/film", "direct/film", "whitted/film", "ao/film", "filter", "rank1of2", "li/path", "li/direct"):
        assert out[name].max() > 0, name
    assert out["path/pass3_spw1"].tobytes() == out["path/pass3_spw4"].tobytes() == out["path/film"].tobytes()
    inside = np.zeros((H, W), bool)
    inside[CROP[1]:CROP[3], CROP[0]:CROP[2]] = True
    assert out["path/crop"][inside].tobytes() == out["path/film"][inside].tobytes() and not out["path/crop"][~inside].any()
    assert len(out["camera_rays/keys"]) == W * H * 2


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", [PATH, DIRECT], ids=["path", "direct"])
def test_film_does_not_depend_on_pass_size_or_layout(hip_ctx, integrator):
    """spp 4 in passes of 1, 3 (an uneven last pass) and 4 samples, a wave as 64 pixels of one sample or 16 pixels of four: one film"""
    scene = pbrt_hip.Scene(hip_ctx, _cornell())
    cam = scenes.cornell_camera(W, H)
    films = {(per_pass, spw): scene.render(cam, W, H, 4, integrator=integrator, max_depth=3, seed=9, bounds=CROP, spp_per_pass=per_pass, samples_per_wave=spw)[0]
             for per_pass in (1, 3, 4) for spw in (1, 4)}
    scene.close()
    ref = films[(4, 1)]
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    for key, f in films.items():
        assert f.tobytes() == ref.tobytes(), key
