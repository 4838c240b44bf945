"""The path integrator's transient records (rays, hit records, pending direct-lighting estimate) live at the path's POSITION in
the shade queue, not at its path number (wf_state.h): every bounce hands them to a new index, through LDS staging and two
generations of buffers. These are the shapes at which that indexing can go wrong, small enough to run in a second each.

Every case is held to the CPU oracle as tests/test_gpu_render.py holds its cases (equal filter-weight sums, per-pixel
|gpu - cpu| <= 1e-5 * max(1, |cpu|), RMSE <= 1e-6: every hit decision and random draw matches, only the order of the float
additions inside a pixel may differ in the last bit) with equal closest-hit and shadow ray counts, and the film must be the
SAME BITS whatever visits the queue in another order or numbers the paths differently: shade_order 0 / 1 / 2, ray_order
0 / 1, samples_per_wave 1 / default.
"""
import numpy as np
import pytest

import oracle
import pbrt_hip
from pbrt_hip import scenes

from glossy_cases import _with_glossy_rows

pytestmark = pytest.mark.gpu

TOL_PIXEL = 1e-5
TOL_RMSE = 1e-6

VARIANTS = [dict(shade_order=1), dict(shade_order=2), dict(ray_order=1), dict(samples_per_wave=1),
            dict(shade_order=1, ray_order=1, samples_per_wave=1), dict(shade_order=2, samples_per_wave=1)]


def _compare(film_gpu, film_cpu):
    assert np.array_equal(film_gpu[..., 3], film_cpu[..., 3]), "filter weight sums differ"
    rgb_g, rgb_c = pbrt_hip.film_to_rgb(film_gpu), oracle.film_to_rgb(film_cpu)
    err = np.abs(rgb_g - rgb_c)
    rmse = float(np.sqrt(np.mean((rgb_g.astype(np.float64) - rgb_c) ** 2)))
    assert np.all(err <= TOL_PIXEL * np.maximum(1.0, np.abs(rgb_c))), f"max err {err.max()} rmse {rmse}"
    assert rmse <= TOL_RMSE


def _check(hip_ctx, sc, cam, w, h, spp, oracle_kw=None, **kw):
    """Oracle parity of the default render, then the same bits and ray counts from every variant."""
    osc = oracle.OracleScene(sc)
    film_c, st_c = osc.render(scenes.camera_dict_to_floats(cam), w, h, spp, **(kw if oracle_kw is None else oracle_kw))
    osc.close()
    g = pbrt_hip.Scene(hip_ctx, sc)
    film, st = g.render(cam, w, h, spp, **kw)
    _compare(film, film_c)
    assert st["rays_closest"] + st["rays_shadow"] == st_c["rays"]
    assert st["camera_samples"] == st_c["camera_samples"]
    assert oracle.film_to_rgb(film_c).mean() > 0.01
    for v in VARIANTS:
        f, s = g.render(cam, w, h, spp, **kw, **v)
        assert f.tobytes() == film.tobytes(), v
        assert (s["rays_closest"], s["rays_shadow"]) == (st["rays_closest"], st["rays_shadow"]), v
    g.close()
    return st


def _thinning_scene():
    return scenes.random_triangles(20_000, seq=5, size=0.05)


def test_queue_thins_every_bounce(hip_ctx):
    """(a) Matte triangles under a constant environment light, 40 x 24 pixels x 8 spp at depth 8: the pixel bounds cut the
    16 x 16 tiles, so placeholder paths sit in the first queue; paths escape at every bounce, the survivors of one block
    land in two blocks of the next launch and the last block of every later launch is ragged."""
    w, h, spp = 40, 24, 8
    st = _check(hip_ctx, _thinning_scene(), scenes.random_triangles_camera(w, h), w, h, spp, max_depth=8, seed=11)
    assert st["camera_samples"] == w * h * spp and st["rays_shadow"] > 0


def test_generations_reused_across_ragged_passes(hip_ctx):
    """(b) The same frame in passes of 3, 3 and 2 samples: both generations of the buffers are reused, whichever was
    current when a pass ended, and a shorter pass follows a longer one. The oracle has no passes: one film for all."""
    w, h, spp = 40, 24, 8
    kw = dict(max_depth=8, seed=11)
    _check(hip_ctx, _thinning_scene(), scenes.random_triangles_camera(w, h), w, h, spp, oracle_kw=kw, spp_per_pass=3, **kw)
    g = pbrt_hip.Scene(hip_ctx, _thinning_scene())
    one, st_one = g.render(scenes.random_triangles_camera(w, h), w, h, spp, **kw)
    three, st_three = g.render(scenes.random_triangles_camera(w, h), w, h, spp, spp_per_pass=3, **kw)
    g.close()
    assert one.tobytes() == three.tobytes()
    assert (st_one["rays_closest"], st_one["rays_shadow"]) == (st_three["rays_closest"], st_three["rays_shadow"])


def test_area_light_mis_reads_ray_and_barycentrics_at_the_slot(hip_ctx):
    """(c) Cornell box: a MIS ray that reaches the emitter has its direction and the hit's barycentrics read back in
    estimate_direct_resolve, at the record index the previous launch wrote them to."""
    w, h = 40, 36
    _check(hip_ctx, scenes.cornell_box(), scenes.cornell_camera(w, h), w, h, 6, max_depth=8, light_strategy=1, seed=13)


def test_specular_bounces_hold_a_slot_with_one_ray(hip_ctx):
    """(d) Mirror and glass beside matte, area lights and an environment: a specular bounce has no pending estimate, its
    path holds a slot with the continuation ray only, next to paths with all three rays."""
    w, h = 40, 24
    _check(hip_ctx, scenes.mixed_materials_scene(), scenes.random_triangles_camera(w, h), w, h, 8, max_depth=12,
           light_strategy=1, seed=17)


def test_two_level_hits_use_their_second_float4(hip_ctx):
    """(e) Instances: the hit record's second float4 (the instance slot) is written and read at the slot as well."""
    w, h = 40, 24
    sc = scenes.instanced_scene(1500, 60, extent=1.2, tri_size=0.08)   # dense enough for 4 rays per camera sample
    _check(hip_ctx, sc, scenes.instanced_camera(w, h, 1.2), w, h, 6, max_depth=8, light_strategy=1, seed=19)


def test_glossy_instantiations(hip_ctx):
    """(f) Plastic and metal beside matte, mirror and glass: k_shade<*, GLOSSY> stages and flushes the same records."""
    w, h = 40, 24
    sc = _with_glossy_rows(scenes.mixed_materials_scene())
    tm = sc["tri_material"].copy()
    tm[:20000] = np.arange(20000) % 5   # matte, mirror, glass, plastic, metal
    sc["tri_material"] = tm
    _check(hip_ctx, sc, scenes.random_triangles_camera(w, h), w, h, 6, max_depth=8, light_strategy=1, seed=23)


def test_li_batch_that_is_no_multiple_of_256(hip_ctx):
    """(g) pbrt_hip_li on 3001 rays: generation 0 comes from k_li_generate (padding entries included), the radiance is the
    oracle's li within the render tests' per-value bound, with equal ray counts."""
    sc = _thinning_scene()
    n = 3001
    rays = scenes.random_rays(n, 29, origin_extent=1.2)
    keys = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(777)
    osc = oracle.OracleScene(sc)
    g = pbrt_hip.Scene(hip_ctx, sc)
    cpu, st_c = osc.li(rays, keys, max_depth=8, draws_before_li=5)
    gpu, st_g = g.li(rays, keys, max_depth=8, draws_before_li=5)
    assert st_g["rays_closest"] + st_g["rays_shadow"] == st_c["rays"]
    assert np.all(np.abs(gpu - cpu) <= TOL_PIXEL * np.maximum(1.0, np.abs(cpu))), np.abs(gpu - cpu).max()
    assert cpu.max() > 0.01
    again, st_again = g.li(rays, keys, max_depth=8, draws_before_li=5)   # the buffers come back from the cache, swapped or not
    assert again.tobytes() == gpu.tobytes()
    assert (st_again["rays_closest"], st_again["rays_shadow"]) == (st_g["rays_closest"], st_g["rays_shadow"])
    g.close()
    osc.close()


def test_sorted_ray_queue_carries_slot_tokens(hip_ctx):
    """Only queues of >= 2^20 rays are put into Morton order, and only from the second bounce on: the one size in this file
    at which the trace queue the traversal kernel reads is a sorted copy of slot tokens. Far too many paths for the oracle in
    a quick test (tests/test_gpu_render.py holds the unsorted order to it): here the sorted and the queue-order frames, and
    the material-sorted shade queue on top, must be the same bits with the same ray counts."""
    w, h, spp = 512, 288, 16
    g = pbrt_hip.Scene(hip_ctx, scenes.random_triangles(100_000, seq=4, size=0.03))
    cam = scenes.random_triangles_camera(w, h)
    a, st_a = g.render(cam, w, h, spp, max_depth=5, seed=9)
    assert a[..., :3].max() > 0
    for v in (dict(ray_order=1), dict(shade_order=2), dict(shade_order=1, spp_per_pass=5)):
        b, st_b = g.render(cam, w, h, spp, max_depth=5, seed=9, **v)
        assert a.tobytes() == b.tobytes(), v
        assert (st_a["rays_closest"], st_a["rays_shadow"]) == (st_b["rays_closest"], st_b["rays_shadow"]), v
    g.close()
