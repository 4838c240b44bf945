"""The sorted ray queue carries one sort entry per PATH (wf_state.h: Queues::keys, wf_ray_expand.h): from the second bounce
on k_shade leaves a (cell, record << 4 | which rays) pair per path instead of up to three trace-queue entries, the host
sorts the pairs and two kernels expand the sorted list into the trace queue, closest-hit rays first. Nothing of that may
show in a result: every case renders in Morton order (ray_order 0) and in queue order (ray_order 1, which never takes the
new path) and asks for the same film bytes and the same ray counts.

The frames are the smallest that still have a wavefront of >= 2^20 rays behind the first bounce (only those are sorted),
2.0 - 3.5 M paths (the ray counts per wavefront were read from the library's log); test_the_sorted_path_ran_and_the_frame_under_the_gate_agrees reads the library's own per-wavefront log
to show that such a wavefront was there, and covers the unsorted expansion with a frame that cannot reach the gate.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1 << 20  # render.hip: RenderJob::trace_wavefront sorts queues of at least this many rays


def _both_orders(g, cam, w, h, spp, **kw):
    a, st_a = g.render(cam, w, h, spp, ray_order=0, **kw)
    b, st_b = g.render(cam, w, h, spp, ray_order=1, **kw)
    assert a.tobytes() == b.tobytes()
    assert (st_a["rays_closest"], st_a["rays_shadow"]) == (st_b["rays_closest"], st_b["rays_shadow"])
    assert np.isfinite(a).all() and a[..., :3].any()
    return st_a


def test_matte_under_an_environment_light(hip_ctx):
    """Every surviving path emits all three rays and its MIS ray is boolean (an infinite light): two tokens in the any-hit
    section, one in the closest-hit section."""
    w, h = 512, 288
    g = pbrt_hip.Scene(hip_ctx, scenes.random_triangles(100_000, seq=4, size=0.03))
    st = _both_orders(g, scenes.random_triangles_camera(w, h), w, h, 16, max_depth=5, seed=9)
    assert st["rays_shadow"] > 0
    g.close()


def test_matte_mirror_and_glass_mixed(hip_ctx):
    """Specular bounces emit a continuation ray only, matte ones up to three, towards an area light (MIS ray in the
    closest-hit section) or the environment (boolean); paths that end leave the shade queue and get no sort entry."""
    w, h = 512, 288
    g = pbrt_hip.Scene(hip_ctx, scenes.mixed_materials_scene())
    _both_orders(g, scenes.random_triangles_camera(w, h), w, h, 24, max_depth=5, seed=21)  # 1.8 M, 1.5 M, 1.2 M rays at wavefronts 2-4
    g.close()


def test_area_light_only(hip_ctx):
    """The Cornell box: no infinite light, so no MIS ray is boolean and all of them land in the closest-hit section."""
    w = h = 384
    g = pbrt_hip.Scene(hip_ctx, scenes.cornell_box())
    _both_orders(g, scenes.cornell_camera(w, h), w, h, 16, max_depth=5, seed=3)
    g.close()


def test_instanced_scene(hip_ctx):
    """A two-level scene: the tokens go through the instanced traversal kernels (INST)."""
    w, h = 512, 288
    g = pbrt_hip.Scene(hip_ctx, scenes.two_level_scene())
    _both_orders(g, scenes.two_level_camera(w, h), w, h, 24, max_depth=5, seed=5)  # 1.3 M and 1.1 M rays at wavefronts 2 and 3
    g.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_tile_share_in_several_passes(hip_ctx, rank):
    """One rank's half of the tiles in two passes of 12 samples: the sort and expansion buffers are used again by the second
    pass, and the entry counts are multiples of nothing."""
    w, h = 768, 432
    g = pbrt_hip.Scene(hip_ctx, scenes.random_triangles(100_000, seq=4, size=0.03))
    _both_orders(g, scenes.random_triangles_camera(w, h), w, h, 24, max_depth=5, seed=13, tile_rank=rank, tile_world=2, spp_per_pass=12)
    g.close()


_CHILD = r"""
import hashlib, sys
import pbrt_hip
from pbrt_hip import scenes
ctx = pbrt_hip.Context(0)  # PBRT_HIP_TRACE_LOG is read here
g = pbrt_hip.Scene(ctx, scenes.random_triangles(100_000, seq=4, size=0.03))
for name, (w, h, spp) in (("big", (512, 288, 16)), ("small", (256, 144, 9))):
    cam = scenes.random_triangles_camera(w, h)
    for order in (0, 1):
        sys.stderr.write(f"RENDER {name} {order}\n")
        sys.stderr.flush()
        film, st = g.render(cam, w, h, spp, max_depth=5, seed=9, ray_order=order)
        print(name, order, hashlib.sha256(film.tobytes()).hexdigest(), st["rays_closest"], st["rays_shadow"], flush=True)
g.close()
ctx.close()
"""


def test_the_sorted_path_ran_and_the_frame_under_the_gate_agrees():
    """In a process of its own with PBRT_HIP_TRACE_LOG set (one stderr line per traversal launch; each render here is one
    pass, so the lines of a render are its wavefronts in order): the 512x288x16 frame has a wavefront of index >= 2 with at
    least 2^20 rays, i.e. the sort and the expansion ran; the 256x144x9 frame has 331 776 paths, at most 995 328 rays per
    wavefront, so none of its queues is sorted and every one from index 2 on goes through the expansion alone. Both frames
    agree with their queue-order renders."""
    env = dict(os.environ, PBRT_HIP_TRACE_LOG="1")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "pbrt-rs_amd")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, order, digest, rc, rs = line.split()
        out[(name, int(order))] = (digest, int(rc), int(rs))
    assert len(out) == 4
    assert out[("big", 0)] == out[("big", 1)]
    assert out[("small", 0)] == out[("small", 1)]
    rays = {}
    cur = None
    for line in r.stderr.splitlines():
        m = re.match(r"RENDER (\w+) (\d)", line)
        if m:
            cur = (m.group(1), int(m.group(2)))
            rays[cur] = []
            continue
        m = re.match(r"\[pbrt_hip\] k_trace: (\d+) rays", line)
        if m and cur:
            rays[cur].append(int(m.group(1)))
    print(rays)
    assert max(rays[("big", 0)][2:]) >= GATE
    assert len(rays[("small", 0)]) > 2 and max(rays[("small", 0)][2:]) < GATE
    assert rays[("big", 0)] == rays[("big", 1)] and rays[("small", 0)] == rays[("small", 1)]
