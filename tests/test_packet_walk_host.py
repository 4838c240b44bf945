"""Host model of the packet walk (pbrt-rs_amd/csrc/trace_wide_packet.h), no GPU.

The camera wavefront of a one-level scene is walked once per wave of 64 rays instead of once per ray. The argument that the
hits stay the reference's is wide_bvh.h's, one step further: the near-first order of the leaves depends on a ray only through
its three dir_is_neg bits, so the rays of one negmask share one order; a wave that visits a child whenever ANY of its lanes
passes the filter shows every lane a superset of the leaves of its own walk, in that order, and every leaf is confirmed per lane
with the reference's slab test on the exact box and the lane's current t_max. tests/native/packet_walk_check.cpp runs that walk
on the host with the product's own builder and filter arithmetic, beside the per-ray walk over the same records and the
reference's loop over the binary tree, and compares every lane's (slot, t, b0, b1, b2) bit for bit.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
from test_wide_host import _tree

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "packet_walk_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "libpacket_walk_check.so")
COUNTS = ("lanes", "left_to_binary", "packet_records", "packet_leaves", "ray_records", "ray_leaves", "negmask_groups", "groups",
          "deepest_stack", "stack_need", "packet_differs", "per_ray_differs")


@pytest.fixture(scope="module")
def chk():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(HERE, "..", "pbrt-rs_amd", "csrc", f) for f in ("host_wide.cpp", "host_wide.h", "wide_bvh.h", "wide_build.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        tmp = f"{OUT}.{os.getpid()}"   # renamed when complete: parallel test workers never load a half-written library
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", tmp, SRC])
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.packet_walk_check.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.packet_walk_check.restype = ctypes.c_int64
    return L


def _walk(chk, nodes, tris, rays, group=64):
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
    counts = np.zeros(len(COUNTS), dtype=np.int64)
    bad = chk.packet_walk_check(nodes.ctypes.data, len(nodes), tris.ctypes.data, len(tris), rays.ctypes.data, len(rays), group, counts.ctypes.data)
    return bad, dict(zip(COUNTS, counts.tolist()))


def _bundle(rng, n_groups, origin_spread, dir_spread, centre_dirs=None):
    """n_groups x 64 rays: per group one base origin and one base direction, lanes spread around them by the two widths."""
    o0 = rng.uniform(-2.5, 2.5, (n_groups, 1, 3))
    d0 = centre_dirs if centre_dirs is not None else -o0 + rng.normal(0, 0.3, (n_groups, 1, 3))   # towards the cloud around the origin
    o = o0 + rng.normal(0, 1, (n_groups, 64, 3)) * origin_spread
    d = d0 + rng.normal(0, 1, (n_groups, 64, 3)) * dir_spread
    t = np.full((n_groups, 64, 1), np.inf)
    return np.concatenate([o, d, t], axis=2).astype(np.float32)


def _negmask_groups(rays):
    m = (rays[..., 3] < 0) * 1 + (rays[..., 4] < 0) * 2 + (rays[..., 5] < 0) * 4
    return np.array([len(np.unique(g)) for g in m])


@pytest.mark.parametrize("big,max_prims", [(False, 1), (True, 3), (True, 4)])
def test_packets_of_every_kind_give_the_reference_hits(chk, big, max_prims):
    """Equal and mixed negmask, shared and different origins, leaves of 1 to max_prims triangles, groups of 64 and of fewer,
    placeholders (t_max < 0), axis-parallel rays (left to the binary walk) and finite t_max among the lanes."""
    # small triangles: one per leaf; large overlapping ones: SAH leaves of 3 and 4 (leaves of 2: the duplicated triangles below)
    sc = scenes.random_triangles(3000, seq=5, size=0.4) if big else scenes.random_triangles(20_000, seq=3, size=0.05)
    nodes, tris = _tree(sc, max_prims)
    assert nodes["n_primitives"].max() == max_prims
    rng = np.random.default_rng(40 + max_prims)
    pixel = _bundle(rng, 60, 0.0, 0.002)          # shared origin, one pixel wide: one negmask (nearly always)
    lens = _bundle(rng, 40, 0.02, 0.002)          # origins on a lens
    fan = _bundle(rng, 40, 0.0, 0.6)              # shared origin, a wide fan: several octants in one wave
    loose = _bundle(rng, 40, 1.0, 1.0)            # nothing shared
    axis = _bundle(rng, 20, 0.0, 0.01, centre_dirs=np.array([0.0, 0.0, -1.0]))   # straddles dir.x = 0 and dir.y = 0: the centre row and column
    axis[:, :, :3] = np.array([0.0, 0.0, 3.5], dtype=np.float32)
    assert (_negmask_groups(pixel) == 1).mean() > 0.8 and (_negmask_groups(fan) > 1).mean() > 0.5 and (_negmask_groups(axis) > 1).all()
    rays = np.concatenate([pixel, lens, fan, loose, axis])
    rays[::7, 5::9, 6] = -1.0                     # placeholders
    rays[1::5, 3::11, 3] = 0.0                    # axis-parallel lanes
    rays[2::3, ::4, 6] = rng.uniform(0.5, 4.0, rays[2::3, ::4, 6].shape)   # finite t_max
    bad, c = _walk(chk, nodes, tris, rays)
    assert bad == 0, c
    assert c["lanes"] > 0.8 * rays.shape[0] * 64 and c["left_to_binary"] > 0
    assert c["negmask_groups"] > c["groups"] and c["deepest_stack"] <= c["stack_need"]
    bad, c = _walk(chk, nodes, tris, rays.reshape(-1, 7)[: 37 * 50], group=37)
    assert bad == 0 and c["groups"] == 50, c


@pytest.mark.parametrize("max_prims,split", [(1, 0), (4, 0), (2, 2), (4, 3)])
def test_duplicated_triangles_and_rays_through_shared_vertices(chk, max_prims, split):
    """Triangles that occur twice (ties between equal hits) in a mesh whose triangles share vertices, rays aimed exactly at the
    vertices and at edge midpoints, from one origin per wave and from different ones."""
    rng = np.random.default_rng(7)
    g = 14
    xs, ys = np.meshgrid(np.linspace(-1, 1, g), np.linspace(-1, 1, g), indexing="ij")
    zs = 0.15 * np.sin(3 * xs) * np.cos(2 * ys)
    verts = np.stack([xs, ys, zs], axis=2).reshape(-1, 3).astype(np.float32)
    quad = np.array([[i * g + j, (i + 1) * g + j, (i + 1) * g + j + 1, i * g + j + 1] for i in range(g - 1) for j in range(g - 1)])
    idx = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]).astype(np.int32)
    idx = np.concatenate([idx, idx[::2]])         # every second triangle twice
    sc = dict(positions=verts, indices=idx)
    nodes, tris = _tree(sc, max_prims, split)
    assert nodes["n_primitives"].max() >= 2       # the builders keep equal triangles in one leaf
    tri = verts[idx]
    targets = np.concatenate([tri.reshape(-1, 3), (tri[:, 0] + tri[:, 1]) * np.float32(0.5)])
    targets = targets[rng.integers(0, len(targets), 64 * 120)].reshape(120, 64, 3)
    o_shared = np.broadcast_to(rng.uniform(-1, 1, (120, 1, 3)) + np.array([0, 0, 3.0]), targets.shape)
    o_own = o_shared + rng.normal(0, 0.3, targets.shape)
    for o in (o_shared, o_own):
        o = o.astype(np.float32)
        rays = np.concatenate([o, (targets - o).astype(np.float32), np.full((120, 64, 1), np.inf, dtype=np.float32)], axis=2)
        bad, c = _walk(chk, nodes, tris, rays)
        assert bad == 0, c
        assert c["lanes"] + c["left_to_binary"] == 120 * 64 and c["lanes"] > 0.95 * 120 * 64


def _camera_rays(cam, xs, ys, spp, rng):
    """Pinhole camera rays of `spp` uniform samples in each pixel (x, y) (PerspectiveCamera::generate_ray, lens_radius 0)."""
    r2c = np.asarray(cam["raster_to_camera"], dtype=np.float64).reshape(4, 4)
    c2w = np.asarray(cam["camera_to_world"], dtype=np.float64).reshape(4, 4)
    px = xs[:, None] + rng.random((len(xs), spp))
    py = ys[:, None] + rng.random((len(xs), spp))
    p = np.stack([px, py, np.zeros_like(px), np.ones_like(px)], axis=2) @ r2c.T
    d = p[..., :3] / p[..., 3:]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    d = d @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return np.concatenate([o, d, np.full(d.shape[:2] + (1,), np.inf)], axis=2).astype(np.float32)


def test_step_ratio_of_one_pixel_packets_on_the_benchmark_tree(chk):
    """What the packet kernel's estimate rests on (profiles/r14_camera_packets.txt): on the benchmark's tree (config 3: 1 M random
    triangles) under its camera, the records and leaves a one-pixel packet of 64 samples visits against the mean of its rays' own
    walks. A packet visits the union of its rays' walks: the ratio is at least 1 (the union holds every walk) and at most 64 (it
    holds nothing else)."""
    nodes, tris = _tree(scenes.random_triangles(1_000_000, seq=1), 4)
    cam = scenes.random_triangles_camera(1920, 1080)
    rng = np.random.default_rng(14)
    n_pix = 3000
    rays = _camera_rays(cam, rng.integers(0, 1920, n_pix).astype(np.float64), rng.integers(0, 1080, n_pix).astype(np.float64), 64, rng)
    bad, c = _walk(chk, nodes, tris, rays)
    assert bad == 0, c
    rec_ratio = c["packet_records"] / (c["ray_records"] / 64.0)
    leaf_ratio = c["packet_leaves"] / (c["ray_leaves"] / 64.0)
    print(f"packet / mean-ray: records {rec_ratio:.3f} ({c['packet_records'] / n_pix:.1f} vs {c['ray_records'] / 64.0 / n_pix:.1f} per pixel), "
          f"leaves {leaf_ratio:.3f} ({c['packet_leaves'] / n_pix:.2f} vs {c['ray_leaves'] / 64.0 / n_pix:.2f}), "
          f"negmask groups per packet {c['negmask_groups'] / c['groups']:.4f}, deepest stack {c['deepest_stack']} of {c['stack_need']}")
    assert c["lanes"] == n_pix * 64
    assert 1.0 <= rec_ratio <= 64.0 and 1.0 <= leaf_ratio <= 64.0
