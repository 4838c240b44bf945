"""The camera wavefront as one-pixel wave packets (pbrt-rs_amd/csrc/trace_wide_packet.h, k_trace_wide_packet).

Where a wave of camera paths is the 64 samples of one pixel, a one-level scene's wide records are walked once per wave instead
of once per ray. Nothing of that may show in a result: every case renders with the packets on (the default), with them off
(pbrt_hip_context_set_camera_packets) and over the binary records (PBRT_TRAVERSAL_STACK) and asks for the same film bytes and
the same ray counts; pbrt_hip_context_camera_kernel says which kernel traced the camera rays. The host model of the walk is
tests/test_packet_walk_host.py.
"""
import numpy as np
import pytest

import oracle
import pbrt_hip
from pbrt_hip import scenes
from test_gpu_render import _compare

pytestmark = pytest.mark.gpu

PACKET, PER_LANE = pbrt_hip.CAMERA_KERNEL_PACKET, pbrt_hip.CAMERA_KERNEL_PER_LANE


def _three_ways(ctx, g, cam, w, h, spp, expect=PACKET, **kw):
    """Packets on, packets off, binary records: identical films and ray counts. Returns the film and the stats."""
    kw.setdefault("max_depth", 3)
    try:
        film, st = g.render(cam, w, h, spp, **kw)
        assert ctx.camera_kernel() == expect
        ctx.set_camera_packets(pbrt_hip.CAMERA_PACKETS_OFF)
        film_off, st_off = g.render(cam, w, h, spp, **kw)
        assert ctx.camera_kernel() == PER_LANE
        ctx.set_camera_packets(pbrt_hip.CAMERA_PACKETS_AUTO)
        ctx.set_traversal(pbrt_hip.TRAVERSAL_STACK)
        film_bin, st_bin = g.render(cam, w, h, spp, **kw)
        assert ctx.camera_kernel() == PER_LANE
    finally:   # the context is shared by the session
        ctx.set_camera_packets(pbrt_hip.CAMERA_PACKETS_AUTO)
        ctx.set_traversal(pbrt_hip.TRAVERSAL_AUTO)
    for other, st_o in ((film_off, st_off), (film_bin, st_bin)):
        assert film.tobytes() == other.tobytes()
        assert (st["rays_closest"], st["rays_shadow"], st["camera_samples"]) == (st_o["rays_closest"], st_o["rays_shadow"], st_o["camera_samples"])
    assert np.isfinite(film).all()
    return film, st


@pytest.fixture(scope="module")
def cloud(hip_ctx):
    sc = scenes.random_triangles(20_000, seq=3, size=0.05)
    g = pbrt_hip.Scene(hip_ctx, sc)
    assert g.wide_records()[0] > 0
    yield sc, g
    g.close()


def test_one_pixel_per_wave(hip_ctx, cloud):
    """64 spp: a wave of paths is one pixel's samples and the packet kernel traces the camera rays."""
    w, h = 64, 48
    film, st = _three_ways(hip_ctx, cloud[1], scenes.random_triangles_camera(w, h), w, h, 64, seed=5)
    assert film[..., :3].any() and st["rays_shadow"] > 0


def test_film_equals_the_oracle(hip_ctx, cloud):
    w, h = 32, 24
    cam = scenes.random_triangles_camera(w, h)
    film, st = _three_ways(hip_ctx, cloud[1], cam, w, h, 64, seed=2)
    osc = oracle.OracleScene(cloud[0])
    film_c, st_c = osc.render(scenes.camera_dict_to_floats(cam), w, h, 64, max_depth=3, seed=2)
    osc.close()
    assert st["rays_closest"] + st["rays_shadow"] == st_c["rays"]
    _compare(film, film_c)   # the suite's comparison with the oracle (test_gpu_render.py): equal weights, 1e-5 per pixel, 1e-6 rmse


def test_centre_row_and_column_split_a_wave_by_negmask(hip_ctx, cloud):
    """A view along -z with the image centre inside the film: the pixels around the centre row and column hold rays of both
    signs of dir.y and dir.x, so a wave there walks once per negmask group."""
    w, h = 33, 25     # odd: the centre row and column run through the middle of pixels
    cam = scenes.random_triangles_camera(w, h)
    rays, _, _, pix = cloud[1].camera_rays(cam, w, h, 64, seed=4)
    # the export lists the paths sample by sample; in the render a wave of paths is the 64 samples of one pixel
    valid = pix[:, 0] >= 0
    order = np.argsort(pix[valid, 1] * w + pix[valid, 0], kind="stable")
    d = rays["d"][valid][order].reshape(-1, 64, 3)
    assert len(d) == w * h
    negmask = (d[..., 0] < 0) * 1 + (d[..., 1] < 0) * 2 + (d[..., 2] < 0) * 4
    groups = np.array([len(np.unique(m)) for m in negmask])
    assert (groups > 1).sum() >= w + h - 1 and groups.max() == 4
    _three_ways(hip_ctx, cloud[1], cam, w, h, 64, seed=4)


def test_orthographic_camera_leaves_every_ray_to_the_follow_up_launch(hip_ctx, cloud):
    """Every ray is axis-parallel (two zero direction components): wide_ray_covered rejects all of them."""
    w, h = 32, 24
    cam = scenes.orthographic_camera((0.0, 0.0, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h)
    film, _ = _three_ways(hip_ctx, cloud[1], cam, w, h, 64, seed=6)
    assert film[..., :3].any()


def test_thin_lens_origins_differ_inside_a_wave(hip_ctx, cloud):
    w, h = 32, 24
    cam = scenes.perspective_camera((0.0, 0.0, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, w, h, lens_radius=0.05, focal_distance=3.5)
    _three_ways(hip_ctx, cloud[1], cam, w, h, 64, seed=7)


def test_cropped_pixel_bounds_leave_placeholders_in_the_waves(hip_ctx, cloud):
    w, h = 64, 48
    _three_ways(hip_ctx, cloud[1], scenes.random_triangles_camera(w, h), w, h, 64, seed=8, bounds=(5, 3, 43, 30))


def test_tile_share(hip_ctx, cloud):
    w, h = 64, 48
    _three_ways(hip_ctx, cloud[1], scenes.random_triangles_camera(w, h), w, h, 64, seed=9, tile_rank=1, tile_world=2)


def test_48_spp_keeps_the_per_lane_kernel(hip_ctx, cloud):
    """48 samples per pixel: a wave holds 16 samples of four pixels (group_shift 4) and the camera rays keep k_trace_wide."""
    w, h = 32, 24
    _three_ways(hip_ctx, cloud[1], scenes.random_triangles_camera(w, h), w, h, 48, expect=PER_LANE, seed=10)


def test_several_passes(hip_ctx, cloud):
    """128 spp in two passes of 64: the packet kernel runs once per pass."""
    w, h = 32, 24
    _three_ways(hip_ctx, cloud[1], scenes.random_triangles_camera(w, h), w, h, 128, seed=11, spp_per_pass=64)


def test_adversarial_meshes_under_a_camera(hip_ctx):
    """The meshes of test_gpu_wide.py::test_adversarial_meshes_and_rays_through_vertices_and_edges (coincident vertices, zero-area
    and repeated triangles) seen by a camera that looks at one of their vertices: ties between equal hits inside a wave."""
    from hypothesis import given, settings, strategies as st
    from test_property_host import meshes

    @settings(max_examples=12, deadline=None)
    @given(mesh=meshes(), max_prims=st.sampled_from([1, 2, 4]), split=st.sampled_from([0, 1, 2, 3]), which=st.integers(0, 1000))
    def check(mesh, max_prims, split, which):
        verts, idx = mesh
        sc = dict(positions=verts, indices=idx, tri_material=np.zeros(len(idx), dtype=np.int32),
                  materials=scenes._materials([(1, (0.5, 0.5, 0.5), (0, 0, 0), 1.0)]),
                  tri_light=np.full(len(idx), -1, dtype=np.int32), lights=scenes._lights([(pbrt_hip.scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1)]))
        target = verts[idx.reshape(-1)[which % idx.size]].astype(np.float64)
        scale = max(float(np.abs(verts).max()), 1.0)
        eye = target + np.array([0.3, -0.2, 1.0]) * 2.0 * scale
        if not (np.isfinite(eye).all() and np.isfinite(target).all()):
            return
        g = pbrt_hip.Scene(hip_ctx, sc, max_prims_in_node=max_prims, split_method=split)
        try:
            n_rec, why = g.wide_records()
            assert n_rec >= 0 or why
            cam = scenes.perspective_camera(tuple(eye), tuple(target), (0.0, 1.0, 0.0), 30.0, 16, 16)
            _three_ways(hip_ctx, g, cam, 16, 16, 64, expect=PACKET if n_rec >= 0 else PER_LANE, seed=which)
        finally:
            g.close()

    check()


def test_deep_tree(hip_ctx):
    """The tree of test_gpu_wide.py::test_stacks_deeper_than_the_lds_part (large overlapping triangles, one per leaf): the walk
    needs more stack than the per-lane kernel's LDS part holds. The wave's stack holds it (64 references), or the per-lane
    kernel runs; the film is the same either way."""
    sc = scenes.random_triangles(3000, seq=5, size=0.4)
    g = pbrt_hip.Scene(hip_ctx, sc, max_prims_in_node=1, split_method=pbrt_hip.SPLIT_MIDDLE)
    assert g.wide_records()[0] > 0
    w, h = 32, 24
    try:
        film, _ = g.render(scenes.random_triangles_camera(w, h), w, h, 64, max_depth=3, seed=12)
        expect = hip_ctx.camera_kernel()
        assert expect in (PACKET, PER_LANE)
        _three_ways(hip_ctx, g, scenes.random_triangles_camera(w, h), w, h, 64, expect=expect, seed=12)
    finally:
        g.close()


def test_not_selected(hip_ctx, cloud):
    """Two-level, sphere and moving scenes, and a render with counting on, keep the per-lane kernels."""
    from motion_cases import FIVE, FLOOR, SUN, make_scene
    w, h = 32, 24
    for sc, cam in ((scenes.two_level_scene(), scenes.two_level_camera(w, h)),
                    (scenes.sphere_scene(), scenes.sphere_camera(w, h)),
                    (make_scene(FIVE, world=FLOOR, lights=SUN), scenes.perspective_camera((1.0, -7.0, 4.0), (0, 0, 0), (0, 0, 1), 50.0, w, h))):
        g = pbrt_hip.Scene(hip_ctx, sc)
        film, _ = g.render(cam, w, h, 64, max_depth=3, seed=1)
        assert hip_ctx.camera_kernel() == PER_LANE and np.isfinite(film).all()
        g.close()
    cam = scenes.random_triangles_camera(w, h)
    plain, _ = cloud[1].render(cam, w, h, 64, max_depth=3, seed=1)
    assert hip_ctx.camera_kernel() == PACKET
    for mode in (1, 2):
        try:
            hip_ctx.set_counting(mode)
            counted, _ = cloud[1].render(cam, w, h, 64, max_depth=3, seed=1)
            assert hip_ctx.camera_kernel() == PER_LANE
        finally:
            hip_ctx.set_counting(0)
        assert counted.tobytes() == plain.tobytes()


def test_fetch_probe_reports_a_rate(hip_ctx, cloud):
    """pbrt_hip_probe_packet_fetch: both forms of the wave-uniform record fetch run and report a rate."""
    for form in (0, 1):
        assert cloud[1].probe_packet_fetch(form, iters=64) > 0.0
