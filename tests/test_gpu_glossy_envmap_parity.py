"""GPU parity of plastic / metal and of image environment maps against the CPU oracle at the same sampler seed, held as
test_gpu_render.py holds matte / mirror / glass under constant lights: per pixel 1e-5 * max(1, |cpu|), RMSE 1e-6, the weight
channel equal, and rays_closest + rays_shadow equal to the oracle's rays. The BSDF itself is compared sample for sample,
bit for bit, through pbrt_hip_bsdf_query / orc_bsdf_query. The oracle's side (oracle/src/o_microfacet.h, o_reflection.h,
o_render.h) is pinned by test_oracle_microfacet.py, test_oracle_envmap.py and test_exact_rational_pin.py on the host."""
import numpy as np
import pytest

import oracle
import pbrt_hip
from pbrt_hip import scenes
from envmap_cases import _rot, _sun_map
from glossy_cases import CASES, _directions, _glossy_mixed, _table_scene, _unit, _with_glossy_rows
from test_gpu_render import _compare

pytestmark = pytest.mark.gpu

FIELDS = ("f", "pdf", "wi_s", "f_s", "pdf_s", "flags")


def _edge_directions(ax, ay, seed):
    """What test_bsdf_query_matches_model has to leave out: grazing and exactly tangent wo / wi, wo below the surface,
    wo + wi = 0, the normal-incidence branch of trowbridge_reitz_sample11 (cos of the stretched wo on both sides of 0.9999)
    and u at 0, 0.5 and 1 - ulp."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    wo, wi, u = [], [], []

    def add(o, i, uu=None):
        o, i = np.asarray(o, f32).reshape(-1, 3), np.asarray(i, f32).reshape(-1, 3)
        wo.append(o)
        wi.append(i)
        u.append(rng.random((len(o), 2)).astype(f32) if uu is None else np.asarray(uu, f32).reshape(-1, 2))

    n = 2000
    base_o, base_i = _unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(n, 3)))
    for z in (1e-6, -1e-6, 1e-4, -1e-3, 0.0, -0.0):
        o, i = base_o.copy(), base_i.copy()
        o[:, 2] = z
        add(o, base_i)              # wo grazing / tangent
        i[:, 2] = z
        add(base_o, i)              # wi grazing / tangent
        add(o, i)                   # both
    below = base_o.copy()
    below[:, 2] = -np.abs(below[:, 2])
    add(below, base_i)
    add(below, _unit(below * np.array([-1, -1, 1]) + 0.1 * rng.normal(size=(n, 3))))
    add(base_o, -base_o.astype(f32))                      # wo + wi = 0 exactly
    add(base_o, _unit(-base_o + 1e-4 * rng.normal(size=(n, 3))))
    # the stretched wo = normalize(ax x, ay y, z): tilt the unstretched one so that its cosine straddles 0.9999
    for tilt in (0.002, 0.0141, 0.02, 0.1):
        phi = rng.uniform(0, 2 * np.pi, n)
        s = tilt * rng.uniform(0.5, 1.5, n)
        o = _unit(np.stack([s * np.cos(phi) / max(ax, 1e-3), s * np.sin(phi) / max(ay, 1e-3), np.ones(n)], axis=1))
        o = np.where(np.linalg.norm(o[:, :2], axis=1, keepdims=True) < 0.999, o, base_o)
        add(o, base_i)
        add(-o, base_i)
    add([[0, 0, 1], [0, 0, -1], [0, 0, 1], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [0, 0, 1], [0.6, 0, 0.8], [0, 0, 1], [0, 0, 1]])
    top = np.nextafter(f32(1), f32(0))
    corners = np.array([(a, b) for a in (0.0, 0.5, top) for b in (0.0, 0.5, top)], f32)
    for c in corners:
        k = 300
        add(base_o[:k], base_i[:k], np.broadcast_to(c, (k, 2)))
        add(below[:k], base_i[:k], np.broadcast_to(c, (k, 2)))
    return np.concatenate(wo), np.concatenate(wi), np.concatenate(u)


def _same_bits(a, b):
    """bit equality per entry; a NaN equals a NaN (the payload is not part of the arithmetic)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    else:
        eq = a == b
    return eq if eq.ndim == 1 else eq.all(axis=1)


@pytest.fixture(scope="module")
def tables(hip_ctx):
    sc = _table_scene([c[1] for c in CASES])
    dev, cpu = pbrt_hip.Scene(hip_ctx, sc), oracle.OracleScene(sc)
    for i, c in enumerate(CASES):
        if c[2] is not None:
            dev.set_material_roughness(i, c[2][0], c[2][1], remap=c[2][2])
            cpu.set_material_roughness(i, c[2][0], c[2][1], remap=c[2][2])
    yield dev, cpu
    dev.close()
    cpu.close()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bsdf_bit_for_bit(tables, i):
    """Scene.bsdf_query == OracleScene.bsdf_query in every bit of f, pdf, wi_s, f_s, pdf_s and the sampled flags, over the
    model test's directions and the ones it leaves out; no sample is exempt."""
    dev, cpu = tables
    m = CASES[i][3]
    a = _directions(20000, 100 + i)
    b = _edge_directions(getattr(m, "ax", 1.0), getattr(m, "ay", 1.0), 300 + i)
    wo, wi, u = (np.concatenate([x, y]) for x, y in zip(a, b))
    qd, qc = dev.bsdf_query(i, wo, wi, u), cpu.bsdf_query(i, wo, wi, u)
    report = []
    for k in FIELDS:
        eq = _same_bits(qd[k], qc[k])
        print(f"{CASES[i][0]} {k}: {int((~eq).sum())} of {eq.size} differ")
        if not eq.all():
            j = int(np.nonzero(~eq)[0][0])
            report.append(f"{k}: {int((~eq).sum())} of {eq.size} differ, first at {j}: wo {wo[j]} wi {wi[j]} u {u[j]} "
                          f"device {qd[k][j]} oracle {qc[k][j]}")
    assert not report, "\n".join(report)
    assert (qc["pdf_s"] > 0).mean() > 0.3   # the comparison is not one of zeros


def _pair(hip_ctx, sc, setup=None):
    """the oracle's and the device's scene of `sc`, `setup(scene)` applied to both (roughness, maps)"""
    osc = oracle.OracleScene(sc, normals=sc.get("normals"), uvs=sc.get("uvs"), tangents=sc.get("tangents"))
    gsc = pbrt_hip.Scene(hip_ctx, sc)
    if setup is not None:
        setup(osc)
        setup(gsc)
    return osc, gsc


def _check(osc, gsc, cam, w, h, spp, **kw):
    film_c, st_c = osc.render(scenes.camera_dict_to_floats(cam), w, h, spp, **kw)
    film_g, st_g = gsc.render(cam, w, h, spp, **kw)
    _compare(film_g, film_c)
    assert st_g["rays_closest"] + st_g["rays_shadow"] == st_c["rays"]
    assert st_g["camera_samples"] == st_c["camera_samples"]
    return film_g, film_c


def _both(hip_ctx, sc, cam, w, h, spp, setup=None, **kw):
    osc, gsc = _pair(hip_ctx, sc, setup)
    out = _check(osc, gsc, cam, w, h, spp, **kw)
    gsc.close()
    osc.close()
    return out


W, H = 64, 64


@pytest.fixture(scope="module")
def glossy_pair(hip_ctx):
    osc, gsc = _pair(hip_ctx, _glossy_mixed())
    yield osc, gsc
    gsc.close()
    osc.close()


@pytest.mark.parametrize("max_depth", [1, 5, 16])
@pytest.mark.parametrize("rr_threshold", [1.0, 0.3])
@pytest.mark.parametrize("light_strategy", [0, 1, 2])
def test_glossy_mixed_path(glossy_pair, light_strategy, rr_threshold, max_depth):
    """matte, mirror, glass, plastic and metal by triangle under area lights and a constant infinite light: glossy bounces keep
    PF_SPECULAR_BOUNCE clear, beta and Russian roulette after them, the MIS weight of a glossy BSDF sample."""
    film_g, _ = _check(*glossy_pair, scenes.random_triangles_camera(W, H), W, H, 4, max_depth=max_depth, rr_threshold=rr_threshold,
                       light_strategy=light_strategy, seed=11)
    assert pbrt_hip.film_to_rgb(film_g).mean() > 0.01


@pytest.mark.parametrize("integrator,kw", [(1, dict(max_depth=1, light_strategy=0)), (1, dict(max_depth=3, light_strategy=0)),
                                           (1, dict(max_depth=1, light_strategy=1)), (1, dict(max_depth=3, light_strategy=1)),
                                           (2, dict(max_depth=4)), (3, dict(ao_samples=4))])
def test_glossy_mixed_other_integrators(glossy_pair, integrator, kw):
    _check(*glossy_pair, scenes.random_triangles_camera(W, H), W, H, 4, integrator=integrator, seed=13, **kw)


@pytest.mark.parametrize("sampler", [("stratified", 3, 2, True, 4), ("zerotwo", 4), ("halton",)])
def test_glossy_mixed_samplers_and_tile_shares(hip_ctx, sampler):
    """the tabulating samplers on path and on the direct-lighting sample arrays, and the frame as the sum of 3 tile shares"""
    sc = _glossy_mixed()
    sc["lights"]["n_samples"] = 3
    osc, gsc = _pair(hip_ctx, sc)
    cam = scenes.random_triangles_camera(W, H)
    _check(osc, gsc, cam, W, H, 6, max_depth=5, light_strategy=1, seed=53, sampler=sampler)
    for depth in (1, 3):
        _check(osc, gsc, cam, W, H, 4, integrator=1, max_depth=depth, light_strategy=0, seed=59, sampler=sampler)
    kw = dict(max_depth=5, light_strategy=1, seed=53, sampler=sampler)
    film_c, st_c = osc.render(scenes.camera_dict_to_floats(cam), W, H, 6, **kw)
    parts = [gsc.render(cam, W, H, 6, tile_rank=r, tile_world=3, **kw) for r in range(3)]
    _compare(sum(p[0] for p in parts), film_c)
    assert sum(p[1]["rays_closest"] + p[1]["rays_shadow"] for p in parts) == st_c["rays"]
    gsc.close()
    osc.close()


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=5, light_strategy=1)), (1, dict(max_depth=3, light_strategy=0)),
                                           (2, dict(max_depth=3))])
def test_anisotropic_metal_follows_the_mesh_tangents(hip_ctx, integrator, kw):
    """anisotropic and unremapped roughness on a mesh with per-vertex normals, uvs and tangents: the lobe's x axis is the
    shading dpdu, which varies over the mesh."""
    sc = scenes.with_vertex_shading(_glossy_mixed(), seq=7, normals=True, uvs=True, tangents=True)
    n = len(sc["materials"])

    def setup(s):
        s.set_material_roughness(n - 1, 0.15, 0.6, remap=False)   # metal
        s.set_material_roughness(n - 2, 0.05, 0.05, remap=False)  # plastic
    film_g, _ = _both(hip_ctx, sc, scenes.random_triangles_camera(W, H), W, H, 4, setup=setup, integrator=integrator, seed=67, **kw)
    # the anisotropy matters: swapped alphas render another film
    g = pbrt_hip.Scene(hip_ctx, sc)
    g.set_material_roughness(n - 1, 0.6, 0.15, remap=False)
    g.set_material_roughness(n - 2, 0.05, 0.05, remap=False)
    other, _ = g.render(scenes.random_triangles_camera(W, H), W, H, 4, integrator=integrator, seed=67, **kw)
    g.close()
    assert other.tobytes() != film_g.tobytes()


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=5, light_strategy=1)), (0, dict(max_depth=4, light_strategy=2)),
                                           (1, dict(max_depth=3, light_strategy=0)), (2, dict(max_depth=3))])
def test_glossy_spheres_beside_a_sphere_light(hip_ctx, integrator, kw):
    """plastic and metal on spheres (material column 4 / 5) in the Cornell box beside a sphere area light"""
    sc = _with_glossy_rows(scenes.cornell_box())
    n_mat = len(sc["materials"])
    n_tris, n_l = sc["indices"].shape[0], len(sc["lights"])
    sph = np.zeros((4, 8), dtype=np.float32)
    sph[0] = (400.0, 300.0, 200.0, 40.0, 0, n_l, 0, 0)               # the emitter
    sph[1] = (180.0, 120.0, 250.0, 90.0, n_mat - 2, -1, 0, 0)        # plastic
    sph[2] = (380.0, 100.0, 350.0, 80.0, n_mat - 1, -1, 0, 0)        # metal
    sph[3] = (278.0, 400.0, 300.0, 60.0, n_mat - 1, -1, 0, 0)
    sc["spheres"] = sph
    sc["lights"] = np.concatenate([sc["lights"], scenes._lights([(scenes.LIGHT_DIFFUSE_AREA, (30.0, 25.0, 20.0), n_tris, 0, 2)])])
    _both(hip_ctx, sc, scenes.cornell_camera(W, H), W, H, 4, integrator=integrator, seed=101, **kw)


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=5, light_strategy=1)), (1, dict(max_depth=3, light_strategy=0))])
def test_instance_overrides_to_glossy(hip_ctx, integrator, kw):
    sc = _with_glossy_rows(scenes.instanced_scene(n_base_tris=2000, n_instances=60, extent=1.5))
    sc["instance_material"] = (np.arange(60) % 5).astype(np.int32)
    _both(hip_ctx, sc, scenes.instanced_camera(W, H, extent=1.5), W, H, 4, integrator=integrator, seed=11, **kw)


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=8, light_strategy=1)), (0, dict(max_depth=5, light_strategy=0)),
                                           (1, dict(max_depth=3, light_strategy=0))])
def test_two_level_scene_with_glossy_objects(hip_ctx, integrator, kw):
    """glossy object triangles (per-triangle rows and instance overrides) lit by the emitting world quad"""
    sc = _with_glossy_rows(scenes.two_level_scene())
    n_mat = len(sc["materials"])
    for k, obj in enumerate(sc["objects"]):
        tm = np.asarray(obj["tri_material"]).copy()
        tm[k::3] = n_mat - 2 + (k % 2)
        obj["tri_material"] = tm.astype(np.int32)
    im = np.asarray(sc["instance_material"]).copy()
    im[::4] = n_mat - 1
    sc["instance_material"] = im.astype(np.int32)
    w, h = 80, 56
    _both(hip_ctx, sc, scenes.two_level_camera(w, h), w, h, 4, integrator=integrator, seed=6, **kw)


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=5, light_strategy=0)), (0, dict(max_depth=5, light_strategy=2)),
                                           (1, dict(max_depth=5, light_strategy=0)), (2, dict(max_depth=5))])
def test_delta_lights_on_glossy_surfaces(hip_ctx, integrator, kw):
    extra = [scenes.point_light((0.2, 0.9, -0.4), (3.0, 3.0, 3.0)), scenes.distant_light((0.0, 1.0, 0.2), (0.8, 0.8, 0.8)),
             scenes.spot_light((1.5, 1.5, 1.5), (0.0, 0.0, 0.0), (20.0, 18.0, 15.0), 40.0, 30.0)]
    for keep in (True, False):
        sc = scenes.with_lights(_glossy_mixed(), extra, keep_existing=keep)
        _both(hip_ctx, sc, scenes.random_triangles_camera(W, H), W, H, 4, integrator=integrator, seed=43, **kw)


@pytest.mark.parametrize("integrator,kw", [(0, dict(max_depth=8, light_strategy=1)), (1, dict(max_depth=3, light_strategy=0)),
                                           (2, dict(max_depth=4))])
def test_an_unused_glossy_row_against_the_oracle(hip_ctx, integrator, kw):
    """matte / mirror / glass through the glossy kernel instantiations (a glossy row that no triangle uses selects them)"""
    sc = _with_glossy_rows(scenes.mixed_materials_scene(n_tris=3000))
    _both(hip_ctx, sc, scenes.random_triangles_camera(W, H), W, H, 4, integrator=integrator, seed=11, **kw)


# ---- image environment maps ----

def _map_300x140():
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0.1, 1.0, size=(140, 300, 3)).astype(np.float32)
    rgb[30:34, 200:204] = 500.0
    return rgb


ROT = _rot((0.3, -0.5, 0.8), 37.0)
MAPS = {"sun": (lambda: _sun_map(level=200.0), None), "sun_rot": (lambda: _sun_map(level=200.0), ROT), "m300x140": (_map_300x140, None),
        "m300x140_rot": (_map_300x140, ROT), "m1x1": (lambda: np.full((1, 1, 3), 0.8, np.float32), ROT)}


def _mapped_scene(name):
    if name == "cornell":
        sc = scenes.with_lights(scenes.cornell_box(), scenes._lights([(scenes.LIGHT_INFINITE, (0.3, 0.4, 0.5), -1, 0, 1)]))
        return sc, scenes.cornell_camera(W, H)
    sc = scenes.mixed_materials_scene(n_tris=3000) if name == "mixed" else _glossy_mixed()
    return sc, scenes.random_triangles_camera(W, H)


def _infinite(sc):
    return int(np.nonzero(sc["lights"]["type"] == scenes.LIGHT_INFINITE)[0][0])


@pytest.mark.parametrize("which", list(MAPS))
@pytest.mark.parametrize("name", ["cornell", "mixed", "glossy"])
def test_image_maps(hip_ctx, name, which):
    """le on escaped camera, specular and MIS rays, sample_li / pdf_li with light_to_world, the power and spatial light
    distributions over a mapped light: path at depth 8 with each strategy (the spatial one twice, a map replaced in between),
    direct lighting with both strategies, Whitted at depth 4."""
    sc, cam = _mapped_scene(name)
    make, m = MAPS[which]
    rgb, inf = make(), _infinite(sc)
    osc, gsc = _pair(hip_ctx, sc, lambda s: s.set_environment_map(inf, rgb, m))
    for strategy in (0, 1, 2):
        _check(osc, gsc, cam, W, H, 4, max_depth=8, light_strategy=strategy, seed=5)
    other = _sun_map(sun=(20, 40), level=80.0)
    for s in (osc, gsc):
        s.set_environment_map(inf, other, m)
    _check(osc, gsc, cam, W, H, 4, max_depth=8, light_strategy=2, seed=5)
    for s in (osc, gsc):
        s.set_environment_map(inf, rgb, m)
    for strategy in (0, 1):
        _check(osc, gsc, cam, W, H, 4, integrator=1, max_depth=3, light_strategy=strategy, seed=7)
    _check(osc, gsc, cam, W, H, 4, integrator=2, max_depth=4, seed=9)
    gsc.close()
    osc.close()


def test_image_map_through_the_environment_camera(hip_ctx):
    sc, _ = _mapped_scene("glossy")
    rgb, inf = _map_300x140(), _infinite(sc)
    cam = scenes.environment_camera((0.1, 0.2, 0.3), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    _both(hip_ctx, sc, cam, 96, 48, 4, setup=lambda s: s.set_environment_map(inf, rgb, ROT), max_depth=5, seed=3)


@pytest.mark.parametrize("light_strategy", [0, 1, 2])
def test_two_infinite_lights_with_different_maps(hip_ctx, light_strategy):
    sc, cam = _mapped_scene("glossy")
    sc = scenes.with_lights(sc, scenes._lights([(scenes.LIGHT_INFINITE, (0.5, 0.4, 0.3), -1, 0, 1)]))
    ids = [int(i) for i in np.nonzero(sc["lights"]["type"] == scenes.LIGHT_INFINITE)[0]]
    assert len(ids) == 2

    def setup(s):
        s.set_environment_map(ids[0], _sun_map(level=200.0), ROT)
        s.set_environment_map(ids[1], _map_300x140(), None)
    osc, gsc = _pair(hip_ctx, sc, setup)
    _check(osc, gsc, cam, W, H, 4, max_depth=8, light_strategy=light_strategy, seed=5)
    _check(osc, gsc, cam, W, H, 4, integrator=1, max_depth=3, light_strategy=light_strategy % 2, seed=7)
    gsc.close()
    osc.close()


def test_image_map_on_an_instanced_scene(hip_ctx):
    sc = _with_glossy_rows(scenes.instanced_scene(n_base_tris=2000, n_instances=60, extent=1.5))
    sc["instance_material"] = (np.arange(60) % 5).astype(np.int32)
    if not (sc["lights"]["type"] == scenes.LIGHT_INFINITE).any():
        sc = scenes.with_lights(sc, scenes._lights([(scenes.LIGHT_INFINITE, (0.6, 0.6, 0.6), -1, 0, 1)]))
    inf = _infinite(sc)
    rgb = _sun_map(level=200.0)
    osc, gsc = _pair(hip_ctx, sc, lambda s: s.set_environment_map(inf, rgb, ROT))
    cam = scenes.instanced_camera(W, H, extent=1.5)
    for strategy in (1, 2):
        _check(osc, gsc, cam, W, H, 4, max_depth=6, light_strategy=strategy, seed=47)
    gsc.close()
    osc.close()


@pytest.mark.parametrize("integrator,kw", [(pbrt_hip.INTEGRATOR_PATH, dict(max_depth=8, light_strategy=1)),
                                           (pbrt_hip.INTEGRATOR_DIRECT, dict(max_depth=3, light_strategy=0)),
                                           (pbrt_hip.INTEGRATOR_WHITTED, dict(max_depth=5)),
                                           (pbrt_hip.INTEGRATOR_AO, dict(ao_samples=8))])
def test_li_on_a_glossy_scene_under_a_map(hip_ctx, integrator, kw):
    """Scene.li against OracleScene.li on arbitrary rays, held as test_gpu_li.py holds them."""
    sc = _glossy_mixed()
    rgb, inf = _map_300x140(), _infinite(sc)
    osc, gsc = _pair(hip_ctx, sc, lambda s: s.set_environment_map(inf, rgb, ROT))
    n = 3001
    rays = scenes.random_rays(n, 17, origin_extent=1.2)
    keys = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(12345)
    for skip in (0, 5):
        cpu, st_c = osc.li(rays, keys, integrator=integrator, draws_before_li=skip, **kw)
        gpu, st_g = gsc.li(rays, keys, integrator=integrator, draws_before_li=skip, **kw)
        assert st_g["rays_closest"] + st_g["rays_shadow"] == st_c["rays"]
        assert np.all(np.abs(gpu - cpu) <= 1e-5 * np.maximum(1.0, np.abs(cpu))), np.abs(gpu - cpu).max()
    assert cpu.max() > 0.01
    gsc.close()
    osc.close()
