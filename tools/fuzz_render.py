"""Fuzz campaign: random small scenes through Integrator::render on the GPU and in the oracle, same seed; every film must agree
to the parity tests' tolerance and every ray count exactly. What the fixed scenes of tests/test_gpu_render.py cannot reach:
random mixes of geometry scale, shared-vertex meshes, materials, light kinds, integrators, samplers, depths, crop windows.
usage: python tools/fuzz_render.py [n_cases] [first_seed] [--glossy-envmap]   (GPU box; prints one line per failing case, exits 1 if any)
--glossy-envmap adds plastic / metal rows (on triangles, spheres and instances; sometimes anisotropic or unremapped through
set_material_roughness) and image maps on the infinite lights to the cases; without it every seed is the case it always was."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pbrt-rs_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import oracle, pbrt_hip
from pbrt_hip import scenes

TOL_PIXEL, TOL_RMSE = 1e-5, 1e-6   # tests/test_gpu_render.py


def grid_mesh(rng, n, scale):
    """A height-field of (n-1)^2 * 2 triangles with shared vertices (ties on edges and vertices are possible)."""
    xs = np.linspace(-1, 1, n)
    g = np.array([[x, rng.uniform(-0.15, 0.15), z] for z in xs for x in xs], dtype=np.float64)
    quads = [(z * n + x, z * n + x + 1, (z + 1) * n + x + 1, (z + 1) * n + x) for z in range(n - 1) for x in range(n - 1)]
    idx = np.array([t for a, b, c, d in quads for t in ((a, c, b), (a, d, c))], dtype=np.int32)
    return (g * scale).astype(np.float32), idx


def glossy_rows(grng):
    """2-3 plastic / metal rows with random Kd / Ks / eta / k and a roughness from 1e-3 to 1, and the roughness calls
    (row offset, u, v, remap) some of them get afterwards"""
    rows, calls = [], []
    for k in range(int(grng.integers(2, 4))):
        r = float(10.0 ** grng.uniform(-3, 0))
        if k == 0 or (k == 2 and grng.random() < 0.5):
            kd = (0.0, 0.0, 0.0) if grng.random() < 0.15 else tuple(grng.uniform(0.05, 0.7, 3))
            ks = (0.0, 0.0, 0.0) if grng.random() < 0.15 else tuple(grng.uniform(0.1, 0.9, 3))
            rows.append(scenes.plastic(kd, ks, r))
            if grng.random() < 0.3:
                calls.append((k, r, r, False))
        else:
            k_ = (0.0, 0.0, 0.0) if grng.random() < 0.1 else tuple(grng.uniform(0.0, 5.0, 3))
            rows.append(scenes.metal(tuple(grng.uniform(0.1, 3.0, 3)), k_, r))
            if grng.random() < 0.5:
                calls.append((k, r, float(10.0 ** grng.uniform(-3, 0)), bool(grng.integers(0, 2))))
    return rows, calls


def environment_maps(grng, lights):
    """image maps for some of the infinite lights: (light, rgb, light_to_world or None); 1x1 to 64x32, powers of two and not"""
    maps = []
    for i in np.nonzero(lights["type"] == scenes.LIGHT_INFINITE)[0]:
        if grng.random() < 0.65:
            w, h = [(1, 1), (2, 1), (4, 2), (8, 4), (16, 8), (64, 32), (3, 2), (5, 7), (24, 10), (50, 20), (64, 32), (33, 17)][int(grng.integers(0, 12))]
            rgb = grng.uniform(0.05, 1.5, (h, w, 3)).astype(np.float32)
            if grng.random() < 0.35:
                rgb[int(grng.integers(0, h)), int(grng.integers(0, w))] = grng.uniform(50, 500, 3).astype(np.float32)
            m = None
            if grng.random() < 0.5:
                m = np.eye(4, dtype=np.float32)
                m[:3, :3] = scenes._random_rigid(grng.uniform(0, 1, 3))[:3, :3].astype(np.float32)
            maps.append((int(i), rgb, m))
    return maps


def make_case(seed, glossy_envmap=False):
    rng = np.random.default_rng(seed)
    grng = np.random.default_rng(seed ^ 0x910557e)   # --glossy-envmap: its own generator, the draws below stay what they were
    roughness_calls, n_glossy = [], 0
    scale = float(rng.choice([0.01, 1.0, 1.0, 1.0, 300.0]))
    kind = rng.choice(["cloud", "grid", "cloud+grid", "cornell"])
    pos, idx = [], []
    if kind == "cornell":
        sc = scenes.cornell_box()
        cam_eye = None
    else:
        if "cloud" in kind:
            n = int(rng.integers(1, 400))
            c = scenes.random_triangles(n, seq=int(rng.integers(1, 1000)), extent=1.0, size=float(rng.choice([0.02, 0.1, 0.4])))
            pos.append(c["positions"] * np.float32(scale)); idx.append(c["indices"])
        if "grid" in kind:
            gp, gi = grid_mesh(rng, int(rng.integers(2, 9)), scale)
            gi = gi + (len(pos[0]) if pos else 0)
            pos.append(gp); idx.append(gi)
        positions, indices = np.concatenate(pos).astype(np.float32), np.concatenate(idx).astype(np.int32)
        n_t = len(indices)
        mats = scenes._materials([(scenes.MAT_MATTE, tuple(rng.uniform(0.2, 0.8, 3)), (0, 0, 0), 1.0),
                                  (scenes.MAT_MIRROR, (0.9, 0.9, 0.9), (0, 0, 0), 1.0),
                                  (scenes.MAT_GLASS, (1.0, 1.0, 1.0), (0.95, 0.95, 0.95), float(rng.choice([1.33, 1.5, 2.0]))),
                                  (scenes.MAT_NONE, (0, 0, 0), (0, 0, 0), 1.0)])
        pm = rng.choice([[1, 0, 0, 0], [0.6, 0.2, 0.2, 0.0], [0.5, 0.2, 0.2, 0.1]])
        tri_material = rng.choice(4, n_t, p=np.array(pm, dtype=np.float64)).astype(np.int32)
        tri_light = np.full(n_t, -1, dtype=np.int32)
        lights = []
        if rng.random() < 0.75:
            lights.append((scenes.LIGHT_INFINITE, tuple(rng.uniform(0.2, 1.0, 3)), -1, 0, 1))
        for _ in range(int(rng.integers(0, 4)) if rng.random() < 0.8 else int(rng.integers(4, 14))):   # area lights on random triangles
            t = int(rng.integers(0, n_t))
            if tri_light[t] < 0:
                tri_light[t] = len(lights)
                tri_material[t] = 0
                lights.append((scenes.LIGHT_DIFFUSE_AREA, tuple(rng.uniform(2, 20, 3)), t, int(rng.integers(0, 2)), int(rng.integers(1, 3))))
        if rng.random() < 0.3:
            lights.append(scenes.point_light(tuple(rng.uniform(-1.5, 1.5, 3) * scale), tuple(rng.uniform(1, 5, 3) * scale * scale)))
        if rng.random() < 0.2:
            lights.append(scenes.distant_light(tuple(rng.normal(size=3)), tuple(rng.uniform(0.5, 2, 3))))
        if rng.random() < 0.2:
            lights.append(scenes.spot_light(tuple(rng.uniform(1, 2, 3) * scale), (0.0, 0.0, 0.0), tuple(rng.uniform(2, 8, 3) * scale * scale)))
        if not lights:
            lights.append((scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1))
        if glossy_envmap and grng.random() < 0.8:
            rows, calls = glossy_rows(grng)
            n_glossy = len(rows)
            roughness_calls = [(len(mats) + k, u, v, remap) for k, u, v, remap in calls]
            mats = np.concatenate([mats, scenes._materials(rows)])
            pick = (grng.random(n_t) < float(grng.choice([0.1, 0.4, 0.9]))) & (tri_light < 0)
            tri_material[pick] = (len(mats) - n_glossy + grng.integers(0, n_glossy, n_t))[pick].astype(np.int32)
        extra = {}
        r_extra = rng.random()
        if r_extra < 0.2:
            # full spheres placed by a translation beside the triangles (sphere.rs), some of them area lights: primitive n_t + i
            sph = []
            for k in range(int(rng.integers(1, 4))):
                light = -1
                if rng.random() < 0.4:
                    light = len(lights)
                    lights.append((scenes.LIGHT_DIFFUSE_AREA, tuple(rng.uniform(2, 12, 3)), n_t + k, 0, int(rng.integers(1, 3))))
                sph.append([*(rng.uniform(-0.8, 0.8, 3) * scale), float(rng.uniform(0.1, 0.5)) * scale, 0 if light >= 0 else int(rng.integers(0, 3)), light, 0, 0])
            extra["spheres"] = np.array(sph, dtype=np.float32)
            for row in extra["spheres"]:
                if n_glossy and row[5] < 0 and grng.random() < 0.4:
                    row[4] = len(mats) - n_glossy + int(grng.integers(0, n_glossy))
        elif r_extra < 0.35 and not any(tri_light >= 0):
            # TransformedPrimitive instances of the mesh, material by instance (primitive.rs:105-159; instances carry no area lights)
            n_inst = int(rng.integers(1, 12))
            inst = np.zeros((n_inst, 2, 4, 4), dtype=np.float32)
            for k in range(n_inst):
                m = scenes._random_rigid(rng.uniform(0, 1, 3))
                m[:3, 3] = rng.uniform(-1.2, 1.2, 3) * scale
                inst[k, 0], inst[k, 1] = m.astype(np.float32), np.linalg.inv(m).astype(np.float32)
            inst[:, :, 3, :] = (0, 0, 0, 1)
            extra["instances"] = inst
            extra["instance_material"] = rng.integers(-1, 3, n_inst).astype(np.int32)
            if n_glossy:
                pick = grng.random(n_inst) < 0.3
                extra["instance_material"][pick] = (len(mats) - n_glossy + grng.integers(0, n_glossy, n_inst))[pick]
        sc = dict(positions=positions, indices=indices, tri_material=tri_material, materials=mats, tri_light=tri_light,
                  lights=scenes._lights(lights), **extra)
        if not extra and rng.random() < 0.12:
            # the general two-level scene: this mesh cut into 1-3 object aggregates, instances of them, and world-space triangles
            # (a floor and, sometimes, an emitting quad) beside the instances in the top-level leaves (primitive.rs:105-159)
            n_obj = int(rng.integers(1, 4))
            cuts = np.sort(rng.choice(np.arange(1, max(n_t, 2)), size=min(n_obj - 1, max(n_t - 1, 0)), replace=False)) if n_t > 1 else np.array([], dtype=np.int64)
            parts = np.split(np.arange(n_t), cuts)
            objs = [dict(positions=positions, indices=indices[p_], tri_material=tri_material[p_]) for p_ in parts if len(p_)]
            n_inst = int(rng.integers(1, 10))
            inst = np.zeros((n_inst, 2, 4, 4), dtype=np.float32)
            for k in range(n_inst):
                m = scenes._random_rigid(rng.uniform(0, 1, 3))
                m[:3, 3] = rng.uniform(-1.0, 1.0, 3) * scale
                inst[k, 0], inst[k, 1] = m.astype(np.float32), np.linalg.inv(m).astype(np.float32)
            inst[:, :, 3, :] = (0, 0, 0, 1)
            e = 1.8 * scale
            wp = np.array([[-e, -1.3 * scale, -e], [e, -1.3 * scale, -e], [e, -1.3 * scale, e], [-e, -1.3 * scale, e],
                           [-0.5 * scale, 1.5 * scale, -0.5 * scale], [0.5 * scale, 1.5 * scale, -0.5 * scale], [0.5 * scale, 1.5 * scale, 0.5 * scale], [-0.5 * scale, 1.5 * scale, 0.5 * scale]], dtype=np.float32)
            wi = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7]], dtype=np.int32)
            wl = np.array([-1, -1, -1, -1], dtype=np.int32)
            lts = [l for l in lights if not (isinstance(l, tuple) and l[0] == scenes.LIGHT_DIFFUSE_AREA)]   # instanced triangles carry no area lights
            if rng.random() < 0.6:
                wl[2], wl[3] = len(lts), len(lts) + 1
                lts += [(scenes.LIGHT_DIFFUSE_AREA, (12.0, 11.0, 9.0), 2, 0, 1), (scenes.LIGHT_DIFFUSE_AREA, (12.0, 11.0, 9.0), 3, 0, 1)]
            if not lts:
                lts.append((scenes.LIGHT_INFINITE, (1.0, 1.0, 1.0), -1, 0, 1))
            sc = dict(objects=objs, instances=inst, instance_object=rng.integers(0, len(objs), n_inst).astype(np.int32),
                      instance_material=rng.integers(-1, 3, n_inst).astype(np.int32),
                      world=dict(positions=wp, indices=wi, tri_material=np.zeros(4, dtype=np.int32), tri_light=wl),
                      materials=mats, lights=scenes._lights(lts), positions=positions, indices=indices)
            if n_glossy:
                pick = grng.random(n_inst) < 0.3
                sc["instance_material"][pick] = (len(mats) - n_glossy + grng.integers(0, n_glossy, n_inst))[pick]
        elif not extra and rng.random() < 0.25:
            # TriangleMesh n / s / uv (triangle.rs:17-26, 252-312): shading frames from per-vertex data
            sc = scenes.with_vertex_shading(sc, seq=int(rng.integers(1, 1000)), normals=bool(rng.integers(0, 2)), uvs=bool(rng.integers(0, 2)) or True,
                                            tangents=bool(rng.integers(0, 2)))
        cam_eye = tuple(np.array([rng.uniform(-1, 1), rng.uniform(0.3, 1.5), rng.uniform(2.0, 3.5)]) * scale)
    w, h = int(rng.choice([24, 33, 48])), int(rng.choice([16, 24, 31]))
    if cam_eye is None:
        cam = scenes.cornell_camera(w, h)
    else:
        ck = rng.choice(["perspective", "perspective", "perspective", "orthographic", "environment"])
        if ck == "orthographic":     # cameras/orthographic.rs:82-104
            cam = scenes.orthographic_camera(cam_eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.3 * scale, w, h,
                                             lens_radius=float(rng.choice([0.0, 0.05 * scale])), focal_distance=3.0 * scale)
        elif ck == "environment":    # cameras/environment.rs:37-56
            cam = scenes.environment_camera(tuple(np.array(cam_eye) * 0.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        else:
            cam = scenes.perspective_camera(cam_eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), float(rng.uniform(25, 60)), w, h,
                                            lens_radius=float(rng.choice([0.0, 0.0, 0.05 * scale])), focal_distance=3.0 * scale)
    integ = int(rng.choice([0, 0, 0, 1, 2, 3]))
    kw = dict(integrator=integ, max_depth=int(rng.integers(1, 9)) if rng.random() < 0.85 else int(rng.integers(9, 20)), seed=int(rng.integers(0, 1 << 30)))
    if rng.random() < 0.15:
        kw["max_sample_luminance"] = float(rng.choice([0.5, 2.0, 10.0]))   # Film::max_sample_luminance (film.rs:253-255)
    if integ == 0:
        kw.update(rr_threshold=float(rng.choice([1.0, 0.3])), light_strategy=int(rng.integers(0, 3)))
    elif integ == 1:
        kw.update(light_strategy=int(rng.integers(0, 2)))
    elif integ == 3:
        kw.update(ao_samples=int(rng.integers(1, 9)), cos_sample=bool(rng.integers(0, 2)))
    smp = rng.choice(["random", "random", "stratified", "zerotwo", "halton"])
    spp = int(rng.choice([1, 2, 4]))
    if np.random.default_rng(seed ^ 0x64a).random() < 0.03:   # round 5: a pass of 64 samples = one pixel per wave (k_film_accumulate_rows)
        spp = 64
    if smp == "stratified":
        kw["sampler"] = ("stratified", 2, spp, bool(rng.integers(0, 2)), int(rng.integers(0, 5)))
    elif smp == "zerotwo":
        kw["sampler"] = ("zerotwo", int(rng.integers(0, 5)))
    elif smp == "halton":
        kw["sampler"] = ("halton",)
    gpu_only = dict(shade_order=int(rng.integers(0, 3)), spp_per_pass=int(rng.integers(0, 3)), ray_order=int(rng.integers(0, 2)))   # must not change the film
    # round 5: the dealing order of the tiles (its own generator: the draws of the cases above stay what they were)
    gpu_only["tile_order"] = int(np.random.default_rng(seed ^ 0x71e0).integers(0, 2))
    gpu_only["samples_per_wave"] = int(np.random.default_rng(seed ^ 0x5a3e).choice([0, 0, 1, 2, 4, 16, 64]))   # the path layout over the waves
    opts_layout = int(np.random.default_rng(seed ^ 0x11e5).integers(0, 3))   # pbrt_hip_context_set_wide_layout: by size / packed / lines
    plain = "spheres" not in sc and "instances" not in sc and "objects" not in sc and "normals" not in sc and "uvs" not in sc and "tangents" not in sc
    opts = dict(device_build=bool(plain and rng.random() < 0.2),     # the tree built on the device (HLBVH) against the oracle's HLBVH
                tile_split=int(rng.choice([1, 1, 2, 3])),              # the frame as the sum of the ranks' tile shares
                # pbrt_hip_context_set_traversal: wide records / binary + stack / binary stackless (single-level triangle scenes)
                # (its own generator: the draws of the cases above stay what they were in profiles/r03_fuzz.txt)
                layout=opts_layout,
                traversal=int(np.random.default_rng(seed ^ 0x7ac3).choice([0, 0, 1, 2] if ("spheres" not in sc and "instances" not in sc and "objects" not in sc) else [0, 0, 1])))
    r_f = rng.random()
    if r_f < 0.3:
        x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
        kw["bounds"] = (x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1)))
    elif r_f < 0.42:
        # a wider reconstruction filter (src/filters/*.rs, FilmTile::add_sample film.rs:252-295): float atomics on the GPU, tile
        # merges in the oracle — only the order of the additions differs (tests/test_gpu_render.py::test_reconstruction_filters)
        fk = [("gaussian", 2.0, 2.0, 0.0), ("mitchell", 2.0, 1 / 3, 1 / 3), ("triangle", 1.5, 0.0, 0.0), ("lanczos", 3.0, 3.0, 0.0)][int(rng.integers(0, 4))]
        kw["filter"] = pbrt_hip.filter_table(fk[0], fk[1], fk[1], fk[2], fk[3])
    opts["roughness"] = roughness_calls
    opts["maps"] = environment_maps(grng, sc["lights"]) if glossy_envmap else []
    opts["glossy_used"] = bool(n_glossy and (np.any(sc.get("tri_material", np.zeros(0)) >= len(sc["materials"]) - n_glossy)
                                             or any(np.any(o["tri_material"] >= len(sc["materials"]) - n_glossy) for o in sc.get("objects", []))
                                             or np.any(sc.get("instance_material", np.zeros(0)) >= len(sc["materials"]) - n_glossy)
                                             or ("spheres" in sc and np.any(sc["spheres"][:, 4] >= len(sc["materials"]) - n_glossy))))
    what = kind + (" +spheres" if "spheres" in sc else "") + (" two-level" if "objects" in sc else " instanced" if "instances" in sc else "")
    what += (" +vertex data" if ("normals" in sc or "uvs" in sc or "tangents" in sc) else "")
    if glossy_envmap:
        what += f" glossy rows {n_glossy} roughness calls {roughness_calls} maps {[(i, m.shape[1], m.shape[0], x is not None) for i, m, x in opts['maps']]}"
    shown = {k: v for k, v in opts.items() if k not in ("roughness", "maps", "glossy_used")}
    return sc, cam, w, h, spp, kw, gpu_only, opts, f"{what} scale {scale} tris {len(sc['indices'])} lights {len(sc['lights'])} {w}x{h}x{spp} {kw} {gpu_only} {shown}"


def main():
    glossy_envmap = "--glossy-envmap" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if a != "--glossy-envmap"]
    n_cases = int(args[0]) if len(args) > 0 else 200
    first = int(args[1]) if len(args) > 1 else 0
    ctx = pbrt_hip.Context(0)
    bad, refused, t0 = 0, 0, time.time()
    mix = dict(glossy=0, maps=0, both=0)
    for seed in range(first, first + n_cases):
        sc, cam, w, h, spp, kw, gpu_only, opts, desc = make_case(seed, glossy_envmap)
        mix["glossy"] += opts["glossy_used"]
        mix["maps"] += bool(opts["maps"])
        mix["both"] += bool(opts["glossy_used"] and opts["maps"])
        ctx.set_traversal(pbrt_hip.TRAVERSAL_AUTO)
        try:
            if opts["device_build"]:
                osc = oracle.OracleScene(sc, split_method=pbrt_hip.SPLIT_HLBVH)
                gsc = pbrt_hip.Scene(ctx, sc, device_build=True)
            else:
                osc = oracle.OracleScene(sc, normals=sc.get("normals"), uvs=sc.get("uvs"), tangents=sc.get("tangents"))
                ctx.set_wide_layout(opts["layout"])
                try:
                    gsc = pbrt_hip.Scene(ctx, sc)
                finally:
                    ctx.set_wide_layout(pbrt_hip.WIDE_LAYOUT_AUTO)
            for scene in (osc, gsc):   # --glossy-envmap: the same roughness calls and maps on both sides
                for m_, u_, v_, remap_ in opts["roughness"]:
                    scene.set_material_roughness(m_, u_, v_, remap=remap_)
                for light_, rgb_, l2w_ in opts["maps"]:
                    scene.set_environment_map(light_, rgb_, l2w_)
            okw = dict(kw)
            film_c, st_c = osc.render(scenes.camera_dict_to_floats(cam), w, h, spp, n_threads=4, **okw)
            ctx.set_traversal(opts["traversal"])
            if opts["tile_split"] == 1:
                film_g, st_g = gsc.render(cam, w, h, spp, **kw, **gpu_only)
            else:   # integrator.rs:412-477 over ranks: the films of the tile shares add up to the frame, their rays to its rays
                film_g, st_g = None, dict(rays_closest=0, rays_shadow=0)
                for rank in range(opts["tile_split"]):
                    f, st = gsc.render(cam, w, h, spp, tile_rank=rank, tile_world=opts["tile_split"], **kw, **gpu_only)
                    film_g = f if film_g is None else film_g + f
                    st_g["rays_closest"] += st["rays_closest"]
                    st_g["rays_shadow"] += st["rays_shadow"]
            li_bad = None
            if "sampler" not in kw and seed % 4 == 0:
                # Integrator::li in batch form (integrator.rs:29-42): arbitrary rays and stream keys against the oracle's li
                lrng = np.random.default_rng(seed ^ 0x5bd1e995)
                n_li = int(lrng.integers(1, 700))
                cen = sc["positions"].mean(axis=0)
                ext = float(np.abs(sc["positions"] - cen).max()) + 1e-6
                lr = scenes.random_rays(n_li, int(lrng.integers(1, 1 << 20)), origin_extent=1.0)
                lr["o"] = (lr["o"] * np.float32(ext * 1.2) + cen).astype(np.float32)
                keys = lrng.integers(0, 1 << 62, n_li).astype(np.uint64)
                lkw = {k: v for k, v in kw.items() if k in ("integrator", "max_depth", "rr_threshold", "light_strategy", "ao_samples", "cos_sample")}
                skip = int(lrng.choice([0, 5]))
                lc, lst_c = osc.li(lr, keys, draws_before_li=skip, **lkw)
                lg, lst_g = gsc.li(lr, keys, draws_before_li=skip, **{k: v for k, v in lkw.items() if k != "cos_sample"},
                                   **({"light_strategy": int(bool(lkw.get("cos_sample", True)))} if lkw.get("integrator") == 3 else {}))
                fin = np.isfinite(lc) & np.isfinite(lg)
                if (lst_g["rays_closest"] + lst_g["rays_shadow"] != lst_c["rays"] or np.any(np.isfinite(lc) != np.isfinite(lg))
                        or np.any(np.abs(lg[fin] - lc[fin]) > 1e-5 * np.maximum(1.0, np.abs(lc[fin])))):
                    li_bad = f"li: rays gpu {lst_g['rays_closest'] + lst_g['rays_shadow']} cpu {lst_c['rays']}, max err {np.abs(lg[fin] - lc[fin]).max() if fin.any() else None}"
            gsc.close(); osc.close()
            rays_g = st_g["rays_closest"] + st_g["rays_shadow"]
            rgb_g, rgb_c = pbrt_hip.film_to_rgb(film_g), oracle.film_to_rgb(film_c)
            err = np.abs(rgb_g - rgb_c)
            if "filter" in kw:
                fin = np.isfinite(film_c) & np.isfinite(film_g)
                ok = (np.all(np.isfinite(film_c) == np.isfinite(film_g)) and np.allclose(film_g[fin], film_c[fin], rtol=5e-5, atol=5e-5 * max(1.0, float(np.abs(film_c[fin]).max(initial=0.0))))
                      and rays_g == st_c["rays"])
            else:
                ok = (np.array_equal(film_g[..., 3], film_c[..., 3]) and np.all(np.isfinite(rgb_g) == np.isfinite(rgb_c))
                      and np.all(err[np.isfinite(err)] <= TOL_PIXEL * np.maximum(1.0, np.abs(rgb_c[np.isfinite(err)])))
                      and rays_g == st_c["rays"])
            if li_bad:
                bad += 1
                print(f"MISMATCH seed {seed}: {desc}\n   {li_bad}", flush=True)
            if not ok:
                bad += 1
                fin = np.isfinite(err)
                print(f"MISMATCH seed {seed}: {desc}\n   rays gpu {rays_g} cpu {st_c['rays']}; max err {err[fin].max() if fin.any() else None}; "
                      f"pixels off {(err > TOL_PIXEL * np.maximum(1.0, np.abs(rgb_c))).any(axis=-1).sum()} of {w * h}", flush=True)
        except pbrt_hip.PbrtHipError as e:
            # the one refusal the generator can reach: Halton sample arrays past the 1000 tabulated dimensions, where the
            # reference panics in start_pixel (halton.rs:100-108 via sampler.rs:355-368) — expected exactly then
            n_arrays = 2 * kw.get("max_depth", 5) * len(sc["lights"]) if (kw.get("integrator") == 1 and kw.get("light_strategy") == 0) else 0
            if "too many sample arrays" in str(e) and kw.get("sampler", ("",))[0] == "halton" and 5 + 2 * n_arrays > 1000:
                refused += 1
            else:
                bad += 1
                print(f"ERROR seed {seed}: {desc}\n   {type(e).__name__}: {e}", flush=True)
        except Exception as e:  # noqa: BLE001
            bad += 1
            print(f"ERROR seed {seed}: {desc}\n   {type(e).__name__}: {e}", flush=True)
        if (seed - first + 1) % 50 == 0:
            print(f"... {seed - first + 1} cases, {bad} bad, {time.time() - t0:.0f} s", flush=True)
    if glossy_envmap:
        print(f"fuzz_render --glossy-envmap: {mix['glossy']} cases with a glossy row in use, {mix['maps']} with an image map, {mix['both']} with both; "
              f"{time.time() - t0:.0f} s", flush=True)
    print(f"fuzz_render: {n_cases} cases from seed {first}: {bad} mismatching"
          + (f" ({refused} refused where the reference panics: Halton arrays past 1000 dimensions)" if refused else ""), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
