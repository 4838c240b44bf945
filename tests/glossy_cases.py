"""The material table, directions and relative check that hold a BSDF implementation to the float64 model
(microfacet_model.py): shared by test_gpu_glossy.py (the device's pbrt_hip_bsdf_query) and test_oracle_microfacet.py (the CPU
oracle's orc_bsdf_query), so both are held with the same cases, masks and tolerances."""
import numpy as np

from pbrt_hip import scenes
import microfacet_model as mm

ETA, K = (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)  # a gold-like conductor


def _table_scene(rows):
    sc = scenes.glossy_plane_point_light_scene(rows[0])
    sc["materials"] = scenes._materials(rows)
    return sc


# (row, roughness call (u, v, remap) or None, model)
CASES = [
    ("plastic_kd_only", scenes.plastic((0.5, 0.4, 0.3), (0, 0, 0), 0.1), None, mm.Material.plastic((0.5, 0.4, 0.3), (0, 0, 0), 0.1)),
    ("plastic_ks_only", scenes.plastic((0, 0, 0), (0.6, 0.5, 0.4), 0.1), None, mm.Material.plastic((0, 0, 0), (0.6, 0.5, 0.4), 0.1)),
    ("plastic_both", scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.3), None, mm.Material.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.3)),
    ("plastic_rough1", scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 1.0), None, mm.Material.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 1.0)),
    ("plastic_alpha_1e-3", scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.1), (1e-3, 1e-3, False),
     mm.Material.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 1e-3, remap=False)),
    ("metal_iso", scenes.metal(ETA, K, 0.01), None, mm.Material.metal(ETA, K, 0.01)),
    ("metal_iso_remap_r1e-3", scenes.metal(ETA, K, 0.001), None, mm.Material.metal(ETA, K, 0.001)),
    ("metal_aniso", scenes.metal(ETA, K, 0.01), (0.15, 0.6, False), mm.Material.metal(ETA, K, 0.15, 0.6, remap=False)),
    ("metal_aniso_remap", scenes.metal(ETA, K, 0.01), (0.05, 0.3, True), mm.Material.metal(ETA, K, 0.05, 0.3)),
    ("metal_k0", scenes.metal((1.5, 1.6, 1.7), (0, 0, 0), 0.2), None, mm.Material.metal((1.5, 1.6, 1.7), (0, 0, 0), 0.2)),
    ("metal_alpha1", scenes.metal(ETA, K, 0.01), (1.0, 1.0, False), mm.Material.metal(ETA, K, 1.0, remap=False)),
    ("matte", (scenes.MAT_MATTE, (0.6, 0.5, 0.4), (0, 0, 0), 1.0), None, mm.Material(mm.MAT_MATTE, (0.6, 0.5, 0.4))),
]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _directions(n, seed):
    rng = np.random.default_rng(seed)
    wo = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    wi = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    # some wi near the mirror direction, where the glossy lobes live
    k = n // 3
    r = wo[:k] * np.array([-1, -1, 1], np.float32)
    wi[:k] = _unit(r + 0.15 * rng.normal(size=(k, 3))).astype(np.float32)
    u = rng.random((n, 2)).astype(np.float32)
    return wo, wi, u


def _rel_check(dev, ref, mask, what, rtol):
    dev, ref, rtol = dev[mask].astype(np.float64), ref[mask], rtol[mask]
    zero = ref == 0
    assert np.all(dev[zero] == 0), f"{what}: device nonzero where the model is 0: {dev[zero][dev[zero] != 0][:5]}"
    err = np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-30)
    bad = (err > rtol) & ~zero
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} beyond {rtol}: worst {err.max():.3g}, dev {dev[bad][:4]} model {ref[bad][:4]}"


# (metal_aniso's alphas (0.15, 0.6) are left out: there the rational fit of the slope_y inverse in trowbridge_reitz_sample11,
# pbrt-v3's / Heitz's approximation, is told apart from the pdf by 10^6 samples in float64 as well)
CHI2 = [("plastic_both", 2, 35.0), ("plastic_both", 2, 80.0), ("metal_aniso_remap", 8, 35.0), ("metal_k0", 9, 20.0),
        ("plastic_ks_only", 1, 60.0), ("metal_iso_below", 9, 140.0)]


def _point_light_rays(n_side=6):
    o = np.array([0.1, 0.2, 3.0])
    xs = np.linspace(-2.5, 2.5, n_side)
    pts = np.array([(x, y, 0.0) for x in xs for y in xs])
    d = _unit(pts - o)
    rays = np.zeros(len(d), dtype=scenes.RAY_DTYPE)
    rays["o"] = o.astype(np.float32)
    rays["d"] = d.astype(np.float32)
    rays["t_max"] = np.inf
    return rays


def _with_glossy_rows(sc):
    sc = dict(sc)
    extra = scenes._materials([scenes.plastic((0.3, 0.2, 0.1), (0.5, 0.5, 0.5), 0.1), scenes.metal(ETA, K, 0.05)])
    sc["materials"] = np.concatenate([sc["materials"], extra])
    return sc


def _glossy_mixed():
    sc = _with_glossy_rows(scenes.mixed_materials_scene(n_tris=3000))
    tm = sc["tri_material"].copy()
    tm[:3000] = np.arange(3000) % 5  # matte, mirror, glass, plastic, metal
    sc["tri_material"] = tm
    return sc


def glossy_envmap_golden():
    """The scene of tests/golden/glossy_envmap_64x64x4.npz: the glossy mixed scene with a 12x6 image map (resampled to 16x8,
    one hot texel, a rotated light_to_world) on its infinite light. Returns (scene, camera, width, height, spp, render keywords,
    light index, map, light_to_world)."""
    from envmap_cases import _rot
    sc = _glossy_mixed()
    light = int(np.nonzero(sc["lights"]["type"] == scenes.LIGHT_INFINITE)[0][0])
    rgb = (0.1 + 0.9 * scenes.pcg32_float(91, 6 * 12 * 3).reshape(6, 12, 3)).astype(np.float32)
    rgb[1, 7] = (40.0, 36.0, 28.0)
    w = h = 64
    return (sc, scenes.random_triangles_camera(w, h), w, h, 4, dict(max_depth=8, light_strategy=1, seed=21), light, rgb,
            _rot((0.3, -0.5, 0.8), 37.0))
