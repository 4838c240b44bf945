"""estimate_direct (csrc/wf_lights.h: estimate_direct_emit / estimate_direct_resolve) for the level-2 rows (matte with sigma,
rough glass, substrate), the Disney rows and the lobe rows (uber, translucent, mix) under a finite area light and under an image
environment map, held to float64 quadratures of the models (mis_cases.py; held to themselves on the CPU by test_mis_model.py).
The older tests of these rows use point lights, which take no BSDF-sampled half and no MIS weight, and a constant environment,
which both halves see alike; here the scattering pdf in the light half's weight (transmission side included), LobeBsdf's
non-specular mask, light_triangle_intersect and the area-to-solid-angle pdf of a mesh emitter along a BSDF-sampled direction,
the emitter-identity and emitting-side tests (from below a transmissive sheet too), env_pdf / env_le under a rotated map, and the
specular lobes of a lobe row beside its other lobes (PF_SPECULAR_BOUNCE, the specular branches of direct lighting and Whitted)
all move the expectation. Kernels: k_shade<BIN, 2|3>, k_shade_lobes<BIN>, k_shade_direct<MODE, 2|3|19>.

Each comparison is a batch of N rays through Scene.li at one plane point with fixed stream keys, so a result repeats.
Acceptance: |mean - ref| <= 5 se + the quadrature's error + 1e-4 ref per channel (se: the sample standard error; 1e-4: the
float32 allowance of the project's furnace tests; 5 se and not 4: the file makes some 5000 comparisons, so a correct library
would miss one in about three sets of keys at 4 se and one in 350 at 5), with the conditions that make it mean something
asserted beside it: the quadrature's error below se / 4, and 5 se <= 0.1 ref (N_SAMPLES raises N where 8192 samples miss
that; NO_WHITTED names the comparisons that 65536 would not bring there). Where nothing arrives (the emitter faces away)
every sample is 0."""
import numpy as np
import pytest

import pbrt_hip

import mis_cases as mc

pytestmark = pytest.mark.gpu
PATH, DIRECT, WHITTED = pbrt_hip.INTEGRATOR_PATH, pbrt_hip.INTEGRATOR_DIRECT, pbrt_hip.INTEGRATOR_WHITTED
N = 8192
# Samples per point where 8192 leave 5 se above 0.1 ref: case id -> N, at most 65536. From a run at 8192: the next power of two
# above 1.3 (5 se / (0.1 ref))^2 times as many.
_X2, _X4, _X8 = 2 * N, 4 * N, 8 * N
N_SAMPLES = {
    "substrate-eye+1-light+1-near": _X2, "rough_glass-eye+1-light+1-near": _X4, "rough_glass-eye+1-light-1-near": _X4,
    "rough_glass-eye+1-light-1-far": _X4, "rough_glass-eye-1-light+1-near": _X2, "rough_glass-eye-1-light+1-far": _X2,
    "disney_spec_trans-eye+1-light-1-near": _X8, "disney_spec_trans-eye+1-light-1-far": _X4, "disney_thin-eye+1-light-1-near": _X4,
    "disney_thin-eye+1-light-1-far": _X2, "uber-eye+1-light-1-near": _X2, "uber-eye+1-light-1-far": _X2, "translucent-eye+1-light-1-near": _X4,
    "translucent-eye-1-light+1-near": _X2,
    "disney_opaque-eye+1-dir1": _X2, "substrate-eye+1-dir0": _X8, "mix_matte_metal-eye+1-dir0": _X4, "mix_matte_metal-eye+1-dir1": _X8,
    "translucent-eye+1-dir0": _X8, "translucent-eye+1-dir1": _X8, "translucent-eye-1-dir1": _X4, "uber-eye-1-dir1": _X2, "disney_thin-eye-1-dir1": _X4}
# Where Whitted is left out: it samples each light once and has no BSDF-sampled half, so a lobe of alpha 0.1 to 0.25 on a large
# emitter or under the map's bright block leaves 5 se at 2.7 to 13 times 0.1 ref at 8192 samples: 65536 would not do. The other
# estimators of these cases stay.
NO_WHITTED = {
    "rough_glass-eye+1-light-1-near", "rough_glass-eye-1-light+1-near", "disney_spec_trans-eye+1-light-1-near", "disney_thin-eye+1-light-1-near",
    "translucent-eye+1-light-1-near",
    "substrate-eye+1-dir1", "rough_glass-eye+1-dir0", "rough_glass-eye+1-dir1", "rough_glass-eye-1-dir0", "rough_glass-eye-1-dir1",
    "disney_spec_trans-eye+1-dir0", "disney_spec_trans-eye+1-dir1", "disney_spec_trans-eye-1-dir0", "disney_spec_trans-eye-1-dir1",
    "disney_thin-eye+1-dir0", "disney_thin-eye+1-dir1", "disney_thin-eye-1-dir0", "translucent-eye-1-dir0"}
LIGHT_CASES = [(v, e) for v in mc.VIEWS for e in mc.EMITTERS]
LIGHT_IDS = [f"{mc.view_name(v)}-{e}" for v, e in LIGHT_CASES]


_ENV_IDS = [mc.env_view_name(v) for v in mc.ENV_VIEWS]
assert set(N_SAMPLES) | NO_WHITTED <= set(LIGHT_IDS) | set(_ENV_IDS) and max(N_SAMPLES.values()) <= 65536


def light_estimators(specular):
    """path with both light strategies at depth 1, path at depth 5 (the same reference: the emitter's own row is black, and Le
    met after a non-specular bounce is not added), direct lighting with both strategies, Whitted; the last two at depth 2 where
    the row has specular lobes (their specular branches)"""
    d = 2 if specular else 1
    return {"path-all-1": dict(integrator=PATH, max_depth=1, light_strategy=0), "path-one-1": dict(integrator=PATH, max_depth=1, light_strategy=1),
            "path-one-5": dict(integrator=PATH, max_depth=5, light_strategy=1), "direct-all": dict(integrator=DIRECT, max_depth=d, light_strategy=0),
            "direct-one": dict(integrator=DIRECT, max_depth=d, light_strategy=1), "whitted": dict(integrator=WHITTED, max_depth=d, light_strategy=0)}


def env_estimators(specular):
    d = 2 if specular else 1
    return {"path-1": dict(integrator=PATH, max_depth=1, light_strategy=1), "direct": dict(integrator=DIRECT, max_depth=d, light_strategy=0),
            "whitted": dict(integrator=WHITTED, max_depth=d, light_strategy=0)}


def compare(what, rgb, n_points, n, ref, err):
    """the acceptance of one batch: (worst |mean - ref| / allowance, worst 5 se / (0.1 ref), worst error / (se / 4), failures)"""
    v = rgb.astype(np.float64).reshape(n_points, n, 3)
    mean, se = v.mean(axis=1), v.std(axis=1, ddof=1) / np.sqrt(n)
    fails = []
    if not np.isfinite(v).all():
        fails.append(f"{what}: not finite")
    dark = ref == 0.0
    if dark.any() and not (v[np.broadcast_to(dark[:, None, :], v.shape)] == 0.0).all():
        fails.append(f"{what}: samples other than 0 where nothing arrives: mean {mean[dark]}")
    lit = ~dark
    if not lit.any():
        return 0.0, 0.0, 0.0, fails
    allow = 5.0 * se + err + 1e-4 * ref
    ratio = np.where(lit, np.abs(mean - ref) / np.where(lit, allow, 1.0), 0.0)
    power = np.where(lit, 5.0 * se / np.where(lit, 0.1 * ref, 1.0), 0.0)
    fine = np.where(lit, err / np.where(lit, se / 4.0 + 1e-12, 1.0), 0.0)
    if ratio.max() > 1.0:
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        fails.append(f"{what}: point {k[0]} channel {k[1]}: mean {mean[k]:.6g} ref {ref[k]:.6g} se {se[k]:.3g} error {err[k]:.3g}, {ratio[k]:.2f} allowances")
    if power.max() > 1.0:
        fails.append(f"{what}: 5 se is {power.max():.2f} of 0.1 ref: N must be {power.max() ** 2:.1f} times as large")
    if fine.max() > 1.0:
        fails.append(f"{what}: the quadrature's error is {fine.max():.2f} of se / 4")
    return float(ratio.max()), float(power.max()), float(fine.max()), fails


@pytest.mark.parametrize("view,emitter", LIGHT_CASES, ids=LIGHT_IDS)
def test_area_light(hip_ctx, view, emitter):
    """The row on a large plane under a rectangular mesh emitter of two triangles, one diffuse area light each, on a black matte
    row: `near` (2 x 2 at 0.5, one-sided, the lobes aimed at it: by the model the BSDF-sampled half carries up to 0.96 of the
    estimate), `far` (1.0 x 0.6 at height 1, two-sided, the lobes aimed past it: the light-sampled half carries it) and `away`
    (`near` facing away from the plane: every sample is 0), with eye and emitter on either side of the plane as the view says.
    Four plane points, the scene once axis-aligned and once with every position and ray under a rigid rotation (general ss / ts
    through the anisotropic rows; the reference is the same), six estimators. Reference: mis_cases.light_reference, the
    quadrature over the rectangle plus the specular lobes' term."""
    row, ref = mc.ROWS[view[0]], mc.light_reference(view, emitter)
    case = f"{mc.view_name(view)}-{emitter}"
    n = N_SAMPLES.get(case, N)
    keys = np.arange(len(mc.POINTS) * n, dtype=np.uint64) * 13 + 7
    worst, fails = np.zeros(3), []
    for orientation, rotation in mc.ORIENTATIONS.items():
        sc, after = mc.light_scene(row, emitter, view[2], rotation)
        scene = pbrt_hip.Scene(hip_ctx, sc)
        after(scene)
        rays = np.repeat(mc.view_rays(view, emitter, rotation), n)
        for name, kw in light_estimators(row.specular is not None).items():
            if name == "whitted" and case in NO_WHITTED:
                continue
            *figures, f = compare(f"{case} {orientation} {name}", scene.li(rays, keys, **kw)[0], len(mc.POINTS), n, ref["ref"], ref["err"])
            worst = np.maximum(worst, figures)
            fails += f
        scene.close()
    print(f"{case} [{row.family}] N {n}: worst |mean - ref| / allowance {worst[0]:.3f}, worst 5 se / (0.1 ref) {worst[1]:.3f}, "
          f"worst quadrature error / (se / 4) {worst[2]:.3f}, BSDF-branch share {np.round(ref['share'], 4)}, specular part of green {ref['spec'][:, 1]}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("view", mc.ENV_VIEWS, ids=[mc.env_view_name(v) for v in mc.ENV_VIEWS])
def test_image_environment_map(hip_ctx, view):
    """The row on scenes.glossy_plane_env_scene under a 32 x 16 map (a block 30 times as bright as its 0.2 to 0.5 ground) with a
    light_to_world of two 0.7 rad rotations: two directions per row, from below as well for the rows that transmit; path at depth
    1, direct lighting, Whitted (depth 2 for the last two where the row has specular lobes). Reference:
    mis_cases.env_reference, the quadrature over the sphere in the light's own (theta, phi) plus the specular lobes' term."""
    row, ref = mc.ROWS[view[0]], mc.env_reference(view)
    case = mc.env_view_name(view)
    n = N_SAMPLES.get(case, N)
    keys = np.arange(n, dtype=np.uint64) * 13 + 7
    sc, after = mc.env_scene(row)
    scene = pbrt_hip.Scene(hip_ctx, sc)
    after(scene)
    rays = np.repeat(mc.env_ray(view), n)
    worst, fails = np.zeros(3), []
    for name, kw in env_estimators(row.specular is not None).items():
        if name == "whitted" and case in NO_WHITTED:
            continue
        *figures, f = compare(f"{case} {name}", scene.li(rays, keys, **kw)[0], 1, n, ref["ref"][None, :], ref["err"][None, :])
        worst = np.maximum(worst, figures)
        fails += f
    scene.close()
    print(f"{case} [{row.family}] N {n}: worst |mean - ref| / allowance {worst[0]:.3f}, worst 5 se / (0.1 ref) {worst[1]:.3f}, "
          f"worst quadrature error / (se / 4) {worst[2]:.3f}, BSDF-branch share {ref['share']:.4f}, specular part {ref['spec']}")
    assert not fails, "\n".join(fails)
