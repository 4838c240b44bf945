"""The cases of test_gpu_shape_materials.py with the float64 models alone (shape_material_cases.py): enough rays survive the
exclusions in every case, the point-light test can fail (a wrong tangent frame misses the reference by far more than the
allowance), the point light is generic, and the lossless glass sphere's closed form against a direct simulation. No GPU."""
import numpy as np
import pytest

import bxdf_model as bm
import quadric_model as qm
import shape_material_cases as smc
from test_quadric_model import TRANSFORMS


def test_point_lights_are_generic():
    """every place a case's light may stand is on no object axis of the shape's transform (the tangent frame turns about those),
    and LIGHT_P lies outside every shape's bound"""
    for name, rec, _, _ in smc.POINT_CASES:
        shape = qm.from_record(rec[0])
        lin = shape["o2w"][:3, :3]
        axes = lin / np.sqrt((lin ** 2).sum(axis=0))
        for light in smc.light_candidates(shape):
            to_light = light - shape["o2w"][:3, 3]
            assert np.abs(axes.T @ to_light / np.linalg.norm(to_light)).max() < 0.99, (name, light)
    assert np.linalg.norm(smc.LIGHT_P) > 3.0 + 2.0


@pytest.mark.parametrize("case", smc.POINT_CASES, ids=smc.POINT_IDS)
def test_point_light_cases_keep_enough_rays_and_can_fail(case):
    """At least MIN_KEPT of the N_RAYS rays survive the exclusions (near, self-shadowed or nearly, |cos| < 0.1, the BSDF's
    discontinuity band, reference 0), and on at least half of them each wrong tangent frame (ss := ts; dpdu left in object space;
    dpdu through the inverse transpose) misses the reference by more than 10 x that ray's allowance: the case is neither
    isotropic nor axis-aligned. The last two only where the transform makes them differ from the right frame. The plastic row
    is isotropic (the library refuses another): turning the frame about the normal changes nothing, which is asserted too."""
    name, rec, row_name, _ = case
    shape, row = qm.from_record(rec[0]), smc.ROWS[row_name]
    light, o, d = smc.point_setup(case)
    c = smc.point_light_case(shape, row, light, o, d)
    keep = c["keep"]
    shares = {}
    for v, wrong in c["wrong"].items():
        shares[v] = float((np.abs(wrong[keep] - c["ref"][keep]) > 10.0 * c["allow"][keep]).any(axis=1).mean())
    print(f"{name}: light {np.round(light, 3)}, kept {keep.sum()} of {len(o)}, median relative allowance "
          f"{np.median(c['allow'][keep] / c['ref'][keep]):.3g}, share of kept rays a wrong frame moves by > 10 allowances: {shares}")
    assert keep.sum() >= smc.MIN_KEPT
    if row["anisotropic"]:
        for v in smc.FRAMES[1:]:
            if smc.frame_differs(shape, v):
                assert shares[v] >= 0.5, (name, v, shares[v])
    else:
        assert shares["swapped"] == 0.0


@pytest.mark.parametrize("name,rec", smc.MIRROR_CASES, ids=[c[0] for c in smc.MIRROR_CASES])
def test_mirror_cases_keep_enough_rays(name, rec):
    shape = qm.from_record(rec[0])
    o, d = smc.select_rays(shape)
    c = smc.mirror_case(shape, o, d)
    rel = c["allow"][c["keep"]] / c["ref"][c["keep"]]
    print(f"{name}: kept {c['keep'].sum()} of {len(o)}, relative allowance median {np.median(rel):.3g} worst {rel.max():.3g}")
    assert c["keep"].sum() >= smc.MIN_KEPT
    if name.startswith("sphere"):
        assert c["keep"].sum() >= 0.95 * len(o)  # a convex body seen from outside: only `near` excludes
    # the map has contrast: a normal off by a degree moves the expectation by far more than the allowance on most rays
    tilted = smc.mirror_expectation(shape, o, d + np.float32(0.02) * np.roll(d, 1, axis=1), qm.intersect(shape, o, d)["t"])[0]
    assert (np.abs(tilted - c["ref"])[c["keep"]] > 10.0 * c["allow"][c["keep"]]).any(axis=1).mean() > 0.5


def test_glass_sphere_share_against_a_simulation():
    """1 - (1 - R) R^(D - 1), the closed form the GPU test uses, against the walk it stands for: reflect at the first hit with
    probability R (Le), else at each of the internal hits 1 .. D - 1 leave with probability 1 - R (Le); still inside at hit D: 0."""
    rng = np.random.default_rng(5)
    for cos in (1.0, 0.5, 0.1, 0.03):
        R = float(bm.fr_dielectric(np.array([cos]), 1.0, smc.GLASS_ETA)[0])
        n = 400_000
        out = rng.random(n) < R
        for _ in range(smc.GLASS_DEPTH - 1):
            out |= ~out & (rng.random(n) >= R)
        p = 1.0 - (1.0 - R) * R ** (smc.GLASS_DEPTH - 1)
        assert abs(out.mean() - p) <= 4.0 * np.sqrt(max(p * (1.0 - p), 1e-12) / n) + 1e-12, (cos, out.mean(), p)
    shape = qm.from_record(smc.scenes.sphere_shape(0.8, to_world=TRANSFORMS["rigid"])[0])
    o, d = smc.select_rays(shape, n=smc.GLASS_RAYS)
    share, skip = smc.glass_sphere_share(shape, o, d)
    assert skip.mean() <= 0.05 and ((share > 0.9) & (share <= 1.0)).all() and (share < 1.0 - 1e-6).any()


@pytest.mark.parametrize("body", list(smc.FURNACE_BODIES))
def test_furnace_rays_see_a_free_hemisphere(body):
    """every direction of the hemisphere about the viewer-side normal leaves the hit point without meeting the shape again"""
    rec = smc.FURNACE_BODIES[body]
    shape = qm.from_record(rec[0])
    o, d = smc.furnace_rays(shape, body.split("-")[0])
    m = qm.intersect(shape, o, d)
    fr = qm.surface_frame(shape, m)
    rng = np.random.default_rng(2)
    for i in range(len(o)):
        w = rng.normal(size=(500, 3))
        w /= np.sqrt((w ** 2).sum(axis=1))[:, None]
        side = np.sign((fr["ns"][i] * -d[i].astype(np.float64)).sum())
        w_world = w[:, :1] * fr["ss"][i] + w[:, 1:2] * fr["ts"][i] + side * np.abs(w[:, 2:]) * fr["ns"][i]
        blocked, _ = qm.occluded_from_surface(shape, np.repeat(m["p"][i:i + 1], 500, axis=0), w_world)
        assert not blocked.any()


@pytest.mark.parametrize("name", smc.NARROW_LIGHTS)
def test_narrow_lobe_reference_is_carried_by_the_bsdf_branch(name):
    """the geometry of the narrow-lobe test puts more than half of the estimate on estimate_direct's BSDF-sampled branch at every
    plane point, the eye's ray meets nothing before the plane, and the quadrature's halving error is small beside the value"""
    setup = smc.narrow_setup(name)
    value, err, share = smc.narrow_reference(name)
    print(f"{name}: radiance {value[:, 1]}, quadrature error {err[:, 1]}, BSDF-branch share {share}")
    assert (share > 0.5).all() and (share <= 1.0 + 1e-9).all()
    assert (value > 0.0).all() and (err < 0.01 * value).all()
    o, d = smc.narrow_rays(setup)
    m = qm.intersect(qm.from_record(setup["rec"][0]), o, d)
    t_plane = (setup["y"] - o[:, 1].astype(np.float64)) / d[:, 1].astype(np.float64)
    assert (t_plane > 0.0).all() and (~m["hit"] | (m["t"] > t_plane * (1.0 + 1e-6))).all()
