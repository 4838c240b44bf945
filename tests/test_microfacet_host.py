"""Host checks of the plastic / metal BSDF work: the float64 model's own identities (microfacet_model.py: D is normalised, the
visible-normal pdf integrates to one, its sampler's histogram follows the BSDF pdf) and the C ABI of the two materials (enum
values, the two entry points in the header and in the built library, PbrtMaterial still 32 bytes)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import stats

import microfacet_model as mm
import pbrt_hip
from pbrt_hip import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pbrt_hip.h")


def _hemisphere_grid(ax, ay, n=400):
    """nodes and weights over the upper hemisphere of wh: tan^2 theta = a^2 x / (1 - x) (a = sqrt(ax ay)) resolves the peak"""
    a2 = ax * ay
    x, wx = mm.gauss_legendre(n, 0.0, 1.0)
    phi, wp = mm.gauss_legendre(n, 0.0, 2 * np.pi)
    X, P = np.meshgrid(x, phi, indexing="ij")
    t2 = a2 * X / (1 - X)
    c = 1 / np.sqrt(1 + t2)
    dc_dx = 0.5 * (1 + t2) ** -1.5 * a2 / (1 - X) ** 2
    wh = mm.sphere_dir(c, P).reshape(-1, 3)
    return wh, (np.outer(wx, wp) * dc_dx).reshape(-1)


@pytest.mark.parametrize("ax,ay", [(0.05, 0.05), (0.3, 0.3), (0.8, 0.8), (0.2, 0.6), (1.0, 0.1)])
def test_d_is_normalised(ax, ay):
    wh, w = _hemisphere_grid(ax, ay)
    assert np.sum(mm.tr_d(wh, ax, ay) * wh[:, 2] * w) == pytest.approx(1.0, rel=2e-4)


@pytest.mark.parametrize("ax,ay", [(0.1, 0.1), (0.5, 0.5), (0.3, 0.7)])
@pytest.mark.parametrize("theta_o", [0.0, 30.0, 60.0, 85.0])
def test_visible_normal_pdf_integrates_to_one(ax, ay, theta_o):
    t = np.radians(theta_o)
    wo = np.array([[np.sin(t) * np.cos(0.4), np.sin(t) * np.sin(0.4), np.cos(t)]])
    wh, w = _hemisphere_grid(ax, ay, n=800)
    wo = np.broadcast_to(wo, wh.shape)
    # D G1(wo) max(0, wo.wh) / cos theta_o: the distribution of visible normals (tr_pdf takes |wo.wh|, as the reference does;
    # the two differ on the back-facing normals the sampler never returns)
    front = np.sum(wo * wh, -1) > 0
    assert np.sum(np.where(front, mm.tr_pdf(wo, wh, ax, ay), 0.0) * w) == pytest.approx(1.0, rel=1.5e-3)  # the kink at wo.wh = 0


def _chi2_p(counts, expected, n_valid_missing):
    """Pearson chi^2 with the bins of expected count < 5 pooled (and the 'no sample' bin)"""
    exp = np.append(expected, n_valid_missing[1])
    obs = np.append(counts, n_valid_missing[0])
    small = exp < 5
    e = np.append(exp[~small], exp[small].sum())
    o = np.append(obs[~small], obs[small].sum())
    keep = e > 0
    assert np.all(o[~keep] == 0), "samples where the pdf has no mass"
    chi2 = np.sum((o[keep] - e[keep]) ** 2 / e[keep])
    return stats.chi2.sf(chi2, keep.sum() - 1)


@pytest.mark.parametrize("mat", [mm.Material.plastic((0.4, 0.3, 0.2), (0.5, 0.5, 0.5), 0.1),
                                 mm.Material.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.3, 0.6, remap=False),
                                 mm.Material.plastic((0, 0, 0), (1, 1, 1), 0.4, remap=False)], ids=["plastic", "metal_aniso", "ks_only"])
@pytest.mark.parametrize("theta_o", [20.0, 70.0, 110.0])
def test_model_sampler_histogram_matches_its_pdf(mat, theta_o):
    n = 400_000
    t = np.radians(theta_o)
    wo = np.array([np.sin(t) * np.cos(1.1), np.sin(t) * np.sin(1.1), np.cos(t)])
    rng = np.random.default_rng(int(theta_o))
    u = rng.random((n, 2))
    wi, f, pdf, ok, _ = mm.bsdf_sample_f(mat, np.broadcast_to(wo, (n, 3)).copy(), u)
    expected = mm.pdf_bins(mat, wo).reshape(-1) * n
    counts = np.bincount(mm.bin_of(wi[ok]), minlength=expected.size)
    p = _chi2_p(counts, expected, (n - ok.sum(), n - expected.sum()))
    assert p > 1e-3, p
    # what sample_f returns agrees with f / pdf at the sampled direction
    np.testing.assert_allclose(pdf[ok], mm.bsdf_pdf(mat, np.broadcast_to(wo, (n, 3))[ok], wi[ok]), rtol=1e-12)


def test_as_written_sampler_fails_the_histogram():
    """D64 as the reference writes it (slope = alpha^2): every sample is the same normal; the histogram test catches it"""
    mat = mm.Material.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2), 0.5, remap=False)
    wo = np.array([np.sin(0.5), 0.0, np.cos(0.5)])
    wh = np.array([-0.5 * 0.5, -0.5 * 0.5, 1.0])
    wh /= np.linalg.norm(wh)
    wi = -wo + 2 * np.dot(wo, wh) * wh
    n = 100_000
    expected = mm.pdf_bins(mat, wo).reshape(-1) * n
    counts = np.bincount(mm.bin_of(np.broadcast_to(wi, (n, 3))), minlength=expected.size)
    assert _chi2_p(counts, expected, (0, n - expected.sum())) < 1e-12


def test_albedo_quadrature_matches_monte_carlo():
    mat = mm.Material.plastic((0.3, 0.2, 0.1), (0.6, 0.6, 0.6), 0.2)
    wo = np.array([np.sin(0.7), 0.0, np.cos(0.7)])
    n = 400_000
    u = np.random.default_rng(3).random((n, 2))
    wi, f, pdf, ok, _ = mm.bsdf_sample_f(mat, np.broadcast_to(wo, (n, 3)).copy(), u)
    est = np.where(ok[:, None], f * np.abs(wi[:, 2:3]) / np.where(ok, pdf, 1)[:, None], 0.0)
    mean, se = est.mean(0), est.std(0) / np.sqrt(n)
    assert np.all(np.abs(mm.albedo(mat, wo) - mean) < 4 * se + 1e-9), (mm.albedo(mat, wo), mean, se)


def test_fresnel_limits():
    assert mm.fr_dielectric(np.array([1.0]), 1.0, 1.5)[0] == pytest.approx(0.04)
    # pbrt-v3's plastic: (eta_i, eta_t) = (1.5, 1): total internal reflection past sin theta = 2/3
    assert mm.fr_dielectric(np.array([0.7]), 1.5, 1.0)[0] == 1.0
    np.testing.assert_allclose(mm.fr_conductor(np.array([1.0]), [1.5, 1.5, 1.5], [0, 0, 0])[0], 0.04, rtol=1e-12)
    assert np.all(mm.fr_conductor(np.array([0.0]), [0.2, 1.0, 3.0], [3.0, 2.0, 0.0]) == pytest.approx(1.0))


# ---- the C ABI ----
def test_header_declares_plastic_and_metal():
    h = open(HEADER).read()
    assert re.search(r"PBRT_MAT_PLASTIC\s*=\s*4", h) and re.search(r"PBRT_MAT_METAL\s*=\s*5", h)
    assert re.search(r"int pbrt_hip_scene_set_material_roughness\(PbrtHipScene\* scene, int32_t material, float u_roughness, "
                     r"float v_roughness, int32_t remap\);", h)
    assert re.search(r"int pbrt_hip_bsdf_query\(PbrtHipScene\* scene, int32_t material, int64_t n,", h)
    assert scenes.MAT_PLASTIC == pbrt_hip.MAT_PLASTIC == 4 and scenes.MAT_METAL == pbrt_hip.MAT_METAL == 5
    assert scenes.plastic((1, 0, 0), (0, 1, 0)) == (4, (1, 0, 0), (0, 1, 0), 0.1)
    assert scenes.metal((1, 1, 1), (2, 2, 2)) == (5, (1, 1, 1), (2, 2, 2), 0.01)


def test_material_layout_unchanged(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrt_hip.h"\nint main(void) { printf("%d %d %d %d", '
                   '(int)sizeof(PbrtMaterial), (int)offsetof(PbrtMaterial, kt), (int)offsetof(PbrtMaterial, eta), '
                   'PBRT_MAT_METAL); return 0; }\n')
    exe = tmp_path / "m"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["32", "16", "28", "5"]
    assert scenes.MATERIAL_DTYPE.itemsize == 32


def test_library_exports_the_glossy_entry_points():
    L = ctypes.CDLL(pbrt_hip.LIB_PATH)
    for name in ("pbrt_hip_scene_set_material_roughness", "pbrt_hip_bsdf_query"):
        assert hasattr(L, name), name
        assert name in pbrt_hip.EXPORTS


def test_new_scene_builders_face_up():
    for sc in (scenes.glossy_plane_point_light_scene(scenes.plastic((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))),
               scenes.glossy_plane_env_scene(scenes.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.2)))):
        p = sc["positions"][sc["indices"]].astype(np.float64)
        n = np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 2])  # the device's geometric normal
        assert np.all(n[:, 2] > 0) and np.all(n[:, :2] == 0)
