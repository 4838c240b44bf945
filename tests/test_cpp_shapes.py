"""include/pbrt_hip.hpp: TransformedSphere, Disk and Cylinder (the reference's constructor arguments in its order) compile as
strict C++17, stop at Context creation without a GPU, and on a GPU render the film the Python binding renders of the same
capped-cylinder scene, bit for bit (examples/render_capped_cylinder.cpp)."""
import re
import subprocess

import numpy as np
import pytest

import pbrt_hip
from pbrt_hip import scenes
from test_cpp_example import _build, _open_box


def test_cpp_shapes_compile_and_refuse_to_run_without_a_gpu(tmp_path):
    import torch
    exe = _build(tmp_path, "render_capped_cylinder.cpp")
    hpp = open(pbrt_hip.LIB_PATH.replace("pbrt-rs_amd/pbrt_hip/libpbrt_hip.so", "include/pbrt_hip.hpp")).read()
    for name in ("struct Disk : Shape", "struct Cylinder : Shape", "struct TransformedSphere : Shape", "src/shapes/disk.rs:24-40",
                 "src/shapes/cylinder.rs:23-39", "const std::vector<Shape>& shapes", "const std::vector<Sphere>& spheres"):
        assert name in hpp, name
    if torch.cuda.is_available():
        pytest.skip("a GPU is present (covered by the gpu test)")
    r = subprocess.run([exe, str(tmp_path / "film.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "pbrt::Error (3)" in r.stderr and "no CPU fallback" in r.stderr
    assert not (tmp_path / "film.raw").exists()


@pytest.mark.gpu
def test_cpp_shapes_render_what_the_python_binding_renders(tmp_path, hip_ctx):
    W, H = 64, 48
    raw = tmp_path / "film.raw"
    r = subprocess.run([_build(tmp_path, "render_capped_cylinder.cpp"), str(raw), str(W), str(H)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"capped cylinder: (\d+) camera samples, (\d+) closest-hit \+ (\d+) shadow rays; film xyz (\S+); world bound y \[-1\.00, 1\.00\]", r.stdout)
    assert m and int(m.group(1)) == W * H * 16, r.stdout
    assert re.search(r"top cap: hit 1 t 0\.6000 primitive 13", r.stdout), r.stdout  # y = 0.5 down to -1 + 0.9; 12 triangles, the cylinder, then the cap
    upright = np.array([[1, 0, 0, -0.35], [0, 0, 1, -1], [0, -1, 0, 0.2], [0, 0, 0, 1]], dtype=np.float64)
    squash = np.array([[1, 0, 0, 0.45], [0, 0.5, 0, -0.8], [0, 0, 1, -0.1], [0, 0, 0, 1]], dtype=np.float64)
    sc = dict(_open_box(), shapes=scenes.shapes(scenes.cylinder(0.3, 0.0, 0.9, 270.0, upright, material=1), scenes.disk(0.9, 0.3, 0.0, 270.0, upright, material=2),
                                                scenes.disk(0.0, 0.3, 0.0, 270.0, upright, material=2, reverse_orientation=True),
                                                scenes.sphere_shape(0.4, -0.4, 0.4, 360.0, squash, material=0)))
    g = pbrt_hip.Scene(hip_ctx, sc)
    film, st = g.render(scenes.perspective_camera((0.0, 0.0, -3.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, W, H), W, H, 16, max_depth=5, seed=21, light_strategy=2)  # PathIntegrator::new's default: "spatial"
    g.close()
    assert (st["camera_samples"], st["rays_closest"], st["rays_shadow"]) == tuple(int(m.group(k)) for k in (1, 2, 3))
    assert film[..., :3].mean() > 0.01
    assert raw.read_bytes() == film.tobytes()
