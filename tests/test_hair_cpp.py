"""The hair row's C++ side compiles on a machine without a GPU: the example against include/pbrt_hip.hpp under -pedantic -Werror,
and hair_kernels.hip for gfx950 with the library's own flags."""
import os
import re
import subprocess

from test_cpp_example import ROOT, _build

CSRC = os.path.join(ROOT, "pbrt-rs_amd", "csrc")


def test_hair_strands_example_compiles(tmp_path):
    exe = _build(tmp_path, "render_hair_strands.cpp")
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "pbrt_hip.hpp")).read()
    for name in ("inline PbrtHairDesc hair(", "void set_hair_material(int32_t material, const PbrtHairDesc& desc)"):
        assert name in hpp, name


def test_hair_kernels_cross_compile_for_gfx950(tmp_path):
    """with the flags of build.sh (read from it), device code included; the unit is the only one that names a hair instantiation"""
    flags = re.search(r'^FLAGS="([^"]+)"', open(os.path.join(ROOT, "pbrt-rs_amd", "build.sh")).read(), re.M).group(1).split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags
    obj = tmp_path / "hair_kernels.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-Werror", "-c", "-o", str(obj), "hair_kernels.hip"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert obj.stat().st_size > 0
    for unit in ("render.hip", "curve_kernels.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "k_shade_hair" not in text and "kDirectHair" not in text and "wf_hair.h" not in text, unit
    assert "wf_hair.h" not in open(os.path.join(CSRC, "wavefront.h")).read()
