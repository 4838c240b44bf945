"""The render's host half (pbrt-rs_amd/csrc/host_render.cpp), no GPU.

pbrt_hip_render, pbrt_hip_li and pbrt_hip_camera_rays plan the call on the host (plan_render: the normalised parameters and the
refusals in the order they have always been reported, the tile set, the pass size, the sort switches, the sampler's table
layout, the HaltonSampler's constants) and RenderJob (render.hip) then takes device blocks in the sizes the plan states.
tests/native/render_plan_check.cpp runs the plan on the GPU tests' refusal inputs and compares the messages, and checks what it
computes: a stand-alone program under AddressSanitizer and UBSan, as tests/test_scene_edit_host.py runs the scene setters' host
half.
"""
import os
import re
import subprocess

import pytest

from test_scene_plan_host import BUILD, CSRC, FLAGS, HERE, HIPCC

SRC = os.path.join(HERE, "native", "render_plan_check.cpp")
PLAN_FILES = ("host_render.cpp", "host_film.cpp")   # the plan, and the sample bounds and the tile partition it calls


@pytest.fixture(scope="module")
def built():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "render_plan_check")
    srcs = [os.path.join(CSRC, f) for f in PLAN_FILES] + [SRC]
    objs = [os.path.join(BUILD, "render_plan_" + os.path.basename(s).rsplit(".", 1)[0] + ".o") for s in srcs]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not all(os.path.exists(p) for p in [exe] + objs) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tag = f".{os.getpid()}"   # renamed when complete: parallel test workers never run a half-written program
        jobs = [subprocess.Popen([HIPCC] + FLAGS + ["-c", "-o", o + tag, s]) for s, o in zip(srcs, objs)]   # side by side
        assert [j.wait() for j in jobs] == [0] * len(jobs)
        for o in objs:
            os.replace(o + tag, o)
        subprocess.check_call([HIPCC, "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-o", exe + tag] + objs)
        os.replace(exe + tag, exe)
    return exe, objs[0]


def test_render_plans_and_refusals_under_sanitizers(built):
    exe, _ = built
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 failures"), r.stdout[-2000:]


def test_host_render_makes_no_device_call(built):
    """host_render.cpp is the part of a render a CPU can run: its object refers to no HIP runtime function."""
    _, obj = built
    undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.split("\n")
    names = [line.split()[-1] for line in undefined if line.strip()]
    assert names, "nm listed nothing"
    assert not [n for n in names if re.match(r"_*hip[A-Z_]", n)], names
