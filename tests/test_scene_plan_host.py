"""Scene creation's host phases (pbrt-rs_amd/csrc/host_scene.cpp), no GPU.

Every pbrt_hip_scene_create* entry point checks its description (scene_invalid), lays every table out in host arrays
(plan_scene, plan_two_level_wide) and only then touches the device. The first two phases turn caller-supplied indices into
array subscripts; tests/native/scene_plan_check.cpp runs them on tiny scenes of every kind (triangles, spheres, shapes, two
levels, moving instances) as a stand-alone program under AddressSanitizer and UBSan, checks invariants of the plan, and feeds
the bad inputs of the GPU tests' refusal cases and compares the messages.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbrt-rs_amd", "csrc")
SRC = os.path.join(HERE, "native", "scene_plan_check.cpp")
BUILD = os.path.join(HERE, "native", "_build")
HOST_FILES = ("host_scene.cpp", "host_bvh.cpp", "host_wide.cpp", "host_lobes.cpp", "host_envmap.cpp", "host_motion.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
# the host half only: the headers these files share with the kernels need the HIP front end, the device half is not built
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "--cuda-host-only",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def built():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "scene_plan_check")
    srcs = [os.path.join(CSRC, f) for f in HOST_FILES] + [SRC]
    objs = [os.path.join(BUILD, "scene_plan_" + os.path.basename(s).rsplit(".", 1)[0] + ".o") for s in srcs]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not all(os.path.exists(p) for p in [exe] + objs) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tag = f".{os.getpid()}"   # renamed when complete: parallel test workers never run a half-written program
        jobs = [subprocess.Popen([HIPCC] + FLAGS + ["-c", "-o", o + tag, s]) for s, o in zip(srcs, objs)]   # side by side
        assert [j.wait() for j in jobs] == [0] * len(jobs)
        for o in objs:
            os.replace(o + tag, o)
        # host objects only; the sanitizers' runtimes are the host's here as well
        subprocess.check_call([HIPCC, "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-o", exe + tag] + objs)
        os.replace(exe + tag, exe)
    return exe, objs[0]


def test_scene_plans_and_refusals_under_sanitizers(built):
    exe, _ = built
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 failures"), r.stdout[-2000:]


def test_host_scene_makes_no_device_call(built):
    """host_scene.cpp is the part of scene creation a CPU can run: its object refers to no HIP runtime function."""
    _, obj = built
    undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.split("\n")
    names = [line.split()[-1] for line in undefined if line.strip()]
    assert names, "nm listed nothing"
    assert not [n for n in names if re.match(r"_*hip[A-Z_]", n)], names
