"""The scene setters' host half (pbrt-rs_amd/csrc/host_edit.cpp) and the two-level scenes' combined mesh (host_scene.cpp), no GPU.

Every pbrt_hip_scene_set_* entry point has a host function check its descriptor against the scene's host tables and compute
the bytes the edit writes, and applies them through apply_writes (host_edit.h), which puts the previous bytes back when a write
fails. tests/native/scene_edit_check.cpp runs the host functions on the GPU tests' refusal inputs and compares the messages,
checks what they compute, and drives apply_writes over memcpy with a writer that fails at the k-th call: a stand-alone program
under AddressSanitizer and UBSan, as tests/test_scene_plan_host.py runs scene creation's host phases.
"""
import os
import re
import subprocess

import pytest

from test_scene_plan_host import BUILD, CSRC, FLAGS, HERE, HIPCC, HOST_FILES

SRC = os.path.join(HERE, "native", "scene_edit_check.cpp")
EDIT_FILES = ("host_edit.cpp",) + HOST_FILES
PURE = ("host_edit", "host_scene", "host_lobes", "host_envmap")   # the objects that hold what an edit or a creation computes


@pytest.fixture(scope="module")
def built():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "scene_edit_check")
    srcs = [os.path.join(CSRC, f) for f in EDIT_FILES] + [SRC]
    objs = [os.path.join(BUILD, "scene_edit_" + os.path.basename(s).rsplit(".", 1)[0] + ".o") for s in srcs]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not all(os.path.exists(p) for p in [exe] + objs) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tag = f".{os.getpid()}"   # renamed when complete: parallel test workers never run a half-written program
        jobs = [subprocess.Popen([HIPCC] + FLAGS + ["-c", "-o", o + tag, s]) for s, o in zip(srcs, objs)]   # side by side
        assert [j.wait() for j in jobs] == [0] * len(jobs)
        for o in objs:
            os.replace(o + tag, o)
        subprocess.check_call([HIPCC, "-pthread", "-Xarch_host", "-fsanitize=address,undefined", "-o", exe + tag] + objs)
        os.replace(exe + tag, exe)
    return exe, [o for o in objs if os.path.basename(o)[len("scene_edit_"):-2] in PURE]


def test_scene_edits_and_refusals_under_sanitizers(built):
    exe, _ = built
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 failures"), r.stdout[-2000:]


def test_host_edit_makes_no_device_call(built):
    """What an edit computes and what scene creation lays out is what a CPU can run: no object that holds it refers to a HIP
    runtime function."""
    _, objs = built
    assert len(objs) == len(PURE)
    for obj in objs:
        undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.split("\n")
        names = [line.split()[-1] for line in undefined if line.strip()]
        assert names, "nm listed nothing"
        assert not [n for n in names if re.match(r"_*hip[A-Z_]", n)], (obj, names)
