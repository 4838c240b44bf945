"""Host-side checks of the ray queue's one-entry-per-path sort (pbrt-rs_amd/csrc/wf_ray_expand.h), no GPU.

k_shade leaves one sort value per path, rec << 4 | cont | mis << 1 | shadow << 2 | mis_bool << 3, and the expansion kernels
turn the sorted values into the trace queue: every closest-hit token (continuation rays, non-boolean MIS rays) in list
order, then every any-hit token (boolean MIS rays, shadow rays) in list order. tests/native/path_sort_check.cpp compiles
the packing and the section arithmetic (the very functions the kernels call) for the host; the GPU tests
(test_gpu_path_sort.py) then check the kernels end to end.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "path_sort_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "libpath_sort_check.so")

CONT, MIS, SHADOW, MIS_BOOL = 0, 1, 2, 3  # the `what` of a trace-queue token (wf_state.h: RaySlot, RS_MIS_BOOL)


@pytest.fixture(scope="module")
def chk():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(HERE, "..", "pbrt-rs_amd", "csrc", "wf_ray_expand.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        # built under a name of its own, then renamed: parallel test workers never load a half-written library
        tmp = f"{OUT}.{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", tmp, SRC])
        os.replace(tmp, OUT)
    L = ctypes.CDLL(OUT)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    L.path_sort_roundtrip.argtypes = [u32]
    L.path_sort_pack.argtypes = [u32] + [ctypes.c_int] * 4
    L.path_sort_pack.restype = u32
    for f in (L.path_sort_expand, L.path_sort_expand_tiled):
        f.argtypes = [vp, u32, vp, vp]
        f.restype = u32
    return L


def test_packing_round_trips_at_both_ends_of_the_record_range(chk):
    assert chk.path_sort_rec_bits() == 28
    for rec in (0, 1, 12345, 2**28 - 1):
        assert chk.path_sort_roundtrip(rec) == 0, rec
    # the layout the design states
    assert chk.path_sort_pack(5, 1, 0, 0, 0) == 5 << 4 | 1
    assert chk.path_sort_pack(5, 0, 1, 0, 0) == 5 << 4 | 2
    assert chk.path_sort_pack(5, 0, 0, 1, 0) == 5 << 4 | 4
    assert chk.path_sort_pack(5, 0, 1, 0, 1) == 5 << 4 | 10
    assert chk.path_sort_pack(2**28 - 1, 1, 1, 1, 1) == 2**32 - 1


def _entries(rng, n):
    """n path entries in a shuffled record order (what a sort leaves), each with a flag set k_shade can produce: at least
    one ray, mis_bool only with mis."""
    flags = rng.choice(np.array([f for f in range(1, 16) if not (f & 8 and not f & 2)], dtype=np.uint32), size=n)
    rec = rng.permutation(n).astype(np.uint32)
    return (rec << np.uint32(4)) | flags, rec, flags


def _expected(rec, flags):
    """(closest tokens, any-hit tokens) in list order, restated with numpy."""
    cont, mis, shadow, mb = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
    closest, anyhit = [], []
    for r, c, m, s, b in zip(rec.tolist(), cont.tolist(), mis.tolist(), shadow.tolist(), mb.tolist()):
        if c:
            closest.append(r * 4 + CONT)
        if m and not b:
            closest.append(r * 4 + MIS)
        if m and b:
            anyhit.append(r * 4 + MIS_BOOL)
        if s:
            anyhit.append(r * 4 + SHADOW)
    return np.array(closest, dtype=np.uint32), np.array(anyhit, dtype=np.uint32)


@pytest.mark.parametrize("n", [1, 3, 255, 1024, 1025, 4096 + 77, 50_001])
@pytest.mark.parametrize("which", ["path_sort_expand", "path_sort_expand_tiled"])
def test_expansion_yields_every_ray_once_closest_hit_first(chk, which, n):
    rng = np.random.default_rng(1000 + n)
    entries, rec, flags = _entries(rng, n)
    tokens = np.full(3 * n, 0xFFFFFFFF, dtype=np.uint32)
    n_closest = ctypes.c_uint32(0)
    total = getattr(chk, which)(entries.ctypes.data, n, tokens.ctypes.data, ctypes.byref(n_closest))
    closest, anyhit = _expected(rec, flags)
    assert n_closest.value == len(closest) and total == len(closest) + len(anyhit)
    assert (tokens[total:] == 0xFFFFFFFF).all()
    out = tokens[:total]
    # the sections, each in list order
    assert np.array_equal(out[:n_closest.value], closest)
    assert np.array_equal(out[n_closest.value:], anyhit)
    # every (rec, slot) the flags ask for exactly once; a token's slot decides its section
    assert len(np.unique(out)) == total
    want = set()
    for r, f in zip(rec.tolist(), flags.tolist()):
        if f & 1:
            want.add((r, CONT))
        if f & 2:
            want.add((r, MIS_BOOL if f & 8 else MIS))
        if f & 4:
            want.add((r, SHADOW))
    assert {(int(t) >> 2, int(t) & 3) for t in out} == want
    assert np.isin(out[:n_closest.value] & 3, [CONT, MIS]).all()
    assert np.isin(out[n_closest.value:] & 3, [MIS_BOOL, SHADOW]).all()


def test_entries_without_rays_add_nothing(chk):
    """Flag sets with no ray (0, or mis_bool alone) are never written by k_shade; the arithmetic still gives them no token."""
    entries = np.array([7 << 4, 9 << 4 | 8, 3 << 4 | 1], dtype=np.uint32)
    tokens = np.zeros(9, dtype=np.uint32)
    n_closest = ctypes.c_uint32(0)
    for which in ("path_sort_expand", "path_sort_expand_tiled"):
        total = getattr(chk, which)(entries.ctypes.data, 3, tokens.ctypes.data, ctypes.byref(n_closest))
        assert (total, n_closest.value, int(tokens[0])) == (1, 1, 3 * 4 + CONT)
