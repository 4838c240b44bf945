"""Every launch path the host driver can select, held bit for bit to what the library computed before kernel selection moved into
csrc/kernel_select.h: tests/golden/dispatch_matrix.json, recorded by tests/golden/make_dispatch_matrix.py (whose case list and
runner this file imports, so the two cannot drift). Shading: six scene feature sets x path / direct (both strategies) / Whitted / AO,
the three shade orders, the three builds of the spatial light table, two passes. Traversal: stackless, wide + follow-up, shapes,
spheres, binary for INST 0 / 1 / 2, each with the counting instantiations, through render, intersect and intersect_p. One render
large enough for the ray-queue sort. Films do not depend on which lane runs a path (wf_path.h), so the hashes are exact."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_dispatch_matrix as dm  # noqa: E402

pytestmark = pytest.mark.gpu

with open(dm.FIXTURE) as _fh:
    GOLDEN = json.load(_fh)
CASES = dm.cases()


def test_the_fixture_covers_the_case_list():
    ids = {c["id"] for c in CASES}
    assert set(GOLDEN["cases"]) | set(GOLDEN["excluded"]) == ids and not set(GOLDEN["cases"]) & set(GOLDEN["excluded"])
    assert len(GOLDEN["excluded"]) * 20 <= len(CASES)  # at most 5 %
    for f in dm.FEATURES:
        for integ in dm.INTEGRATORS:
            assert any(c["kind"] == "shade" and c["feature"] == f and c["integrator"] == integ and c["id"] in GOLDEN["cases"] for c in CASES), (f, integ)


@pytest.fixture(scope="module")
def scene_cache(hip_ctx):
    cache = dm.SceneCache(hip_ctx)
    yield cache
    cache.close()


@pytest.mark.parametrize("case", [c for c in CASES if c["id"] in GOLDEN["cases"]], ids=lambda c: c["id"])
def test_case_equals_the_recorded_run(hip_ctx, scene_cache, case):
    want = GOLDEN["cases"][case["id"]]
    try:
        got = dm.run_case(hip_ctx, scene_cache, case)
    finally:
        hip_ctx.set_traversal(dm.AUTO)
        hip_ctx.set_counting(0)
    if case["kind"] == "trace":
        if case["wide"]:
            assert got["wide_records"], "the case is meant to run the wide kernels: the scene must have wide records"
        if case["counting"] == 1 or (case["counting"] == 2 and case["wide"]):  # the only outside sign that the COUNT build ran
            for stage in ("render_counters", "intersect_counters", "intersect_p_counters"):
                assert got[stage] and all(v > 0 for v in got[stage].values()), (stage, got[stage])
    if case["kind"] == "raysort":
        assert got["ray_order0"] == got["ray_order1"]
    assert got == want
