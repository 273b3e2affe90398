"""The engine's workspace is laid out as the parent build laid it out (tests/golden/engine_layout_parent.json, recorded
with bench/record_engine_layout.py on a build of the parent commit of the change that made the workspace one table):
the total size and every named region's offset from X, for the default sliced engine, the multi-kernel engine at
batch 64 in fp32 with the debug regions, and a small sliced engine with them.  And the step plan of a created engine's
own configuration (csrc/engine_plan.h) agrees with what the engine reports about its fc workers.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))

from record_engine_layout import CASES, REGIONS, case_key, layout, make_engine  # noqa: E402  (the recorder's own cases)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_layout_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("bmax,dtype,debug,persistent", CASES)
def test_layout_and_plan_match_parent(gpu, golden, bmax, dtype, debug, persistent):
    want = golden[case_key(bmax, dtype, debug, persistent)]
    eng = make_engine(bmax, dtype, debug, persistent)
    try:
        got = layout(eng)
        print(case_key(bmax, dtype, debug, persistent), json.dumps(got))
        assert got["kind"] == want["kind"]
        assert got["workspace_bytes"] == want["workspace_bytes"]
        assert sorted(got["offsets"]) == sorted(REGIONS) == sorted(want["offsets"])
        assert got["offsets"] == want["offsets"]
        assert eng.lib.dca_engine_region(eng.h, b"NO_SUCH_REGION") is None
        for B in (1, 8, bmax):
            plan = eng.step_plan(B)
            assert bool(plan.fc) == eng.fc_in_step(B), B
            if eng.kind_name == "sliced":
                assert plan.step_grid == (B + 7) // 8 * 32 + (65 if plan.fc else 0)
            else:
                assert plan.fc == 0 and plan.step_grid == 0 and plan.nparts == 4 * B
    finally:
        eng.close()
