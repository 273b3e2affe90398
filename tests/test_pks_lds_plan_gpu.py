"""The step kernel's LDS plan and tail order change no result: three-step trajectories of the sliced persistent engine
are bitwise those of the parent build (tests/golden/pks_trajectory_parent.json, recorded with
bench/record_pks_trajectory.py on a build of the parent commit), and bf16 runs repeat bitwise.

Cases: batch 3 (workgroups of a group of 8 that exit at once, top and bottom edge slices), 9 (a second, nearly empty
group), 32 (the benchmark's size); three steps cover both staging parities and a staged batch that is consumed.
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pks_trajectory_parent.json")
CASES = [("bf16", 3), ("bf16", 9), ("bf16", 32), ("fp32", 3), ("fp32", 32)]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("dtype,B", CASES)
def test_trajectory_bitwise_parent(gpu, golden, dtype, B):
    from record_pks_trajectory import case_key, fingerprint
    want = golden[case_key(dtype, B)]
    got, params = fingerprint(dtype, B)
    print(case_key(dtype, B), json.dumps(got))
    assert got["losses"] == want["losses"]
    assert got["params_sha256"] == want["params_sha256"]
    if dtype == "bf16":  # run to run
        got2, params2 = fingerprint(dtype, B)
        assert torch.equal(params, params2)
        assert got2["losses"] == got["losses"]
