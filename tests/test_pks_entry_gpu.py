"""The step kernel's entry (every load issued before its one wait, both staging parities read, the index of the next
batch fetched after the staging wait) and the reduction's slab sum (all loads of a 128-slab pass in flight, branch-free
adds) change no result: five-step runs of the sliced persistent engine are bitwise those of the parent build
(tests/golden/pks_entry_parent.json, recorded with bench/record_pks_entry.py on a build of the parent commit).

Cases (bench/record_pks_entry.py): an index list of exactly 4 B + 1 entries, so the last prefetches hit the end clamp
of the index list and both staging parities are used; the same with the cursor moved between steps 2 and 3
(k_pks_prime, then a staged batch); batch 64 on the full device (256 slabs: two passes of the slab sum, fc segments on
the reduction kernel); the coarse 256-element segment layout at world size 1.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))

from record_pks_entry import CASES, case_key, fingerprint  # noqa: E402  (the recorder's own case list)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "pks_entry_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("dtype,B,kind", CASES)
def test_entry_bitwise_parent(gpu, golden, dtype, B, kind):
    want = golden[case_key(dtype, B, kind)]
    got = fingerprint(dtype, B, kind)
    print(case_key(dtype, B, kind), json.dumps(got))
    assert got["losses"] == want["losses"]
    assert got["state_sha256"] == want["state_sha256"]
