"""Record (or print) the bitwise trajectory fingerprints of the sliced persistent engine (GPU).

For every case (dtype, batch) of ``CASES`` run ``engine_diag.trajectory(dtype, 4, B, 3, persistent=True)`` and keep
the SHA-256 of the final parameter vector's bytes and the three step losses.  ``tests/test_pks_lds_plan_gpu.py``
compares the build under test with ``tests/golden/pks_trajectory_parent.json``; that file is written by running this
script on a build of the PARENT commit of a change that must not alter results, never on the changed code:

    python bench/record_pks_trajectory.py --out tests/golden/pks_trajectory_parent.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [("bf16", 3), ("bf16", 9), ("bf16", 32), ("fp32", 3), ("fp32", 32)]
STEPS = 3


def case_key(dtype: str, B: int) -> str:
    return f"{dtype}/B{B}"


def fingerprint(dtype: str, B: int):
    """(record, final parameter tensor) of one case"""
    import engine_diag
    r = engine_diag.trajectory(dtype, 4, B, STEPS, persistent=True)
    params = r["params"].contiguous()
    sha = hashlib.sha256(params.numpy().tobytes()).hexdigest()
    return {"params_sha256": sha, "losses": [float(x) for x in r["losses_engine"]]}, params


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the fixture here (default: print only)")
    a = ap.parse_args()
    rec = {}
    for dtype, B in CASES:
        rec[case_key(dtype, B)], _ = fingerprint(dtype, B)
        print(case_key(dtype, B), json.dumps(rec[case_key(dtype, B)]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"steps": STEPS, "rows": 4, "cases": rec}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
