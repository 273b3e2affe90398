"""Record (or print) bitwise fingerprints of the sliced persistent engine for the kernel-entry cases (GPU).

Every case runs 5 single steps through ``set_indices`` / ``set_cursor`` / ``run`` on an index list of exactly
``4 * B + 1`` entries, so the fifth batch and the prefetches of the fourth and fifth step read past the list's end
(``sample_id``'s end clamp), and both staging parities are consumed.  Kept per case: the five step losses and the
SHA-256 of the final state (every parameter and BatchNorm buffer).  ``tests/test_pks_entry_gpu.py`` compares the build
under test with ``tests/golden/pks_entry_parent.json``; that file is written by running this script on a build of the
PARENT commit of a change that must not alter results, never on the changed code:

    python bench/record_pks_entry.py --out tests/golden/pks_entry_parent.json

Cases (dtype, batch, kind):
  plain    5 steps from cursor 0
  cursor   the same with ``set_cursor`` moved between steps 2 and 3 (``k_pks_prime``, then a staged batch)
  full     batch 64 on every CU: 256 gradient slabs, i.e. two 128-slab passes of the reduction's slab sum, and the fc
           segments on the reduction kernel
  coarse   ``set_shared_device(2)`` at world size 1: the 256-element segment layout of a shared device
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 5
CASES = [("bf16", 3, "plain"), ("bf16", 32, "plain"), ("fp32", 3, "plain"), ("fp32", 32, "plain"),
         ("bf16", 32, "cursor"), ("fp32", 32, "cursor"), ("bf16", 64, "full"), ("bf16", 16, "coarse")]


def case_key(dtype: str, B: int, kind: str) -> str:
    return f"{dtype}/B{B}/{kind}"


def fingerprint(dtype: str, B: int, kind: str, seed: int = 3) -> dict:
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine

    n = 4 * B + 1
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int64, generator=g)
    order = torch.randperm(n, generator=g).numpy().astype(np.int32)
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    model = NetResDeep().to(dev)
    eng = NetResDeepEngine(model, data.to(dev), labels.to(dev), EngineConfig(
        batch_max=B, lr=1e-2, dtype=dtype, persistent=True, full_device=(kind == "full")))
    try:
        if kind == "coarse":
            eng.set_shared_device(2)
        eng.set_indices(order)
        eng.set_cursor(0)
        eng.read_loss(reset=True)
        losses = []
        for s in range(STEPS):
            if kind == "cursor" and s == 2:
                eng.set_cursor(B + 5)
            eng.run(B, 1)
            lsum, _ = eng.read_loss(reset=True)
            losses.append(float(lsum))
        eng.check_errors()
        h = hashlib.sha256()
        sd = model.state_dict()
        for k in sorted(sd):
            h.update(k.encode())
            h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    finally:
        eng.close()
    return {"state_sha256": h.hexdigest(), "losses": losses}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the fixture here (default: print only)")
    a = ap.parse_args()
    rec = {}
    for dtype, B, kind in CASES:
        key = case_key(dtype, B, kind)
        try:
            rec[key] = fingerprint(dtype, B, kind)
        except Exception as exc:  # a case the recorded build cannot run is left out of the fixture (and said so)
            print(key, "NOT RECORDED:", repr(exc), flush=True)
            continue
        print(key, json.dumps(rec[key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"steps": STEPS, "cases": rec}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
