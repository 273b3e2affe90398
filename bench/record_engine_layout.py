"""Record (or print) the engine's workspace layout (GPU): total bytes and every named region's offset from ``X``.

``tests/test_engine_layout_gpu.py`` compares the build under test with ``tests/golden/engine_layout_parent.json``; that
file is written by running this script on a build of the PARENT commit of a change that must not move a region, never
on the changed code:

    python bench/record_engine_layout.py --commit <parent sha> --out tests/golden/engine_layout_parent.json

Cases (batch_max, dtype, debug, persistent): the default sliced engine; the multi-kernel engine at batch 64 in fp32
with the debug regions; a small sliced engine with the debug regions.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(32, "bf16", False, None), (64, "fp32", True, False), (8, "bf16", True, None)]
REGIONS = ["X", "Y", "DY", "G", "SCODE", "FPART", "STATS", "BPART", "WSLAB", "SSLAB", "HP", "HH", "HDH", "HDL", "HLOSS",
           "HPART", "HCODE", "WT_F", "WT_D", "SW", "RS_BASE", "CURSOR", "STEPS", "LOSS", "STAMPS", "EPOCH", "ERR",
           "TSLAB", "BNG", "W1B", "SIMG", "SLAB", "COMMT", "PKW", "PKS_GRAN", "PKS_YH", "PKS_BNX", "PKS_HDONE", "C1"]


def case_key(bmax: int, dtype: str, debug: bool, persistent) -> str:
    return f"B{bmax}/{dtype}/debug{int(debug)}/{'auto' if persistent is None else int(persistent)}"


def make_engine(bmax: int, dtype: str, debug: bool, persistent):
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine

    dev = torch.device("cuda", 0)
    data = torch.zeros(bmax, 3, 32, 32, dtype=torch.uint8, device=dev)
    labels = torch.zeros(bmax, dtype=torch.int64, device=dev)
    return NetResDeepEngine(NetResDeep().to(dev), data, labels, EngineConfig(
        batch_max=bmax, dtype=dtype, debug=debug, persistent=persistent))


def layout(eng) -> dict:
    ptr = {n: eng.lib.dca_engine_region(eng.h, n.encode()) for n in REGIONS}
    assert all(ptr.values()), [n for n, p in ptr.items() if not p]
    return {"kind": eng.kind_name, "workspace_bytes": eng.workspace_bytes(),
            "offsets": {n: ptr[n] - ptr["X"] for n in REGIONS}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the fixture here (default: print only)")
    ap.add_argument("--commit", default="unknown", help="the commit the recorded build was made from")
    a = ap.parse_args()
    rec = {}
    for case in CASES:
        eng = make_engine(*case)
        try:
            rec[case_key(*case)] = layout(eng)
        finally:
            eng.close()
        print(case_key(*case), json.dumps(rec[case_key(*case)]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"recorded_on_commit": a.commit, "cases": rec}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
