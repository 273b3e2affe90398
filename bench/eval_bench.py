"""Evaluation throughput of NetResDeep on one device: the fused eval kernel (bf16 and fp32) against the two ways the
model could be evaluated on the GPU without it -- ``OpsModel(net).eval()`` (the ops-layer HIP kernels) and stock
torch eager fp32 ``model.eval()``, both at batch 1000.

Every variant evaluates the same 10,000 synthetic images with the same fixed model state, in one process; the
variants are interleaved (one evaluation of each per round), each whole evaluation -- index upload, kernels, the
reduction of the per-image results and the read-back -- sits between two HIP events.  Prints one JSON line with the
median and the min - max spread per variant; ``rule_met`` says whether the bf16 kernel's median is below both
non-fused medians by more than the larger of their spreads.

    python bench/eval_bench.py [--images 10000] [--warmup 5] [--reps 20] | tee profiles/eval_bench.log
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar  # noqa: E402
from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep  # noqa: E402
from distributeddataparallel_cifar10_amd.ops.models import OpsModel  # noqa: E402
from distributeddataparallel_cifar10_amd.runtime.evaluate import evaluate_module, evaluate_netresdeep  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1000, help="batch of the two non-fused variants")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    data, labels = synthetic_cifar(a.images, seed=1, learnable="hard")
    data, labels = data.to(dev), labels.to(dev)
    torch.manual_seed(0)
    net = NetResDeep().to(dev)
    bn = net.resblocks[0].batch_norm
    with torch.no_grad():  # running statistics away from their initial values; the state stays fixed from here on
        bn.running_mean.normal_(0.0, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    ops = OpsModel(net)
    variants = {
        "fused_bf16": lambda: evaluate_netresdeep(net, data, labels, dtype="bf16"),
        "fused_fp32": lambda: evaluate_netresdeep(net, data, labels, dtype="fp32"),
        "ops_eval_b1000": lambda: evaluate_module(ops, data, labels, batch=a.batch),
        "torch_eager_fp32_b1000": lambda: evaluate_module(net, data, labels, batch=a.batch),
    }
    times = {k: [] for k in variants}
    acc = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
            acc[name] = res.accuracy
    out = {"bench": "eval", "images": a.images, "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                     "images_per_sec": round(a.images / med * 1e3, 1), "accuracy": round(acc[name], 4)}
    spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("ops_eval_b1000", "torch_eager_fp32_b1000"))
    out["rule_met"] = all(out["fused_bf16"]["median_ms"] + spread < out[k]["median_ms"]
                          for k in ("ops_eval_b1000", "torch_eager_fp32_b1000"))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
