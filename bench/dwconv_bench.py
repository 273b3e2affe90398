"""The depthwise 3x3 kernels (csrc/ops_dwconv.hip) against torch's ``conv2d(groups=C)`` (channels_last bf16) on one
device, at the nine distinct depthwise shapes of MobileNetV1 (batch 256, input 224).

1. Per shape: forward, input gradient and weight gradient, each alternated with torch's on the same tensors (one of
   each per repetition) between two HIP events; median and min - max, and the bytes/s of the ops kernel counting x read
   once and y written once (compare with ``bench/micro/bw_micro.hip``'s 1:1 read : write ceiling and, at equal tensor
   sizes, with the grouped kernels in ``profiles/gconv_bench.log``).
2. One whole ``MobileNetV1`` training step (forward, loss, backward, SGD), ``OpsModel`` against stock PyTorch
   (channels_last, bf16 autocast), alternated.

    python bench/dwconv_bench.py [--batch 256] [--reps 30] [--step-reps 10] | tee profiles/dwconv_bench.log
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributeddataparallel_cifar10_amd.ops import functional as F  # noqa: E402

#          C,   H (= W), stride
SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1),
          (512, 14, 2), (1024, 7, 1)]
SIDES = ("ops", "torch")


def _stats(ts, unit="us", scale=1e3, digits=1):
    return {f"median_{unit}": round(statistics.median(ts) * scale, digits),
            f"min_{unit}": round(min(ts) * scale, digits), f"max_{unit}": round(max(ts) * scale, digits)}


def _alternate(fns, warmup, reps):
    """Milliseconds of each of `fns` (name -> callable), one of each per repetition, between two HIP events."""
    times = {k: [] for k in fns}
    for rep in range(warmup + reps):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= warmup:
                times[name].append(t0.elapsed_time(t1))
    return times


def shape_bench(batch, c, hw, stride, warmup, reps, dev):
    g = torch.Generator().manual_seed(c + hw)
    ho = (hw - 1) // stride + 1
    x = torch.randn(batch, hw, hw, c, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn(batch, ho, ho, c, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(c, 1, 3, 3, generator=g) * 0.3).to(dev)
    wb = w.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # the same memory as channels_last NCHW
    conv = dict(stride=stride, padding=1, groups=c)
    pairs = {
        "fwd": (lambda: F.dwconv_fwd(x, w, stride), lambda: TF.conv2d(xt, wb, **conv)),
        "dgrad": (lambda: F.dwconv_dgrad(dy, x.shape, w, stride),
                  lambda: torch.nn.grad.conv2d_input(xt.shape, wb, dyt, **conv)),
        "wgrad": (lambda: F.dwconv_wgrad(x, dy, stride),
                  lambda: torch.nn.grad.conv2d_weight(xt, wb.shape, dyt, **conv)),
    }
    rel = {}  # agreement of the two sides (bf16 rounding of the outputs only)
    for k, (a, b) in pairs.items():
        o, t = a().float(), b().float()
        t = t.permute(0, 2, 3, 1) if k != "wgrad" else t
        rel[k] = round(((o - t).norm() / t.norm()).item(), 5)
    nbytes = (x.numel() + dy.numel()) * 2
    for k, (a, b) in pairs.items():
        times = _alternate({"ops": a, "torch": b}, warmup, reps)
        out = {"bench": "dwconv", "pass": k, "batch": batch, "C": c, "HW": hw, "stride": stride, "reps": reps,
               "ops_vs_torch_rel_l2": rel[k]}
        out.update({s: _stats(times[s]) for s in SIDES})
        out["ops_GBps"] = round(nbytes / (statistics.median(times["ops"]) * 1e-3) / 1e9, 1)
        print(json.dumps(out), flush=True)


def step_bench(batch, warmup, reps, dev):
    from distributeddataparallel_cifar10_amd.models.mobilenet import MobileNetV1
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    torch.manual_seed(0)
    nets = {"ops": MobileNetV1().to(dev), "torch": MobileNetV1().to(dev).to(memory_format=torch.channels_last)}
    run = {"ops": OpsModel(nets["ops"]), "torch": nets["torch"]}
    opts = {s: torch.optim.SGD(nets[s].parameters(), lr=1e-3, momentum=0.9) for s in SIDES}
    x = torch.randn(batch, 3, 224, 224, device=dev)
    xc = x.contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (batch,), device=dev)

    def step(side):
        opts[side].zero_grad(set_to_none=True)
        if side == "ops":
            loss = cross_entropy(run[side](x), y)
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = TF.cross_entropy(run[side](xc), y)
        loss.backward()
        opts[side].step()

    times = _alternate({s: (lambda s=s: step(s)) for s in SIDES}, warmup, reps)
    out = {"bench": "mobilenet_v1_train_step", "batch": batch, "reps": reps}
    out.update({s: _stats(times[s], "ms", 1.0, 2) for s in SIDES})
    out.update({f"{s}_img_s": round(batch / statistics.median(times[s]) * 1e3, 1) for s in SIDES})
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-reps", type=int, default=10, help="training steps per side (0: skip item 2)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "dwconv", "device": torch.cuda.get_device_name(0)}), flush=True)
    for c, hw, stride in SHAPES:
        shape_bench(a.batch, c, hw, stride, a.warmup, a.reps, dev)
    if a.step_reps:
        step_bench(a.batch, 3, a.step_reps, dev)


if __name__ == "__main__":
    main()
