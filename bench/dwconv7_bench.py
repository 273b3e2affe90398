"""The depthwise 7x7 kernels (csrc/ops_dwconv7.hip) against torch's ``conv2d(groups=C)`` (channels_last bf16) on one
device, at the four depthwise shapes of ConvNeXt-T (batch 256, input 224): C / H = 96 / 56, 192 / 28, 384 / 14, 768 / 7.

1. Per shape: forward (with bias), input gradient and weight + bias gradient, each alternated with torch's on the same
   tensors (one of each per repetition) between two HIP events; median and min - max, and the bytes/s of the ops kernel
   against the floor of every tensor moved once (forward and input gradient: one read, one write; weight gradient: two
   reads).  torch's weight-gradient side does not compute the bias gradient.
2. One whole ``convnext_tiny`` training step at 224 (forward, loss, backward, SGD), ``OpsModel`` against stock PyTorch
   (channels_last, bf16 autocast), alternated.

    python bench/dwconv7_bench.py [--batch 256] [--reps 30] [--step-reps 10] | tee profiles/dwconv7_bench.log
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

from dwconv_bench import SIDES, _alternate, _stats  # noqa: E402  (bench/dwconv_bench.py: the script's own directory)
from distributeddataparallel_cifar10_amd.ops import functional as F  # noqa: E402

SHAPES = [(96, 56), (192, 28), (384, 14), (768, 7)]  # C, H (= W)


def shape_bench(batch, c, hw, warmup, reps, dev):
    g = torch.Generator().manual_seed(c + hw)
    x = torch.randn(batch, hw, hw, c, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn(batch, hw, hw, c, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(c, 1, 7, 7, generator=g) * 0.15).to(dev)
    b = torch.randn(c, generator=g).to(dev)
    wb, bb = w.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), b.to(torch.bfloat16)
    xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # the same memory as channels_last NCHW
    conv = dict(stride=1, padding=3, groups=c)
    pairs = {
        "fwd": (lambda: F.dwconv7_fwd(x, w, b), lambda: TF.conv2d(xt, wb, bb, **conv)),
        "dgrad": (lambda: F.dwconv7_dgrad(dy, w), lambda: torch.nn.grad.conv2d_input(xt.shape, wb, dyt, **conv)),
        "wgrad": (lambda: F.dwconv7_wgrad(x, dy)[0], lambda: torch.nn.grad.conv2d_weight(xt, wb.shape, dyt, **conv)),
    }
    rel = {}  # agreement of the two sides (bf16 rounding of the outputs only)
    for k, (a, t) in pairs.items():
        o, t = a().float(), t().float()
        t = t.permute(0, 2, 3, 1) if k != "wgrad" else t
        rel[k] = round(((o - t).norm() / t.norm()).item(), 5)
    nbytes = (x.numel() + dy.numel()) * 2
    for k, (a, t) in pairs.items():
        times = _alternate({"ops": a, "torch": t}, warmup, reps)
        out = {"bench": "dwconv7", "pass": k, "batch": batch, "C": c, "HW": hw, "reps": reps,
               "ops_vs_torch_rel_l2": rel[k]}
        out.update({s: _stats(times[s]) for s in SIDES})
        out["ops_GBps"] = round(nbytes / (statistics.median(times["ops"]) * 1e-3) / 1e9, 1)
        print(json.dumps(out), flush=True)


def step_bench(batch, warmup, reps, dev):
    from distributeddataparallel_cifar10_amd.models.convnext import convnext_tiny
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    torch.manual_seed(0)
    nets = {"ops": convnext_tiny().to(dev), "torch": convnext_tiny().to(dev).to(memory_format=torch.channels_last)}
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
    out = {"bench": "convnext_tiny_224_train_step", "batch": batch, "reps": reps}
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
    print(json.dumps({"bench": "dwconv7", "device": torch.cuda.get_device_name(0)}), flush=True)
    for c, hw in SHAPES:
        shape_bench(a.batch, c, hw, a.warmup, a.reps, dev)
    if a.step_reps:
        step_bench(a.batch, 3, a.step_reps, dev)


if __name__ == "__main__":
    main()
