"""The squeeze-and-excitation kernels (csrc/ops_se.hip) against the same composition in stock torch (channels_last
bf16) on one device, at the four SE-ResNe(X)t-50 shapes (batch 256, input 224).

1. Per shape: squeeze, scale, backward reduce and backward apply, each alternated with torch's composition on the same
   tensors (``--inner`` launches of one side between two HIP events, then the other side, per repetition); median and
   min - max per launch, and the bytes/s of the ops kernel from the bytes it must move: the activation once for the
   squeeze, 3 x for the scale (u, idt, out), 4 x for the reduce (dout, out, u, didt), 3 x for the apply (dout, out, du).
2. One whole ``se_resnext50_32x4d`` training step (forward, loss, backward, SGD), ``OpsModel`` against stock PyTorch
   (channels_last, bf16 autocast), alternated.

    python bench/se_bench.py [--batch 256] [--reps 20] [--inner 10] [--step-reps 8] | tee profiles/se_bench.log
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

SHAPES = [(56, 256), (28, 512), (14, 1024), (7, 2048)]  # H (= W), C
PASSES = {"squeeze": 1, "scale": 3, "bwd_reduce": 4, "bwd_apply": 3}  # activation-sized tensors each kernel moves
SIDES = ("ops", "torch")
BF16 = torch.bfloat16


def _stats(ts, unit="us", scale=1e3, digits=1):
    return {f"median_{unit}": round(statistics.median(ts) * scale, digits),
            f"min_{unit}": round(min(ts) * scale, digits), f"max_{unit}": round(max(ts) * scale, digits)}


def _alternate(fns, warmup, reps, inner=1):
    """Milliseconds per call of each of `fns` (name -> callable): per repetition `inner` calls of one, then of the
    next, each run between two HIP events."""
    times = {k: [] for k in fns}
    for rep in range(warmup + reps):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            if rep >= warmup:
                times[name].append(t0.elapsed_time(t1) / inner)
    return times


def shape_bench(batch, hw, c, warmup, reps, inner, dev):
    g = torch.Generator().manual_seed(c + hw)
    p = hw * hw
    u, idt, dout = (torch.randn(batch, hw, hw, c, generator=g).to(BF16).to(dev) for _ in range(3))
    z = (2.0 * torch.randn(batch, c, generator=g)).to(dev)
    ds = torch.randn(batch, c, generator=g).to(BF16).to(dev)
    out = F.se_scale_fwd(u, z, idt)
    ut, it, dt, ot = (t.permute(0, 3, 1, 2) for t in (u, idt, dout, out))  # the same memory as channels_last NCHW

    def gate():
        return torch.sigmoid(z)[:, :, None, None]

    def t_reduce():
        didt = dt * (ot > 0)
        gg = torch.sigmoid(z)
        return didt, (didt * ut).sum((2, 3), dtype=torch.float32) * gg * (1 - gg)

    pairs = {
        "squeeze": (lambda: F.se_squeeze_fwd(u), lambda: ut.mean((2, 3))),
        "scale": (lambda: F.se_scale_fwd(u, z, idt), lambda: torch.relu(ut * gate().to(BF16) + it)),
        "bwd_reduce": (lambda: F.se_bwd_reduce(dout, out, u, z)[1], lambda: t_reduce()[1]),
        "bwd_apply": (lambda: F.se_bwd_apply(dout, out, z, ds),
                      lambda: dt * (ot > 0) * gate().to(BF16) + (ds / p)[:, :, None, None]),
    }
    for k, (a, b) in pairs.items():
        o, t = a().float(), b().float()
        t = t.permute(0, 2, 3, 1) if t.dim() == 4 else t
        rel = round(((o - t).norm() / t.norm()).item(), 5)  # agreement of the two sides (torch rounds more often)
        times = _alternate({"ops": a, "torch": b}, warmup, reps, inner)
        res = {"bench": "se", "pass": k, "batch": batch, "C": c, "HW": hw, "reps": reps, "inner": inner,
               "ops_vs_torch_rel_l2": rel}
        res.update({s: _stats(times[s]) for s in SIDES})
        res["ops_GBps"] = round(PASSES[k] * u.numel() * 2 / (statistics.median(times["ops"]) * 1e-3) / 1e9, 1)
        print(json.dumps(res), flush=True)


def step_bench(batch, warmup, reps, dev):
    from distributeddataparallel_cifar10_amd.models.resnet50 import se_resnext50_32x4d
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    torch.manual_seed(0)
    nets = {"ops": se_resnext50_32x4d().to(dev),
            "torch": se_resnext50_32x4d().to(dev).to(memory_format=torch.channels_last)}
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
            with torch.autocast("cuda", dtype=BF16):
                loss = TF.cross_entropy(run[side](xc), y)
        loss.backward()
        opts[side].step()

    times = _alternate({s: (lambda s=s: step(s)) for s in SIDES}, warmup, reps)
    res = {"bench": "se_resnext50_32x4d_train_step", "batch": batch, "reps": reps}
    res.update({s: _stats(times[s], "ms", 1.0, 2) for s in SIDES})
    res.update({f"{s}_img_s": round(batch / statistics.median(times[s]) * 1e3, 1) for s in SIDES})
    print(json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed window")
    ap.add_argument("--step-reps", type=int, default=8, help="training steps per side (0: skip item 2)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "se", "device": torch.cuda.get_device_name(0)}), flush=True)
    for hw, c in SHAPES:
        shape_bench(a.batch, hw, c, a.warmup, a.reps, a.inner, dev)
    if a.step_reps:
        step_bench(a.batch, 3, a.step_reps, dev)


if __name__ == "__main__":
    main()
