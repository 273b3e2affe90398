"""The fused residual-add LayerNorm and GELU kernels (csrc/ops_ln.hip) against the torch compositions they replace in
``OpsModel``'s ViT forward, on one device, at batch 256, 65 and 197 tokens and widths 192 / 384 / 768 (ViT-Tiny / Small
/ Base; the GELU runs on the MLP's [B L, 4 dim] activation).

1. Per shape, two sides alternated on the same data (``--inner`` launches of one side between two HIP events, then the
   other side, per repetition); median and min - max per launch:
     ln_fwd    ``layer_norm_fwd(x, delta, gamma, beta)`` against ``h = x + delta``, the two ``.to(bf16)`` casts of the
               fp32 parameters and ``torch.nn.functional.layer_norm``;
     ln_bwd    ``layer_norm_bwd(h, dy, dres, gamma, stats)`` against ``autograd.grad`` of that composition over a
               retained graph, with the gradients of both h and y (the join) down to x, delta and the fp32 parameters;
     gelu_fwd  ``gelu_fwd(z)`` against ``torch.nn.functional.gelu(z)``;
     gelu_bwd  ``gelu_bwd(dy, z)`` against torch's GELU backward followed by ``dy_prep`` (what ``linear``'s backward
               ran before).
   ops_GBps: the bytes the ops kernels must move (ln_fwd: x, delta in, hsum, y, stats out; ln_bwd: h, dy, dres, stats
   in, dx out; gelu_fwd: z in, a out; gelu_bwd: dy, z in, dz out) over their median time.
2. One whole ViT-Tiny training step at 224 / 16 (forward, loss, backward, SGD) under ``OpsModel``: the fused path
   against the torch path (``DCA_OPS_LN=0``'s), alternated in one process.

    python bench/ln_bench.py [--batch 256] [--reps 20] [--inner 10] [--step-reps 8] | tee profiles/ln_bench.log
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
from distributeddataparallel_cifar10_amd.ops import models  # noqa: E402

TOKENS, DIMS = (65, 197), (192, 384, 768)
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


def _rel(a, b):
    return round(((a.float() - b.float()).norm() / b.float().norm()).item(), 5)


def shape_bench(b, l, dim, warmup, reps, inner, dev):
    g = torch.Generator().manual_seed(1000 * l + dim)
    m, eps = b * l, 1e-5
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, delta, dy, dres = (rn(m, dim).to(BF16).to(dev) for _ in range(4))
    gamma, beta = (1 + 0.1 * rn(dim)).to(dev), (0.1 * rn(dim)).to(dev)
    hsum, y, stats = F.layer_norm_fwd(x, delta, gamma, beta, eps)
    tx, td, tg, tb = (t.clone().requires_grad_() for t in (x, delta, gamma, beta))

    def torch_ln():
        h = tx + td
        return h, TF.layer_norm(h, (dim,), tg.to(BF16), tb.to(BF16), eps)

    th, ty = torch_ln()
    z, dz_in = rn(m, 4 * dim).to(BF16).to(dev), rn(m, 4 * dim).to(BF16).to(dev)
    tz = z.clone().requires_grad_()
    ta = TF.gelu(tz)
    passes = {
        "ln_fwd": {"ops": lambda: F.layer_norm_fwd(x, delta, gamma, beta, eps), "torch": torch_ln},
        "ln_bwd": {"ops": lambda: F.layer_norm_bwd(hsum, dy, dres, gamma, stats),
                   "torch": lambda: torch.autograd.grad((th, ty), (tx, td, tg, tb), (dres, dy), retain_graph=True)},
        "gelu_fwd": {"ops": lambda: F.gelu_fwd(z), "torch": lambda: TF.gelu(z)},
        "gelu_bwd": {"ops": lambda: F.gelu_bwd(dz_in, z),
                     "torch": lambda: F.dy_prep(torch.autograd.grad(ta, tz, dz_in, retain_graph=True)[0])},
    }
    act, wide = m * dim * 2, m * 4 * dim * 2  # bytes of one bf16 activation
    need = {"ln_fwd": 4 * act + 8 * m, "ln_bwd": 4 * act + 8 * m, "gelu_fwd": 2 * wide, "gelu_bwd": 3 * wide}
    agree = {"ln_fwd": (y, ty), "ln_bwd": (passes["ln_bwd"]["ops"]()[0], passes["ln_bwd"]["torch"]()[0]),
             "gelu_fwd": (passes["gelu_fwd"]["ops"](), ta), "gelu_bwd": (passes["gelu_bwd"]["ops"]()[0],
                                                                         passes["gelu_bwd"]["torch"]()[0])}
    for name, fns in passes.items():
        times = _alternate(fns, warmup, reps, inner)
        res = {"bench": "ln", "pass": name, "batch": b, "L": l, "dim": dim, "reps": reps, "inner": inner,
               "ops_vs_torch_rel_l2": _rel(*agree[name])}
        res.update({s: _stats(times[s]) for s in SIDES})
        res["ops_GBps"] = round(need[name] / (statistics.median(times["ops"]) * 1e-3) / 1e9, 1)
        print(json.dumps(res), flush=True)


def step_bench(batch, warmup, reps, dev):
    from distributeddataparallel_cifar10_amd.models.vit import vit_tiny
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    torch.manual_seed(0)
    nets = {s: vit_tiny(img_size=224, patch=16).to(dev) for s in ("ops_ln", "torch_ln")}
    run = {s: OpsModel(nets[s]) for s in nets}
    opts = {s: torch.optim.SGD(nets[s].parameters(), lr=1e-3, momentum=0.9) for s in nets}
    x = torch.randn(batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (batch,), device=dev)

    def step(side):
        models.OPS_LN = side == "ops_ln"  # (read by OpsModel._vit at every forward)
        opts[side].zero_grad(set_to_none=True)
        cross_entropy(run[side](x), y).backward()
        opts[side].step()

    times = _alternate({s: (lambda s=s: step(s)) for s in nets}, warmup, reps)
    models.OPS_LN = True
    res = {"bench": "vit_tiny_224_train_step", "batch": batch, "reps": reps}
    res.update({s: _stats(times[s], "ms", 1.0, 2) for s in nets})
    res.update({f"{s}_img_s": round(batch / statistics.median(times[s]) * 1e3, 1) for s in nets})
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
    print(json.dumps({"bench": "ln", "device": torch.cuda.get_device_name(0)}), flush=True)
    for dim in DIMS:
        for l in TOKENS:
            shape_bench(a.batch, l, dim, a.warmup, a.reps, a.inner, dev)
    if a.step_reps:
        step_bench(a.batch, 3, a.step_reps, dev)


if __name__ == "__main__":
    main()
