"""The fused attention kernels (csrc/ops_attn.hip) against torch's ``scaled_dot_product_attention`` on one device, at
batch 256, heads 3 / 6 / 12 of width 64 (ViT-Tiny / Small / Base) and 65, 197 and 256 tokens.

1. Per shape, forward and backward, three sides alternated on the same data (``--inner`` launches of one side between
   two HIP events, then the next side, per repetition); median and min - max per launch:
     ops           k_attn_fwd / k_attn_bwd on the qkv linear's [B, L, 3, H, D] output;
     torch_kernel  SDPA on pre-transposed contiguous [B, H, L, D] operands: the kernel alone;
     torch_model   SDPA from the [B, L, 3, H, D] tensor to a contiguous [B, L, H D] result, with the permutes and the
                   copy torch needs: what a model pays.
   The torch backward is ``autograd.grad`` over a retained graph.  ops_GBps: the bytes the ops kernel must move (forward:
   qkv in, o and lse out; backward: qkv, o, dout and lse in, dqkv out) over its median time.
2. One whole ViT-Tiny training step at 224 / 16 (forward, loss, backward, SGD), ``OpsModel`` against stock PyTorch
   under bf16 autocast, alternated.

    python bench/attn_bench.py [--batch 256] [--reps 20] [--inner 10] [--step-reps 8] | tee profiles/attn_bench.log
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

HEADS, TOKENS, D = (3, 6, 12), (65, 197, 256), 64
SIDES = ("ops", "torch_kernel", "torch_model")
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


def shape_bench(b, h, l, warmup, reps, inner, dev):
    g = torch.Generator().manual_seed(100 * l + h)
    qkv = torch.randn(b, l, 3, h, D, generator=g).to(BF16).to(dev)
    dout = torch.randn(b, l, h, D, generator=g).to(BF16).to(dev)
    scale = D ** -0.5
    o, lse = F.attention_fwd(qkv, scale)
    q, k, v = (t.contiguous().requires_grad_() for t in qkv.permute(2, 0, 3, 1, 4))  # [B, H, L, D] each
    dout_t = dout.transpose(1, 2).contiguous()
    x = qkv.clone().requires_grad_()

    def model_fwd():
        xq, xk, xv = x.permute(2, 0, 3, 1, 4)
        return TF.scaled_dot_product_attention(xq, xk, xv).transpose(1, 2).reshape(b, l, h * D)

    kernel_out, model_out = TF.scaled_dot_product_attention(q, k, v), model_fwd()
    passes = {
        "fwd": {"ops": lambda: F.attention_fwd(qkv, scale),
                "torch_kernel": lambda: TF.scaled_dot_product_attention(q, k, v), "torch_model": model_fwd},
        "bwd": {"ops": lambda: F.attention_bwd(qkv, o, lse, dout, scale),
                "torch_kernel": lambda: torch.autograd.grad(kernel_out, (q, k, v), dout_t, retain_graph=True),
                "torch_model": lambda: torch.autograd.grad(model_out, x, dout.view(b, l, h * D), retain_graph=True)},
    }
    act = b * l * h * D * 2  # bytes of one [B, L, H, D] bf16 tensor
    need = {"fwd": 4 * act + lse.numel() * 4, "bwd": 8 * act + lse.numel() * 4}
    agree = {"fwd": (o.view(b, l, h * D).float(), model_out.detach().float()),
             "bwd": (passes["bwd"]["ops"]().float(), passes["bwd"]["torch_model"]()[0].float())}
    for name, fns in passes.items():
        got, want = agree[name]
        times = _alternate(fns, warmup, reps, inner)
        res = {"bench": "attn", "pass": name, "batch": b, "heads": h, "L": l, "reps": reps, "inner": inner,
               "ops_vs_torch_rel_l2": round(((got - want).norm() / want.norm()).item(), 5)}
        res.update({s: _stats(times[s]) for s in SIDES})
        res["ops_GBps"] = round(need[name] / (statistics.median(times["ops"]) * 1e-3) / 1e9, 1)
        print(json.dumps(res), flush=True)


def step_bench(batch, warmup, reps, dev):
    from distributeddataparallel_cifar10_amd.models.vit import vit_tiny
    from distributeddataparallel_cifar10_amd.ops import OpsModel, cross_entropy
    torch.manual_seed(0)
    nets = {s: vit_tiny(img_size=224, patch=16).to(dev) for s in ("ops", "torch")}
    run = {"ops": OpsModel(nets["ops"]), "torch": nets["torch"]}
    opts = {s: torch.optim.SGD(nets[s].parameters(), lr=1e-3, momentum=0.9) for s in nets}
    x = torch.randn(batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (batch,), device=dev)

    def step(side):
        opts[side].zero_grad(set_to_none=True)
        if side == "ops":
            loss = cross_entropy(run[side](x), y)
        else:
            with torch.autocast("cuda", dtype=BF16):
                loss = TF.cross_entropy(run[side](x), y)
        loss.backward()
        opts[side].step()

    times = _alternate({s: (lambda s=s: step(s)) for s in nets}, warmup, reps)
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
    print(json.dumps({"bench": "attn", "device": torch.cuda.get_device_name(0)}), flush=True)
    for h in HEADS:
        for l in TOKENS:
            shape_bench(a.batch, h, l, a.warmup, a.reps, a.inner, dev)
    if a.step_reps:
        step_bench(a.batch, 3, a.step_reps, dev)


if __name__ == "__main__":
    main()
