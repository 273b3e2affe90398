"""The PPE model's ROI section on one device: ``ops.roi_align`` (csrc/ops_roi.hip, DCA_OPS_ROI=1) against the torch
``grid_sample`` chain it replaces (DCA_OPS_ROI=0), at the application's shape.

1. The section alone, forward + backward between two HIP events: a batch of 32 ``SyntheticPPE`` images' boxes over
   [32, 8, 10, 1024] NHWC bf16 stride-16 features, 4 x 4 bins, gradient [N, 4, 4, 1024] bf16.
2. A full ``ResNet101ROI`` training step (forward, BCE-with-logits, backward, SGD) of that batch.
3. The kernel launches of the section on each side (torch.profiler, a pass of its own after the timing).

The two sides are alternated (one of each per repetition) in this one call.  Prints one JSON line per item with the
median and the min - max spread of each side.

    python bench/roi_bench.py [--batch 32] [--reps 50] [--step-reps 15] | tee profiles/roi_bench.log
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributeddataparallel_cifar10_amd.apps import ppe  # noqa: E402
from distributeddataparallel_cifar10_amd.ops import roi_align  # noqa: E402

SIDES = ("ops", "torch")  # DCA_OPS_ROI = 1 / 0


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


def _launches(fn) -> int:
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events()
               if e.device_type == DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=15, help="training steps per side (0: skip item 2)")
    ap.add_argument("--layers", default="3,4,23,3", help="blocks per stage of the trunk (ResNet-101)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    ds = ppe.SyntheticPPE(a.batch, seed=0)
    imgs, boxes, labels, _ = ds.detection_collate([ds[i] for i in range(a.batch)])
    boxes, labels = boxes.to(dev), labels.to(dev)
    model = ppe.build_model(None, 3, layers=tuple(int(v) for v in a.layers.split(","))).to(dev)
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(a.batch, 8, 10, 1024, generator=g).to(torch.bfloat16).to(dev).requires_grad_()
    dout = torch.randn(boxes.shape[0], model.bins, model.bins, 1024, generator=g).to(torch.bfloat16).to(dev)
    common = {"batch": a.batch, "boxes": int(boxes.shape[0]), "device": torch.cuda.get_device_name(0)}

    def section(side):
        if side == "ops":
            r = roi_align(feat, boxes, model.bins, 16.0)
        else:  # the chain ResNet101ROI._forward_ops runs with DCA_OPS_ROI=0
            r = model.roi_align(feat.permute(0, 3, 1, 2).float(), boxes.float(), 16.0)
            r = r.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
        feat.grad = None
        r.backward(dout)
        return r

    outs = {s: (section(s).detach().float(), feat.grad.float()) for s in SIDES}
    rel = [((outs["ops"][i] - outs["torch"][i]).norm() / outs["torch"][i].norm()).item() for i in (0, 1)]
    times = _alternate({s: (lambda s=s: section(s)) for s in SIDES}, a.warmup, a.reps)
    out = {"bench": "roi_section", **common, "reps": a.reps, "ops_vs_torch_rel_l2": [round(v, 5) for v in rel]}
    out.update({s: _stats(times[s]) for s in SIDES})
    print(json.dumps(out), flush=True)

    if a.step_reps:
        x = ppe.preprocess_img(imgs.to(dev).float())
        opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
        model.train()

        def step(side):
            ppe.OPS_ROI = side == "ops"
            opt.zero_grad()
            torch.nn.functional.binary_cross_entropy_with_logits(model(x, boxes), labels).backward()
            opt.step()

        times = _alternate({s: (lambda s=s: step(s)) for s in SIDES}, 3, a.step_reps)
        out = {"bench": "roi_train_step", **common, "layers": a.layers, "reps": a.step_reps}
        out.update({s: _stats(times[s], "ms", 1.0, 3) for s in SIDES})
        print(json.dumps(out), flush=True)

    launches = {s: _launches(lambda s=s: section(s)) for s in SIDES}
    print(json.dumps({"bench": "roi_section_launches", **common, **launches}), flush=True)


if __name__ == "__main__":
    main()
