"""Cost of the crop + flip pass (csrc/augment.hip) on one device, against a device-to-device copy of the same bytes,
and what ``--augment`` adds to a training epoch.

1. ``k_augment_u8`` over all ids of an N-image dataset in a sampler permutation (rows scattered; reads N x 3 KiB and
   writes N x 3 KiB), the id list already on the device: the kernel between two HIP events.
2. The yardstick: ``copy_`` of the same tensor, device to device (the same bytes read and written).
3. ``main.py --synthetic N --epochs E --dtype bf16`` with and without ``--augment``, each run a process of its own:
   the per-epoch seconds of the metrics records, epochs 2..E (the first epoch holds the graph captures).

Items 1 and 2 are interleaved (one of each per repetition), and so are the runs of item 3.  Prints one JSON line with
the median and the min - max spread of every item; ``within_1p25x`` says whether the kernel's median is within 1.25x
of the copy's.

    python bench/augment_bench.py [--images 50000] [--reps 9] [--train-reps 9] [--epochs 11] | tee profiles/augment_bench.log
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributeddataparallel_cifar10_amd.data.augment import augment_reference  # noqa: E402
from distributeddataparallel_cifar10_amd.data.sampler import distributed_indices  # noqa: E402
from distributeddataparallel_cifar10_amd.runtime import native  # noqa: E402


def _stats(ts, unit="ms", digits=4):
    return {f"median_{unit}": round(statistics.median(ts), digits), f"min_{unit}": round(min(ts), digits),
            f"max_{unit}": round(max(ts), digits)}


def _train_run(images: int, epochs: int, augment: bool) -> list:
    """One ``main.py`` run; the seconds of epochs 2..`epochs`."""
    with tempfile.TemporaryDirectory() as tmp:
        mj = os.path.join(tmp, "metrics.json")
        cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", str(images), "--epochs", str(epochs),
               "--dtype", "bf16", "--world-size", "1", "--no-checkpoint", "--metrics-json", mj]
        res = subprocess.run(cmd + (["--augment"] if augment else []), cwd=ROOT, capture_output=True, text=True,
                             timeout=600)
        if res.returncode != 0:
            raise RuntimeError(f"main.py failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
        recs = [json.loads(ln) for ln in open(mj).read().splitlines()]
    recs = [r for r in recs if "epoch" in r]
    assert all((r["augment"] is not None) == augment for r in recs)
    return [r["seconds"] for r in recs if r["epoch"] >= 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=50000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--train-reps", type=int, default=9, help="main.py runs per variant (0: skip item 3)")
    ap.add_argument("--epochs", type=int, default=11)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    lib = native.require_native()
    n = a.images
    src = torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    order = distributed_indices(n, 1, 0, seed=0, epoch=0)  # the sampler's permutation of range(n)
    ids = torch.from_numpy(order.astype(np.int32)).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        rc = lib.dca_augment_u8(src.data_ptr(), dst.data_ptr(), ids.data_ptr(), int(ids.numel()), n, 0, 1, 4, 1, st)
        if rc != 0:
            raise RuntimeError(lib.dca_augment_last_error().decode())

    items = {"k_augment_u8": kernel, "copy_d2d": lambda: dst.copy_(src)}
    times = {k: [] for k in items}
    for rep in range(a.warmup + a.reps):
        for name, fn in items.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    kernel()
    torch.cuda.synchronize()
    sample = torch.from_numpy(np.unique(order[:256]))  # the timed output is the definition's (a sample of rows)
    ok = bool(torch.equal(dst[sample.to(dev)].cpu(), augment_reference(src.cpu(), sample, 0, 1)[sample]))
    nbytes = 2 * n * 3072
    out = {"bench": "augment", "images": n, "bytes_moved": nbytes, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "output_checked": ok}
    for name, ts in times.items():
        out[name] = {**_stats(ts), "tb_per_s": round(nbytes / statistics.median(ts) * 1e-9, 3)}
    out["kernel_over_copy"] = round(out["k_augment_u8"]["median_ms"] / out["copy_d2d"]["median_ms"], 3)
    out["within_1p25x"] = out["kernel_over_copy"] <= 1.25
    if a.train_reps:
        del src, dst, ids
        torch.cuda.empty_cache()
        epochs = {"train_plain": [], "train_augment": []}
        for rep in range(a.train_reps):
            epochs["train_plain"] += _train_run(n, a.epochs, False)
            epochs["train_augment"] += _train_run(n, a.epochs, True)
            print(f"[augment_bench] training runs: {rep + 1} of {a.train_reps} pairs done", file=sys.stderr, flush=True)
        for name, ts in epochs.items():
            out[name] = {**_stats(ts, "epoch_s", 5), "runs": a.train_reps, "epochs_per_run": a.epochs - 1}
        out["augment_epoch_extra_ms"] = round(1e3 * (out["train_augment"]["median_epoch_s"]
                                                     - out["train_plain"]["median_epoch_s"]), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
