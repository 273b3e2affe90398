"""Cost of the engine's optimiser pass: microseconds per training step of the plain fused engine (its own SGD inside
the reduction kernel) against the same engine with ``momentum 0.9 + weight decay 5e-4 + cosine table`` (gradient
reduced unapplied, then ``k_apply_opt``) and against that engine with the pass in its EMA form (``optimizer+ema``:
decay 0.999, warm-up on) and in its AdamW form (``adamw``: betas (0.9, 0.999), weight decay 5e-2, the same table),
and that AdamW engine with gradient-norm clipping (``adamw+clip``: ``max_grad_norm`` 0.05, a limit every step exceeds;
one more kernel, ``k_grad_sqnorm``, in front of the pass's CLIP form), and the AdamW engine with gradient accumulation
(``adamw+accum4``: ``accumulate_steps`` 4; one more kernel, ``k_grad_accum``, in front of the pass's ACC form, which
applies an update on every fourth micro-step only; reported per micro-step), sliced engine, bf16 and fp32, batch 32,
one GPU.

One process; the engines of a precision live side by side and are timed in interleaved repetitions (plain, optimiser,
optimiser + EMA, AdamW, AdamW + clip, plain, ...), so clock and thermal drift hit all alike.  Each repetition is `--steps` graph-replayed steps between two
HIP events recorded on the engine's stream; graphs are captured before the first timed repetition.  Reported: median
and min / max over the repetitions, and the difference of the medians.

    python bench/opt_bench.py [--steps 320] [--reps 9] [--batch 32] [--no-ema] [--no-adam] [--no-clip] [--no-accum]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _engine(dtype, batch, optimizer, data, labels, order):
    from distributeddataparallel_cifar10_amd.models.netresdeep import NetResDeep
    from distributeddataparallel_cifar10_amd.runtime.engine import EngineConfig, NetResDeepEngine
    torch.manual_seed(1234)
    model = NetResDeep().to(data.device)
    eng = NetResDeepEngine(model, data, labels, EngineConfig(batch_max=batch, dtype=dtype, persistent=True,
                                                             optimizer=optimizer), max_indices=len(order))
    eng.set_indices(order)
    eng.precapture(batch)
    return eng


def _timed(eng, batch, steps):
    """Microseconds per step of `steps` graph-replayed steps (HIP events on the engine's stream)."""
    st = torch.cuda.ExternalStream(eng.lib.dca_engine_stream(eng.h), device=eng.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.set_cursor(0)
    a.record(st)
    eng.run(batch, steps)
    b.record(st)
    b.synchronize()
    eng.check_errors()
    return 1e3 * a.elapsed_time(b) / steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--no-ema", action="store_true", help="time plain and optimizer only (A/B against older trees)")
    ap.add_argument("--no-adam", action="store_true", help="leave the adamw engine out (A/B against older trees)")
    ap.add_argument("--no-clip", action="store_true", help="leave the adamw+clip engine out (A/B against older trees)")
    ap.add_argument("--no-accum", action="store_true",
                    help="leave the adamw+accum4 engine out (A/B against older trees)")
    a = ap.parse_args(argv)
    from distributeddataparallel_cifar10_amd.data.synthetic import synthetic_cifar
    from distributeddataparallel_cifar10_amd.runtime.engine import OptimizerConfig
    from distributeddataparallel_cifar10_amd.utils.schedule import lr_table
    dev = torch.device("cuda", 0)
    data, labels = synthetic_cifar(16384, seed=0)
    data, labels = data.to(dev), labels.to(dev)
    order = np.resize(np.arange(16384, dtype=np.int32), max(a.steps, a.warmup) * a.batch)
    total = a.warmup + a.steps * a.reps
    out = {}
    for dtype in ("bf16", "fp32"):
        table = lr_table("cosine", 1e-2, total, warmup_steps=32)
        opt = OptimizerConfig(momentum=0.9, weight_decay=5e-4, lr_table=table)
        engines = {"plain": _engine(dtype, a.batch, None, data, labels, order),
                   "optimizer": _engine(dtype, a.batch, opt, data, labels, order)}
        if not a.no_ema:
            ema = OptimizerConfig(momentum=0.9, weight_decay=5e-4, lr_table=table, ema_decay=0.999, ema_warmup=True)
            engines["optimizer+ema"] = _engine(dtype, a.batch, ema, data, labels, order)
        if not a.no_adam:
            adamw = OptimizerConfig(kind="adamw", betas=(0.9, 0.999), weight_decay=5e-2, lr_table=table)
            engines["adamw"] = _engine(dtype, a.batch, adamw, data, labels, order)
            if not a.no_clip:
                clip = OptimizerConfig(kind="adamw", betas=(0.9, 0.999), weight_decay=5e-2, lr_table=table,
                                       max_grad_norm=0.05)
                engines["adamw+clip"] = _engine(dtype, a.batch, clip, data, labels, order)
            if not a.no_accum:
                accum = OptimizerConfig(kind="adamw", betas=(0.9, 0.999), weight_decay=5e-2, lr_table=table,
                                        accumulate_steps=4)
                engines["adamw+accum4"] = _engine(dtype, a.batch, accum, data, labels, order)
        for eng in engines.values():
            _timed(eng, a.batch, a.warmup)
        us = {k: [] for k in engines}
        for _ in range(a.reps):
            for k, eng in engines.items():  # interleaved
                us[k].append(_timed(eng, a.batch, a.steps))
        for k, eng in engines.items():
            loss, _ = eng.read_loss(reset=True)
            assert np.isfinite(loss), (dtype, k, loss)
            if k == "adamw+clip":  # the limit did clip
                norm, clipped = eng.grad_norm()
                assert clipped > 0, (dtype, norm, clipped)
                print(f"{dtype} adamw+clip: {clipped} of {total} steps clipped, last norm {norm:.4f}", flush=True)
            if k == "adamw+accum4":  # one optimiser step per four micro-steps
                assert eng.optimizer_step() == total // 4 and eng.accumulate_phase() == total % 4
                print(f"{dtype} adamw+accum4: {eng.optimizer_step()} optimiser steps in {total} micro-steps", flush=True)
            eng.close()
        med = {k: statistics.median(v) for k, v in us.items()}
        out[dtype] = {"plain_us": round(med["plain"], 2), "optimizer_us": round(med["optimizer"], 2),
                      "delta_us": round(med["optimizer"] - med["plain"], 2)}
        if "optimizer+ema" in med:
            out[dtype].update(ema_us=round(med["optimizer+ema"], 2),
                              ema_delta_us=round(med["optimizer+ema"] - med["optimizer"], 2))
        if "adamw" in med:
            out[dtype].update(adamw_us=round(med["adamw"], 2),
                              adamw_delta_us=round(med["adamw"] - med["optimizer"], 2))
        if "adamw+clip" in med:
            out[dtype].update(clip_us=round(med["adamw+clip"], 2),
                              clip_delta_us=round(med["adamw+clip"] - med["adamw"], 2))
        if "adamw+accum4" in med:
            out[dtype].update(accum_us=round(med["adamw+accum4"], 2),
                              accum_delta_us=round(med["adamw+accum4"] - med["adamw"], 2))
        for k, v in us.items():
            print(f"{dtype} {k:13s} us/step: median {med[k]:.2f}  min {min(v):.2f}  max {max(v):.2f}  "
                  f"reps {' '.join(f'{x:.2f}' for x in v)}", flush=True)
        print(f"{dtype} optimiser pass costs {med['optimizer'] - med['plain']:+.2f} us/step "
              f"({100 * (med['optimizer'] / med['plain'] - 1):+.1f} %)", flush=True)
        if "optimizer+ema" in med:
            print(f"{dtype} EMA form costs {med['optimizer+ema'] - med['optimizer']:+.2f} us/step over optimizer "
                  f"({100 * (med['optimizer+ema'] / med['optimizer'] - 1):+.1f} %)", flush=True)
        if "adamw" in med:
            print(f"{dtype} AdamW form costs {med['adamw'] - med['optimizer']:+.2f} us/step over optimizer "
                  f"({100 * (med['adamw'] / med['optimizer'] - 1):+.1f} %)", flush=True)
        if "adamw+clip" in med:
            print(f"{dtype} clipping costs {med['adamw+clip'] - med['adamw']:+.2f} us/step over adamw "
                  f"({100 * (med['adamw+clip'] / med['adamw'] - 1):+.1f} %)", flush=True)
        if "adamw+accum4" in med:
            print(f"{dtype} accumulation (K = 4) costs {med['adamw+accum4'] - med['adamw']:+.2f} us/micro-step over "
                  f"adamw ({100 * (med['adamw+accum4'] / med['adamw'] - 1):+.1f} %)", flush=True)
    print(json.dumps({"bench": "opt_bench", "engine": "sliced", "batch": a.batch, "steps": a.steps, "reps": a.reps,
                      **out}), flush=True)


if __name__ == "__main__":
    main()
