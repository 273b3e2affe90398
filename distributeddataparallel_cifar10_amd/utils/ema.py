"""Exponential moving average (EMA) of the model's weights: the definition, its float64 oracle, and the host-side
averager of the ``ops`` / ``torch`` engines and the CPU (pure numpy / torch; no device needed).

Definition (the fused engine's optimiser pass, ``csrc/optimizer.hip`` ``k_apply_opt<BF, true>``, implements the same):

* decay of update ``k`` (0-based optimiser step index): ``decay``, or with warm-up ``min(decay, (1 + k) / (10 + k))``
  (timm ``ModelEmaV2`` / ``ModelEmaV3`` warm-up), ``decay`` in [0, 1);
* after the parameter update of step ``k``: ``e' = p' + d_k * (e - p')`` (``p'``: the new parameter value, ``e``: the
  average); in fp32 one subtract and one fused multiply-add, ``fmaf(d, e - p', p')``; with ``d = 0`` it is ``p'`` bit
  for bit;
* averaged: the parameter tensors and the floating-point buffers (BatchNorm ``running_mean`` / ``running_var``, the
  rank's module buffers as the step left them) with the same decay; integer buffers (``num_batches_tracked``) are
  copied -- ``torch.optim.swa_utils.AveragedModel(use_buffers=True)`` / ``ModelEmaV2`` semantics;
* the average starts as a copy of the model at the moment EMA is switched on.
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from typing import Optional

import numpy as np
import torch

from .checkpoint import cpu_state_dict, save_on_rank0, unwrap

WARMUP_NUM, WARMUP_DEN = 1.0, 10.0  # warm-up decay of update k: (1 + k) / (10 + k)


def check_decay(decay) -> float:
    d = float(decay)
    if not 0.0 <= d < 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"EMA decay must lie in [0, 1), got {decay!r}")
    return d


def ema_decay_at(k: int, decay: float, warmup: bool = False) -> float:
    """The decay of update `k` (0-based optimiser step index)."""
    d = check_decay(decay)
    if int(k) != k or k < 0:
        raise ValueError(f"the update index must be a non-negative integer, got {k!r}")
    return min(d, (WARMUP_NUM + int(k)) / (WARMUP_DEN + int(k))) if warmup else d


def ema_reference(e, p_new, d: float) -> np.ndarray:
    """One EMA update in float64 -- the oracle of every implementation: ``e' = p' + d * (e - p')``.  Takes arrays or
    tensors; returns a float64 numpy array."""
    e64, p64 = _f64(e), _f64(p_new)
    return p64 + float(d) * (e64 - p64)


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def ema_path(checkpoint_path: str) -> str:
    return f"{checkpoint_path}.ema.pt"


def save_ema_state(state: dict, checkpoint_path: str, rank: int = 0) -> Optional[str]:
    """Rank 0 writes ``<checkpoint>.ema.pt`` atomically: the averaged model as a reference-format state_dict (CPU
    tensors, the model's keys), so it loads strictly into the model and ``--eval-only --resume`` evaluates it."""
    if rank != 0:
        return None
    # (keys that share a tensor keep sharing it in the file, as in the checkpoint)
    return save_on_rank0(cpu_state_dict(state), ema_path(checkpoint_path))


def load_ema_state(checkpoint_path: str) -> Optional[dict]:
    """The state ``save_ema_state`` wrote beside `checkpoint_path` (CPU tensors), or None if there is no such file."""
    path = ema_path(checkpoint_path)
    if not os.path.exists(path):
        return None
    return torch.load(path, map_location="cpu", weights_only=True)


class ModelEma:
    """The average of `model` (a plain module, or a wrapper such as ``FlatBucketDDP`` / ``OpsModel`` around one), kept
    with torch ops on the model's device: call ``update(k)`` after the ``optimizer.step()`` of optimiser step `k`.

    With a ``FlatBucketDDP`` the parameters are averaged as its one flat buffer (three ops per step), otherwise per
    tensor (``torch._foreach_*``); floating-point buffers per tensor; integer buffers copied."""

    def __init__(self, model, decay: float, warmup: bool = False):
        self.decay, self.warmup = check_decay(decay), bool(warmup)
        self.net = unwrap(model)
        self.last_decay: Optional[float] = None  # the decay of the last update
        flat = getattr(model, "flat", None)
        self._flat = flat if isinstance(flat, torch.Tensor) and flat.is_floating_point() else None
        self._pnames = [n for n, _ in self.net.named_parameters()]
        with torch.no_grad():
            self._pavg_flat = self._flat.detach().clone() if self._flat is not None else None
            if self._pavg_flat is not None:
                # views of the averaged flat buffer where the live parameters are views of the live one
                self.params = model.named_views(self._pavg_flat)
            else:
                self.params = {n: p.detach().clone() for n, p in self.net.named_parameters()}
            self.buffers = {n: b.detach().clone() for n, b in self.net.named_buffers()}

    # ---- the update ---------------------------------------------------------------------------------------------
    @staticmethod
    def _lerp_to(avg: list, live: list, d: float) -> None:
        """avg <- live + d * (avg - live), in place."""
        if not avg:
            return
        torch._foreach_sub_(avg, live)
        torch._foreach_mul_(avg, d)
        torch._foreach_add_(avg, live)

    @torch.no_grad()
    def update(self, k: int) -> float:
        """Update `k` (the 0-based index of the optimiser step just taken); returns the decay it used."""
        d = ema_decay_at(k, self.decay, self.warmup)
        if self._pavg_flat is not None:
            self._lerp_to([self._pavg_flat], [self._flat.detach()], d)
        else:
            live = dict(self.net.named_parameters())
            self._lerp_to([self.params[n] for n in self._pnames], [live[n].detach() for n in self._pnames], d)
        favg, flive = [], []
        for n, b in self.net.named_buffers():
            if b.is_floating_point():
                favg.append(self.buffers[n])
                flive.append(b.detach())
            else:
                self.buffers[n].copy_(b)
        self._lerp_to(favg, flive, d)
        self.last_decay = d
        return d

    # ---- state ---------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """The averaged model under the model's own ``state_dict`` keys (shared tensors stay shared)."""
        live = self.net.state_dict()
        byptr ={(t.data_ptr(), tuple(t.shape)): n for n, t in
                 list(self.net.named_parameters()) + list(self.net.named_buffers())}
        out = type(live)()
        for key, t in live.items():
            name = byptr[(t.data_ptr(), tuple(t.shape))]
            out[key] = self.params[name] if name in self.params else self.buffers[name]
        if hasattr(live, "_metadata"):
            out._metadata = live._metadata
        return out

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        mine = self.state_dict()
        if set(state) != set(mine):
            raise ValueError("EMA state: keys do not match the model's state_dict")
        for key, t in mine.items():
            if tuple(state[key].shape) != tuple(t.shape):
                raise ValueError(f"EMA state: {key} has shape {tuple(state[key].shape)}, expected {tuple(t.shape)}")
            t.copy_(state[key].to(t.device, t.dtype))

    # ---- evaluation ------------------------------------------------------------------------------------------------
    @contextmanager
    def swapped_in(self):
        """The averaged values inside the live module for the body (in-place copies: wrappers whose parameters are
        views of a flat buffer keep working), the live ones back afterwards -- restored bitwise."""
        pairs = [(p.detach(), self.params[n]) for n, p in self.net.named_parameters()]
        pairs += [(b, self.buffers[n]) for n, b in self.net.named_buffers()]
        with torch.no_grad():
            saved = [live.clone() for live, _ in pairs]
            for live, avg in pairs:
                live.copy_(avg)
        try:
            yield self.net
        finally:
            with torch.no_grad():
                for (live, _), keep in zip(pairs, saved):
                    live.copy_(keep)
