"""Per-step learning-rate tables and the float64 oracle of the engine's optimiser pass (pure Python / numpy).

``lr_table`` returns one learning rate per optimiser step.  The same table drives every engine: the fused engine reads
it on the device (``csrc/optimizer.hip``: ``lr_table[min(step, n - 1)]``), the ``ops`` and ``torch`` engines set
``param_groups[...]["lr"]`` from it before each step.

Schedules (``s`` = step index, ``W`` = warm-up steps, ``T`` = total steps, ``t = s - W``):

* warm-up (every kind, ``s < W``): ``base_lr * (s + 1) / (W + 1)`` -- torch ``LambdaLR`` with that factor, i.e. a
  linear ramp that reaches ``base_lr`` exactly at step ``W``;
* ``constant``: ``base_lr``;
* ``step``: ``base_lr * gamma ** (t // step_size)`` -- torch ``StepLR``;
* ``cosine``: ``min_lr + (base_lr - min_lr) * (1 + cos(pi * t / (T - W))) / 2`` -- torch ``CosineAnnealingLR``
  (closed form) with ``T_max = T - W``, ``eta_min = min_lr``.

This is torch's ``SequentialLR([LambdaLR, <main>], milestones=[W])``.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

KINDS = ("constant", "step", "cosine")


def lr_table(kind: str, base_lr: float, total_steps: int, warmup_steps: int = 0, min_lr: float = 0.0,
             step_size: Optional[int] = None, gamma: float = 0.1) -> np.ndarray:
    """float64 [total_steps]: the learning rate of every optimiser step."""
    if kind not in KINDS:
        raise ValueError(f"lr schedule must be one of {KINDS}, got {kind!r}")
    total, warm = int(total_steps), int(warmup_steps)
    if total < 1:
        raise ValueError("total_steps must be positive")
    if warm < 0:
        raise ValueError("warmup_steps must not be negative")
    if kind == "step" and (step_size is None or int(step_size) < 1):
        raise ValueError("the step schedule needs step_size >= 1")
    span = max(total - warm, 1)
    out = np.empty(total, dtype=np.float64)
    for s in range(total):
        if s < warm:
            out[s] = base_lr * (s + 1) / (warm + 1)
            continue
        t = s - warm
        if kind == "constant":
            out[s] = base_lr
        elif kind == "step":
            out[s] = base_lr * gamma ** (t // int(step_size))
        else:
            out[s] = min_lr + (base_lr - min_lr) * (1.0 + math.cos(math.pi * t / span)) / 2.0
    return out


def lr_at(table, step: int) -> float:
    """The table's value at `step`; past its end the last entry holds (as on the device)."""
    return float(table[min(max(int(step), 0), len(table) - 1)])


def sgd_reference(p, g, buf, lr: float, mu: float, wd: float, inv_ws: float = 1.0):
    """One update of SGD with momentum and weight decay (dampening 0) in float64 -- the oracle of ``k_apply_opt``:

        d = g * inv_ws + wd * p;  buf' = mu * buf + d;  p' = p - lr * buf'

    `buf` starts at zero, so the first update equals ``d`` (torch initialises its buffer to ``d``: the same).  Takes
    arrays or tensors; returns ``(p', buf')`` as float64 numpy arrays."""
    p64, g64, b64 = (_f64(x) for x in (p, g, buf))
    d = g64 * float(inv_ws) + float(wd) * p64
    nb = float(mu) * b64 + d
    return p64 - float(lr) * nb, nb


ADAM_KINDS = ("adam", "adamw")


def check_adam(beta1: float, beta2: float, eps: float, wd: float = 0.0) -> None:
    """The value ranges of the Adam rule (the ones every layer enforces): ValueError outside them."""
    if not (0.0 <= float(beta1) < 1.0) or not (0.0 <= float(beta2) < 1.0):
        raise ValueError(f"Adam betas must lie in [0, 1), got ({beta1}, {beta2})")
    if not (float(eps) > 0.0) or not math.isfinite(float(eps)):
        raise ValueError(f"Adam eps must be positive, got {eps}")
    if not (float(wd) >= 0.0):
        raise ValueError(f"weight decay must not be negative, got {wd}")


def adam_reference(p, g, m, v, t: int, lr: float, beta1: float, beta2: float, eps: float, wd: float,
                   decoupled: bool, inv_ws: float = 1.0):
    """One update of Adam (``decoupled=False``: weight decay as an L2 term of the gradient) or AdamW (``True``: decay
    applied to the parameter) in float64 -- torch ``optim.Adam`` / ``AdamW`` with ``amsgrad=False``, the oracle of the
    Adam forms of ``k_apply_opt`` and of ``k_adam``.  `t` is the 1-based step:

        g' = g * inv_ws  (+ wd * p: Adam);   p0 = p * (1 - lr * wd)  (AdamW; else p)
        m' = m + (1 - beta1) * (g' - m);     v' = beta2 * v + (1 - beta2) * g' * g'
        p' = p0 - (lr / (1 - beta1^t)) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

    `m` and `v` start at zero.  Takes arrays or tensors; returns ``(p', m', v')`` as float64 numpy arrays."""
    check_adam(beta1, beta2, eps, wd)
    t = int(t)
    if t < 1:
        raise ValueError("the Adam step t is 1-based")
    p64, g64, m64, v64 = (_f64(x) for x in (p, g, m, v))
    b1, b2, lr, wd = float(beta1), float(beta2), float(lr), float(wd)
    gg = g64 * float(inv_ws)
    if decoupled:
        p0 = p64 * (1.0 - lr * wd)
    else:
        gg = gg + wd * p64
        p0 = p64
    nm = m64 + (1.0 - b1) * (gg - m64)
    nv = b2 * v64 + (1.0 - b2) * gg * gg
    denom = np.sqrt(nv) / math.sqrt(1.0 - b2 ** t) + float(eps)
    return p0 - (lr / (1.0 - b1 ** t)) * nm / denom, nm, nv


def check_max_norm(max_norm) -> float:
    """The limit of gradient-norm clipping as a float: ValueError unless it is positive (a NaN is not)."""
    try:
        v = float(max_norm)
    except (TypeError, ValueError):
        raise ValueError(f"the gradient-norm limit must be a positive number, got {max_norm!r}") from None
    if not v > 0.0:
        raise ValueError(f"the gradient-norm limit must be positive, got {max_norm!r}")
    return v


def clip_reference(grads, max_norm: float, inv_ws: float = 1.0):
    """Global gradient-norm clipping in float64 -- ``torch.nn.utils.clip_grad_norm_`` (L2, ``error_if_nonfinite``
    off), the oracle of ``k_grad_sqnorm`` + the CLIP forms of the optimiser pass, of ``k_sqnorm_part`` + ``k_clip_coef``
    and of the flat optimisers' CPU path.  `grads`: one array / tensor or a sequence of them (the summed gradients):

        x = g * inv_ws  (rounded to fp32 where g is fp32: the averaged gradient as the kernels form it)
        N = sqrt(sum x * x)  in float64;   c = fp32(max_norm / (N + 1e-6))
        coef = c if c < 1 else (c if c != c else 1)      (torch's clamp(max=1): a NaN stays a NaN)

    Returns ``(N, coef)``: a Python float and a ``numpy.float32``; the clipped averaged gradient is ``x * coef`` (one
    more fp32 rounding on the device), and that is what ``sgd_reference`` / ``adam_reference`` then receive."""
    max_norm = check_max_norm(max_norm)
    if hasattr(grads, "detach") or isinstance(grads, np.ndarray):
        grads = [grads]
    total = 0.0
    for g in grads:
        is32 = (hasattr(g, "detach") and str(g.dtype) == "torch.float32") or getattr(g, "dtype", None) == np.float32
        x = _f64(g).reshape(-1) * float(inv_ws)
        if is32:
            with np.errstate(over="ignore", invalid="ignore"):
                x = x.astype(np.float32).astype(np.float64)
        total += float(np.sum(x * x))
    norm = math.sqrt(total) if total == total else float("nan")
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.float32(np.float64(max_norm) / (np.float64(norm) + 1e-6))
    coef = c if c < np.float32(1.0) else (c if c != c else np.float32(1.0))
    return norm, np.float32(coef)


def check_accumulate_steps(k) -> int:
    """The number of micro-steps per optimiser step as an int: ValueError unless it is an integer >= 1 (a bool, a
    float with a fraction, a NaN are not)."""
    bad = isinstance(k, bool)
    try:
        v = int(k)
        bad = bad or v != k
    except (TypeError, ValueError, OverflowError):
        bad = True
    if bad or v < 1:
        raise ValueError(f"accumulate steps must be an integer >= 1, got {k!r}")
    return v


def accumulate_reference(grads, K: int):
    """Gradient accumulation over a window of `K` micro-steps -- the oracle of ``k_grad_accum`` (both the engine's and
    the flat one) and of ``GradAccumulator``'s CPU path.  `grads`: the K summed gradients g_1 .. g_K of the window, in
    order (arrays or tensors of one shape).  Per element in fp32:

        acc = g_1;   acc = acc + g_k  (k = 2 .. K, in order);   G = acc * fp32(1 / K)   (rounded on its own)

    The first micro-step overwrites, so nothing that was in the buffer before takes part.  Returns ``(G32, G64)``: the
    exact fp32 emulation (``numpy.float32``: what the kernels hold, bit for bit) and the same mean in float64 without
    intermediate rounding.  G32 is what ``clip_reference`` / ``sgd_reference`` / ``adam_reference`` then receive in the
    gradient's place (``g * inv_ws`` follows as for a single step)."""
    K = check_accumulate_steps(K)
    grads = list(grads)
    if len(grads) != K:
        raise ValueError(f"a window of K={K} micro-steps needs {K} gradients, got {len(grads)}")
    g32 = [_f64(g).astype(np.float32) if not (isinstance(g, np.ndarray) and g.dtype == np.float32) else g
           for g in grads]
    with np.errstate(over="ignore", invalid="ignore"):
        acc = g32[0].copy()
        for g in g32[1:]:
            acc = (acc + g).astype(np.float32)
        inv_k = np.float32(1.0) / np.float32(K)
        G32 = (acc * inv_k).astype(np.float32)
        G64 = sum(g.astype(np.float64) for g in g32) / float(K)
    return G32, G64


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)
