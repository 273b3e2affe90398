"""Training application shared by ``main.py`` (DDP) and ``main_no_ddp.py`` (single device).

Reference: ``main.py:26-65`` (``train_loop``, ``main``) and ``main_no_ddp.py:22-63`` (``prepare``,
``training_loop``).  Defaults reproduce the reference exactly -- SGD(lr=1e-2), CrossEntropyLoss, epochs 1..99,
per-rank batch 32 with DistributedSampler order (no set_epoch), log + checkpoint at epoch 1 and every 10th epoch,
the same stdout lines -- while the step itself runs on the MI355X-native path:

* ``engine="fused"`` (default on a GPU, NetResDeep): the whole step (forward, loss, backward, gradient
  all-reduce -- one-shot xGMI peer reads or RCCL --, SGD, BN running stats) is ONE hipGraph replay of the native engine; the dataset is
  device-resident; the loss is accumulated on the device and read once per epoch (reference ``loss.item()``
  every step, SURVEY.md Q9: same printed value, no per-step host sync).
* ``engine="ops"``: the framework's general HIP layer kernels (``ops/``: MFMA GEMM convolutions, fused
  BN + ReLU + residual, fused cross-entropy, HIP SGD; fp8 forward GEMMs with ``fp8``) + ``FlatBucketDDP``.
* ``engine="torch"``: stock PyTorch ops + ``FlatBucketDDP`` (generic path; CPU / gloo; any model).

Options beyond the reference (all off by default): max_steps (per epoch), synthetic data, resume, metrics JSON,
fault injection (``fail_at_step``), process-group timeout, set_epoch reshuffling, bf16/fp32 engine precision,
momentum / weight decay / a per-step learning-rate schedule (``optimizer_active``; one table drives every engine),
``--augment`` (per-epoch random crop + flip of the training images, ``data/augment.py``), ``--ema-decay`` (an
exponential moving average of the weights, ``utils/ema.py``: kept by the fused engine's optimiser pass on the device, by
``ModelEma`` on the other engines; evaluated beside the live model and saved as ``<checkpoint>.ema.pt``),
``--optimizer adam`` / ``adamw`` (the Adam forms of the fused engine's optimiser pass, ``FlatAdam`` on ``ops``, torch's
own on ``torch`` and the CPU; ``utils/schedule.py adam_reference`` is the rule).
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn

from .data.cifar import load_cifar10
from .data.loader import DeviceLoader
from .data.synthetic import synthetic_cifar
from .utils.checkpoint import CHECKPOINT_NAME, load_checkpoint, save_checkpoint, unwrap
from .utils.metrics import MetricsLog, epoch_line, should_log, time_line


@dataclass
class TrainConfig:
    epochs: int = 99                 # range(1, 100) (reference main.py:30)
    lr: float = 1e-2                 # reference main.py:27
    batch_size: int = 32             # reference main.py:61 (main_no_ddp.py:31 hard-codes 64)
    data_path: str = "data/CIFAR-10/"
    synthetic: int = 0               # >0: use N synthetic CIFAR-shaped samples instead of the dataset
    synthetic_learnable: bool = False  # synthetic "hard" learnable set (data/synthetic.py: blended class colour,
                                       # random-phase class stripes under noise, 10 % label noise)
    engine: str = "auto"             # auto | fused | torch
    dtype: str = "fp32"              # compute precision: fp32 = the reference's numerics (default), bf16 = MFMA bf16
    max_steps: Optional[int] = None  # per-epoch step cap (smoke tests / benchmarking)
    checkpoint: bool = True
    checkpoint_path: Optional[str] = None
    resume: Optional[str] = None
    metrics_json: Optional[str] = None
    seed: int = 0
    set_epoch: bool = False
    fail_at_step: Optional[int] = None
    backend: str = "nccl"
    port: Optional[int] = None
    timeout_s: Optional[float] = None
    model: str = "netresdeep"        # netresdeep | resnet50 (generic path)
    bucket_mb: float = 4.0           # FlatBucketDDP bucket cap (generic path)
    profile: Optional[str] = None    # directory for torch.profiler traces / kernel summary
    check_sync: int = 0              # >0: assert cross-rank parameter equality every N epochs (and at start)
    allreduce: str = "auto"          # fused engine gradient all-reduce: auto | xgmi (one-shot P2P) | rccl
    fp8: bool = False                # ops engine: fp8 e4m3 forward GEMMs for 1x1 convs / fc (ResNet family)
    eval: Optional[int] = None       # None: no evaluation; 0: the whole held-out set; N: its first N images
    eval_only: bool = False          # load `resume`, evaluate, exit (no training, nothing saved)
    momentum: float = 0.0            # SGD momentum (dampening 0); with the fields below: see optimizer_active()
    weight_decay: float = 0.0        # L2 decay on every parameter tensor (torch's default grouping)
    lr_schedule: Optional[str] = None  # None (constant `lr`, no table) | constant | step | cosine
    lr_warmup_steps: int = 0         # linear warm-up over the first N optimiser steps
    lr_min: float = 0.0              # cosine: the final learning rate
    lr_step_epochs: Optional[int] = None  # step: decay every N epochs ...
    lr_gamma: float = 0.1            # ... by this factor
    augment: bool = False            # per-epoch random crop (zero padding) + horizontal flip of the training images
    augment_pad: int = 4             # crop padding, 0..8
    augment_flip: bool = True
    ema_decay: Optional[float] = None  # None: no average; D in [0, 1): EMA of the weights (see optimizer_active())
    ema_warmup: bool = False         # decay min(D, (1 + k) / (10 + k)) at optimiser step k
    optimizer: str = "sgd"           # sgd | adam (weight_decay as an L2 term) | adamw (weight_decay decoupled)
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    extra: dict = field(default_factory=dict)


def add_cli_args(ap: argparse.ArgumentParser, batch_default: int = 32) -> argparse.ArgumentParser:
    ap.add_argument("--epochs", type=int, default=99)
    ap.add_argument("--max-steps", type=int, default=None, help="cap on steps per epoch")
    ap.add_argument("--batch-size", type=int, default=batch_default)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--synthetic", type=int, nargs="?", const=50000, default=0,
                    help="train on N synthetic CIFAR-shaped samples (default 50000)")
    ap.add_argument("--synthetic-learnable", action="store_true",
                    help="synthetic data whose label is a function of the image (blended class colour + random-phase "
                         "class stripes under noise, 10%% label noise), so the loss has a learning curve; implies "
                         "--synthetic 50000 unless given")
    ap.add_argument("--engine", default="auto", choices=["auto", "fused", "ops", "torch"],
                    help="fused: NetResDeep native engine; ops: the framework's HIP layer kernels (any supported "
                         "model) + FlatBucketDDP; torch: stock PyTorch ops + FlatBucketDDP")
    ap.add_argument("--fp8", action="store_true", help="ops engine: fp8 e4m3 forward GEMMs (1x1 convs, fc)")
    ap.add_argument("--dtype", default="fp32", choices=["bf16", "fp32"],
                    help="fp32 (default): fp32-accurate, the reference's dtype (the sliced engine computes every "
                         "product as 3 bf16 MFMA products, ~2^-17 relative error; the multi-kernel engine exact fp32 "
                         "MFMA); bf16: bf16 MFMA operands, fp32 accumulation")
    ap.add_argument("--no-checkpoint", action="store_true")
    ap.add_argument("--checkpoint-path", default=None)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--metrics-json", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--set-epoch", action="store_true", help="reshuffle every epoch (reference never does)")
    ap.add_argument("--fail-at-step", type=int, default=None, help="fault injection: raise on this global step")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--world-size", type=int, default=None, help="number of ranks (default: GPU count)")
    ap.add_argument("--port", type=int, default=None)
    ap.add_argument("--timeout", type=float, default=None, help="process-group timeout in seconds")
    ap.add_argument("--model", default="netresdeep", choices=["netresdeep", "resnet50"])
    ap.add_argument("--bucket-mb", type=float, default=4.0, help="gradient bucket cap (generic DDP path)")
    ap.add_argument("--profile", default=None, metavar="DIR", help="write torch.profiler traces to DIR")
    ap.add_argument("--check-sync", type=int, default=0, metavar="N",
                    help="assert parameters are identical on all ranks at start and every N epochs")
    ap.add_argument("--allreduce", default="auto", choices=["auto", "xgmi", "rccl"],
                    help="fused engine gradient all-reduce: one-shot xGMI peer reads (auto inside a node) or RCCL")
    ap.add_argument("--eval", type=int, nargs="?", const=0, default=None, metavar="N",
                    help="after every logged epoch (1, 10, 20, ...) and the last one, print the eval-mode accuracy and "
                         "loss on held-out data: the CIFAR-10 test split (its first N images if N is given), or with "
                         "--synthetic* N (default 10000) fresh synthetic images of the same kind")
    ap.add_argument("--eval-only", action="store_true",
                    help="load --resume, evaluate as --eval does, print the result and exit without training")
    ap.add_argument("--momentum", type=float, default=0.0, help="SGD momentum (dampening 0); default 0: plain SGD")
    ap.add_argument("--weight-decay", type=float, default=0.0,
                    help="weight decay on every parameter tensor: an L2 term of the gradient (--optimizer sgd, adam) "
                         "or decoupled (adamw)")
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adam", "adamw"],
                    help="update rule: SGD (default), or torch's Adam / AdamW (amsgrad off) with --adam-beta1, "
                         "--adam-beta2, --adam-eps; --momentum belongs to sgd")
    ap.add_argument("--adam-beta1", type=float, default=0.9, help="Adam / AdamW: first-moment decay, in [0, 1)")
    ap.add_argument("--adam-beta2", type=float, default=0.999, help="Adam / AdamW: second-moment decay, in [0, 1)")
    ap.add_argument("--adam-eps", type=float, default=1e-8, help="Adam / AdamW: the denominator's epsilon, > 0")
    ap.add_argument("--lr-schedule", default=None, choices=["constant", "step", "cosine"],
                    help="per-step learning-rate schedule over epochs x steps-per-epoch steps (default: constant --lr)")
    ap.add_argument("--lr-warmup-steps", type=int, default=0, help="linear warm-up over the first N steps")
    ap.add_argument("--lr-min", type=float, default=0.0, help="cosine schedule: the final learning rate")
    ap.add_argument("--lr-step-epochs", type=int, default=None, help="step schedule: decay every N epochs")
    ap.add_argument("--lr-gamma", type=float, default=0.1, help="step schedule: decay factor")
    ap.add_argument("--augment", action="store_true",
                    help="training images only: every epoch a fresh random crop (zero padding --augment-pad) and "
                         "horizontal flip of each image, as one on-device pass over the uint8 dataset")
    ap.add_argument("--augment-pad", type=int, default=4, metavar="N", help="crop padding in pixels, 0..8 (default 4)")
    ap.add_argument("--augment-no-flip", action="store_true", help="--augment without the horizontal flip")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the parameters and BatchNorm running statistics with "
                         "decay D in [0, 1), updated after every optimiser step; --eval also reports it and every "
                         "checkpoint gets a <checkpoint>.ema.pt beside it (default: off)")
    ap.add_argument("--ema-warmup", action="store_true",
                    help="--ema-decay with the decay min(D, (1 + k) / (10 + k)) at optimiser step k")
    return ap


def config_from_args(a: argparse.Namespace, data_path_default: str) -> TrainConfig:
    learnable = bool(getattr(a, "synthetic_learnable", False))
    eval_only = bool(getattr(a, "eval_only", False))
    if eval_only and not a.resume:
        raise SystemExit("--eval-only requires --resume")
    n_eval = getattr(a, "eval", None)
    if n_eval is not None and n_eval < 0:
        raise SystemExit("--eval N: N must not be negative")
    return TrainConfig(eval=0 if eval_only and n_eval is None else n_eval, eval_only=eval_only,
                       epochs=a.epochs, lr=a.lr, batch_size=a.batch_size, data_path=a.data_root or data_path_default,
                       synthetic=a.synthetic or (50000 if learnable else 0), synthetic_learnable=learnable,
                       engine=a.engine, dtype=a.dtype, max_steps=a.max_steps,
                       checkpoint=not a.no_checkpoint, checkpoint_path=a.checkpoint_path, resume=a.resume,
                       metrics_json=a.metrics_json, seed=a.seed, set_epoch=a.set_epoch, fail_at_step=a.fail_at_step,
                       backend=a.backend, port=a.port, timeout_s=a.timeout, model=a.model, bucket_mb=a.bucket_mb,
                       profile=a.profile, check_sync=a.check_sync, allreduce=a.allreduce, fp8=a.fp8,
                       momentum=getattr(a, "momentum", 0.0), weight_decay=getattr(a, "weight_decay", 0.0),
                       lr_schedule=getattr(a, "lr_schedule", None), lr_warmup_steps=getattr(a, "lr_warmup_steps", 0),
                       lr_min=getattr(a, "lr_min", 0.0), lr_step_epochs=getattr(a, "lr_step_epochs", None),
                       lr_gamma=getattr(a, "lr_gamma", 0.1), augment=bool(getattr(a, "augment", False)),
                       augment_pad=getattr(a, "augment_pad", 4),
                       augment_flip=not getattr(a, "augment_no_flip", False),
                       ema_decay=_ema_decay_arg(getattr(a, "ema_decay", None)),
                       ema_warmup=bool(getattr(a, "ema_warmup", False)), **_optimizer_args(a))


def _optimizer_args(a: argparse.Namespace) -> dict:
    """The ``--optimizer`` / ``--adam-*`` fields of ``TrainConfig``; values no optimiser takes exit here."""
    kind = getattr(a, "optimizer", "sgd")
    out = dict(optimizer=kind, adam_beta1=getattr(a, "adam_beta1", 0.9), adam_beta2=getattr(a, "adam_beta2", 0.999),
               adam_eps=getattr(a, "adam_eps", 1e-8))
    if kind != "sgd":
        if getattr(a, "momentum", 0.0):
            raise SystemExit(f"--momentum belongs to --optimizer sgd; --optimizer {kind} takes --adam-beta1 / "
                             f"--adam-beta2")
        from .utils.schedule import check_adam
        try:
            check_adam(out["adam_beta1"], out["adam_beta2"], out["adam_eps"], getattr(a, "weight_decay", 0.0))
        except ValueError as ex:
            raise SystemExit(f"--optimizer {kind}: {ex}")
    return out


def _ema_decay_arg(decay):
    if decay is not None and not 0.0 <= decay < 1.0:
        raise SystemExit("--ema-decay must lie in [0, 1)")
    return decay


def optimizer_active(cfg: TrainConfig) -> bool:
    """Whether any optimiser option beyond the reference's SGD(lr) is on.  Off (the default): the fused engine runs
    its own fused SGD (``optimizer=None``) and the other engines build FlatSGD(model, lr) / torch.optim.SGD(lr).
    ``--ema-decay`` alone turns it on too: the fused engine keeps the average in its optimiser pass, so it then takes
    the split step form (with a constant table if no schedule is given).  So does ``--optimizer adam`` / ``adamw``:
    the Adam rule is a form of that pass."""
    return bool(cfg.momentum or cfg.weight_decay or cfg.lr_schedule is not None or cfg.lr_warmup_steps
                or cfg.ema_decay is not None or cfg.optimizer != "sgd")


def steps_per_epoch_of(cfg: TrainConfig, n_batches: int) -> int:
    return min(n_batches, cfg.max_steps) if cfg.max_steps else n_batches


def lr_table_for(cfg: TrainConfig, n_batches: int):
    """The run's learning-rate table (one value per optimiser step, epochs x steps per epoch), or None when no
    optimiser option is on.  The same table drives every engine."""
    if not optimizer_active(cfg):
        return None
    from .utils.schedule import lr_table
    spe = steps_per_epoch_of(cfg, n_batches)
    kind = cfg.lr_schedule or "constant"
    if kind == "step" and not cfg.lr_step_epochs:
        raise ValueError("--lr-schedule step needs --lr-step-epochs")
    return lr_table(kind, cfg.lr, max(cfg.epochs * spe, 1), warmup_steps=cfg.lr_warmup_steps, min_lr=cfg.lr_min,
                    step_size=cfg.lr_step_epochs * spe if cfg.lr_step_epochs else None, gamma=cfg.lr_gamma)


def engine_optimizer(cfg: TrainConfig, n_batches: int):
    """The fused engine's ``OptimizerConfig`` for `cfg` (None when no optimiser option is on)."""
    table = lr_table_for(cfg, n_batches)
    if table is None:
        return None
    from .runtime.engine import OptimizerConfig
    return OptimizerConfig(momentum=cfg.momentum, weight_decay=cfg.weight_decay, lr_table=table,
                           ema_decay=cfg.ema_decay, ema_warmup=cfg.ema_warmup, kind=cfg.optimizer,
                           betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps)


def augment_config(cfg: TrainConfig):
    """The training loader's ``AugmentConfig`` for `cfg` (None without ``--augment``); the draws are keyed by the
    run's seed.  Evaluation never augments."""
    if not cfg.augment:
        return None
    from .data.augment import PAD_MAX, AugmentConfig
    if not 0 <= cfg.augment_pad <= PAD_MAX:
        raise SystemExit(f"--augment-pad must be in [0, {PAD_MAX}]")
    return AugmentConfig(pad=cfg.augment_pad, flip=cfg.augment_flip, seed=cfg.seed)


def make_train_loader(cfg: TrainConfig, data, labels, **kw) -> DeviceLoader:
    """The training ``DeviceLoader`` of `cfg` (``--augment`` included); data that the augmentation cannot take fails
    here, at start-up."""
    aug = augment_config(cfg)
    if aug is not None and (data.dtype != torch.uint8 or tuple(data.shape[1:]) != (3, 32, 32)):
        raise SystemExit(f"--augment needs uint8 3x32x32 images; the dataset is {data.dtype} "
                         f"{'x'.join(str(d) for d in data.shape[1:])}")
    return DeviceLoader(data, labels, augment=aug, **kw)


def optim_path(checkpoint_path: str) -> str:
    return f"{checkpoint_path}.optim.pt"


def make_adam(model, cfg: TrainConfig):
    """The generic engines' optimiser of ``--optimizer adam`` / ``adamw``: ``FlatAdam`` over a ``FlatBucketDDP``'s flat
    buffer (the ``ops`` engine's HIP kernel on a GPU), else torch's own ``Adam`` / ``AdamW``."""
    from .parallel.flat_ddp import FlatAdam, FlatBucketDDP
    betas = (cfg.adam_beta1, cfg.adam_beta2)
    if isinstance(model, FlatBucketDDP):
        return FlatAdam(model, cfg.lr, betas=betas, eps=cfg.adam_eps, weight_decay=cfg.weight_decay,
                        decoupled=cfg.optimizer == "adamw")
    cls = torch.optim.AdamW if cfg.optimizer == "adamw" else torch.optim.Adam
    return cls(model.parameters(), lr=cfg.lr, betas=betas, eps=cfg.adam_eps, weight_decay=cfg.weight_decay)


def _flat_views(model, flat, buf) -> dict:
    """{parameter name: view of `buf`}, `buf` laid out like the flat parameter buffer `flat`."""
    out = {}
    for name, p in unwrap(model).named_parameters():
        off = (p.data_ptr() - flat.data_ptr()) // flat.element_size()
        out[name] = buf[off:off + p.numel()].view(p.shape)
    return out


def _state_buffers(model, optimizer, key: str) -> dict:
    """{parameter name: the optimiser's per-parameter state tensor `key`} of a torch optimiser (tensors absent before
    the first step)."""
    return {name: optimizer.state[p][key] for name, p in unwrap(model).named_parameters()
            if optimizer.state.get(p, {}).get(key) is not None}


def _momentum_buffers(model, optimizer) -> dict:
    """{parameter name: momentum buffer} of the generic engines' optimiser (tensors absent before the first step)."""
    from .parallel.flat_ddp import FlatSGD
    if isinstance(optimizer, FlatSGD):
        if optimizer._buf is None:
            return {}
        return _flat_views(model, optimizer.ddp.flat, optimizer._buf)
    return _state_buffers(model, optimizer, "momentum_buffer")


def _adam_moments(model, optimizer) -> tuple:
    """({parameter name: exp_avg}, {parameter name: exp_avg_sq}) of the generic engines' Adam optimiser."""
    from .parallel.flat_ddp import FlatAdam
    if isinstance(optimizer, FlatAdam):
        flat = optimizer.ddp.flat
        return _flat_views(model, flat, optimizer.exp_avg), _flat_views(model, flat, optimizer.exp_avg_sq)
    return _state_buffers(model, optimizer, "exp_avg"), _state_buffers(model, optimizer, "exp_avg_sq")


def save_optimizer_state(model, optimizer, path: str, rank: int, step: int, kind: str = "sgd") -> None:
    """Rank 0 writes ``<checkpoint>.optim.pt`` (atomically): ``{"step", "momentum_buffer": {name: CPU tensor}}``, or
    with `kind` ``adam`` / ``adamw`` ``{"step", "kind", "exp_avg": {...}, "exp_avg_sq": {...}}``."""
    from .parallel.ddp import FusedDDPTrainer
    if rank != 0:
        return

    def cpu(bufs):
        return {k: v.detach().to("cpu", copy=True) for k, v in bufs.items()}
    extra = {}
    if isinstance(model, FusedDDPTrainer):
        st = model.engine.optimizer_state()
        extra["engine"] = model.engine.step_state()  # the step kernels' carried BN shifts (bitwise resume)
    elif kind != "sgd":
        st = dict(zip(("exp_avg", "exp_avg_sq"), _adam_moments(model, optimizer)))
    else:
        st = {"momentum_buffer": _momentum_buffers(model, optimizer)}
    if kind != "sgd":
        state = {"step": int(step), "kind": kind, "exp_avg": cpu(st["exp_avg"]), "exp_avg_sq": cpu(st["exp_avg_sq"]),
                 **extra}
    else:
        state = {"step": int(step), "momentum_buffer": cpu(st["momentum_buffer"]), **extra}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{optim_path(path)}.tmp.{os.getpid()}"
    torch.save(state, tmp)
    os.replace(tmp, optim_path(path))


def load_optimizer_state(model, optimizer, path: str, step: int, kind: str = "sgd") -> bool:
    """Restore ``<checkpoint>.optim.pt`` if present (momentum buffers or Adam moments; the step counter <- `step`).
    A sidecar written by another optimiser kind than `kind` ends the run (one without ``"kind"`` is SGD's)."""
    from .parallel.ddp import FusedDDPTrainer
    from .parallel.flat_ddp import FlatAdam, FlatSGD
    from .runtime.engine import optimizer_state_kind
    if not os.path.exists(optim_path(path)):
        return False
    state = torch.load(optim_path(path), map_location="cpu", weights_only=True)
    theirs = optimizer_state_kind(state)
    if theirs != kind:
        raise SystemExit(f"--resume: {optim_path(path)} holds the state of --optimizer {theirs}, this run uses "
                         f"--optimizer {kind}; resume with --optimizer {theirs}, or remove the file to restart the "
                         f"optimiser state")
    if isinstance(model, FusedDDPTrainer):
        model.engine.load_optimizer_state({**{k: v for k, v in state.items() if k != "engine"}, "step": int(step)})
        if "engine" in state:
            model.engine.load_step_state(state["engine"])
        return True
    named = dict(unwrap(model).named_parameters())
    if kind != "sgd":
        m, v = state["exp_avg"], state["exp_avg_sq"]
        with torch.no_grad():
            if isinstance(optimizer, FlatAdam):
                flat = optimizer.ddp.flat
                for bufs, dst in ((m, optimizer.exp_avg), (v, optimizer.exp_avg_sq)):
                    if bufs:
                        for name, view in _flat_views(model, flat, dst).items():
                            view.copy_(bufs[name])
                optimizer.set_steps_taken(int(step))
            elif m:
                for name, p in named.items():
                    optimizer.state[p] = {"step": torch.tensor(float(step)),
                                          "exp_avg": m[name].to(p.device, p.dtype).clone(),
                                          "exp_avg_sq": v[name].to(p.device, p.dtype).clone()}
        return True
    bufs = state["momentum_buffer"]
    if not bufs:
        return True
    with torch.no_grad():
        if isinstance(optimizer, FlatSGD):
            flat = optimizer.ddp.flat
            optimizer._buf = torch.zeros_like(flat)
            if flat.is_cuda:  # the HIP kernel's "buffer not initialised yet" flag: it is now
                optimizer._first = torch.zeros(1, dtype=torch.int32, device=flat.device)
            for name, p in named.items():
                off = (p.data_ptr() - flat.data_ptr()) // flat.element_size()
                optimizer._buf[off:off + p.numel()].copy_(bufs[name].reshape(-1))
        else:
            for name, p in named.items():
                optimizer.state[p]["momentum_buffer"] = bufs[name].to(p.device, p.dtype).clone()
    return True


def load_dataset(cfg: TrainConfig):
    if cfg.synthetic:
        return synthetic_cifar(cfg.synthetic, seed=cfg.seed, learnable="hard" if cfg.synthetic_learnable else False)
    return load_cifar10(cfg.data_path, train=True)


def load_eval_dataset(cfg: TrainConfig):
    """The held-out set of ``--eval``: the real test split, or synthetic images of the training set's kind drawn with
    another seed (``cfg.seed + 1``); `cfg.eval` = N > 0 keeps the first N."""
    if cfg.synthetic:
        return synthetic_cifar(cfg.eval or 10000, seed=cfg.seed + 1,
                               learnable="hard" if cfg.synthetic_learnable else False)
    data, labels = load_cifar10(cfg.data_path, train=False)
    return (data[:cfg.eval], labels[:cfg.eval]) if cfg.eval else (data, labels)


def eval_line(epoch: int, accuracy: float, mean_loss: float) -> str:
    return "Epoch {}, Test accuracy {:.4f}, Test loss {}".format(epoch, accuracy, mean_loss)


def eval_line_ema(epoch: int, accuracy: float, mean_loss: float) -> str:
    return "Epoch {}, EMA test accuracy {:.4f}, EMA test loss {}".format(epoch, accuracy, mean_loss)


def run_eval(model, data, labels, cfg: TrainConfig, kernel: bool = False, ema=None):
    """Eval-mode result of `model` on (data, labels), sharded over the ranks of the process group (collective).
    A ``FusedDDPTrainer`` evaluates with the fused kernel on its engine's stream; `kernel`: a bare NetResDeep on a GPU,
    the same kernel with no engine; every other model (``FlatBucketDDP``, ``OpsModel``, stock ops) runs as the module in
    eval mode.  `ema`: evaluate the averaged model instead -- ``True`` for a ``FusedDDPTrainer`` (its engine's
    average, read in place), the ``ModelEma`` of any other model (swapped into the module for the call); every rank
    evaluates with rank 0's averaged running statistics, as with the live ones."""
    from .parallel.ddp import FusedDDPTrainer
    from .parallel.flat_ddp import FlatBucketDDP
    from .runtime.evaluate import evaluate_distributed, evaluate_module
    if isinstance(model, FusedDDPTrainer):
        if ema:
            from .runtime.engine import OFF_RS
            avg = model.engine.ema
            return evaluate_distributed(model.module, data, labels, bn_stats_src=(avg[OFF_RS:OFF_RS + 32],
                                                                                   avg[OFF_RS + 32:OFF_RS + 64]),
                                        evaluate=lambda d, l, i, **kw: model.engine.evaluate(d, l, i, ema=True, **kw))
        return evaluate_distributed(model.module, data, labels, evaluate=model.engine.evaluate)
    if ema is not None:
        with ema.swapped_in():
            return run_eval(model, data, labels, cfg, kernel=kernel)
    if kernel:
        return evaluate_distributed(model, data, labels, dtype=cfg.dtype)
    fwd = model.module if isinstance(model, FlatBucketDDP) else model  # an OpsModel stays wrapped: its HIP kernels
    if isinstance(model, FlatBucketDDP) and model.broadcast_buffers:
        model._broadcast_buffers_now()  # rank 0's buffers, as the wrapper's next forward would install them anyway
    return evaluate_distributed(unwrap(model), data, labels, sync_bn_stats=False,
                                evaluate=lambda d, l, i: evaluate_module(fwd, d, l, i))


def eval_only(cfg: TrainConfig, device: torch.device, rank: int = 0):
    """``--eval-only``: build the model, load ``cfg.resume``, evaluate, print; no engine, no training, nothing saved."""
    from .models.netresdeep import NetResDeep
    if not cfg.resume:
        raise ValueError("--eval-only requires --resume")
    if cfg.model == "resnet50":
        from .models.resnet50 import resnet50
        model = resnet50(num_classes=10).to(device)
    else:
        model = NetResDeep().to(device)
    load_checkpoint(model, cfg.resume, strict=True, map_location=device)
    kind = resolve_engine(cfg, device, model)
    if kind == "ops":
        from .ops.models import OpsModel
        model = OpsModel(model, fp8=cfg.fp8)
    data, labels = load_eval_dataset(cfg)
    res = run_eval(model, data, labels, cfg, kernel=kind == "fused")
    if rank == 0:
        print("Test accuracy {:.4f}, Test loss {}".format(res.accuracy, res.mean_loss), flush=True)
    return res


def eval_source(loader: DeviceLoader) -> dict:
    """``FusedDDPTrainer`` keyword for an augmenting loader: evaluate on the pristine dataset by default."""
    return {"eval_data": loader.source} if getattr(loader, "augment", None) is not None else {}


FUSED_BATCH_MAX = 64  # csrc/common.h BMAX_LIMIT: per-rank batch the fused NetResDeep engine supports


def resolve_engine(cfg: TrainConfig, device: torch.device, model: nn.Module) -> str:
    """auto: NetResDeep on the fused engine (per-rank batch <= 64), other models (ResNet family) and larger
    NetResDeep batches on the ops-layer HIP kernels, on a GPU; stock torch ops on the CPU."""
    if cfg.engine == "fused" and cfg.batch_size > FUSED_BATCH_MAX:
        raise ValueError(f"--engine fused supports --batch-size <= {FUSED_BATCH_MAX} per rank "
                         f"(got {cfg.batch_size}); use --engine ops or auto")
    if cfg.engine != "auto":
        return cfg.engine
    if device.type != "cuda":
        return "torch"
    return "fused" if _is_netresdeep(model) and cfg.batch_size <= FUSED_BATCH_MAX else "ops"


def _is_netresdeep(model: nn.Module) -> bool:
    return getattr(model, "n_chans1", None) == 32 and getattr(model, "n_blocks", None) == 10


class _Fault(RuntimeError):
    pass


def train_loop(model, train_loader: DeviceLoader, rank: int, cfg: Optional[TrainConfig] = None,
               optimizer=None) -> dict:
    """Reference ``main.py:26-49`` / ``main_no_ddp.py:36-59``.  `model` is a ``FusedDDPTrainer`` (engine path),
    a ``FlatBucketDDP`` or a plain module (torch path).  Returns a summary dict."""
    from .parallel.ddp import FusedDDPTrainer
    cfg = cfg or TrainConfig()
    mlog = MetricsLog(cfg.metrics_json, rank)
    ckpt = cfg.checkpoint_path or os.path.join(cfg.data_path, CHECKPOINT_NAME)
    fused = isinstance(model, FusedDDPTrainer)
    n_batches = len(train_loader)
    steps_per_epoch = steps_per_epoch_of(cfg, n_batches)
    table = lr_table_for(cfg, n_batches)  # None: no optimiser option on, everything below as in the reference
    start_epoch = int(cfg.extra.get("start_epoch", 1))
    global_step = int(cfg.extra.get("start_step", 0))
    history = []
    from .ops.models import OpsModel
    on_ops = isinstance(getattr(model, "module", None), OpsModel)
    if not fused:
        loss_fn = nn.CrossEntropyLoss()
        if on_ops:
            from .ops.functional import cross_entropy as loss_fn
        if optimizer is None:
            from .parallel.flat_ddp import FlatBucketDDP, FlatSGD
            if table is None:
                optimizer = FlatSGD(model, cfg.lr) if isinstance(model, FlatBucketDDP) else \
                    torch.optim.SGD(model.parameters(), lr=cfg.lr)
            elif cfg.optimizer != "sgd":
                optimizer = make_adam(model, cfg)
            else:
                optimizer = FlatSGD(model, cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay) \
                    if isinstance(model, FlatBucketDDP) else \
                    torch.optim.SGD(model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                                    weight_decay=cfg.weight_decay)
    if table is not None:
        from .utils.schedule import lr_at
        if fused and model.engine.cfg.optimizer is None:
            raise ValueError("optimiser options are on but the fused trainer was built without optimizer= "
                             "(train.engine_optimizer)")
        opt_step = int(cfg.extra.get("opt_step", global_step))
        if cfg.resume:  # momentum buffers of the run being resumed (absent file: they start at zero)
            load_optimizer_state(model, optimizer, cfg.resume, opt_step, cfg.optimizer)
        if fused and opt_step != model.engine.optimizer_step():  # the schedule position (no sidecar to restore)
            model.engine.load_optimizer_state({**model.engine.optimizer_state(), "step": opt_step})
    ema = None  # the generic engines' averager; the fused engine keeps its average in the optimiser pass
    if cfg.ema_decay is not None:
        from .utils.ema import ModelEma, ema_decay_at, load_ema_state, save_ema_state
        if fused and model.engine.ema is None:
            raise ValueError("--ema-decay is on but the fused trainer was built without it (train.engine_optimizer)")
        if not fused:
            ema = ModelEma(model, cfg.ema_decay, cfg.ema_warmup)
        if cfg.resume:  # the average of the run being resumed (absent file: it restarts from the loaded parameters)
            avg = load_ema_state(cfg.resume)
            if avg is None:
                print(f"warning: no {cfg.resume}.ema.pt: the EMA restarts from the loaded parameters", file=sys.stderr)
            elif fused:
                model.engine.load_ema_state_dict(avg)
            else:
                ema.load_state_dict(avg)
    last_lr = cfg.lr
    from contextlib import ExitStack
    from .utils.trace import trace_range as record_function  # torch.profiler + roctx ranges
    from .parallel.dist import assert_params_in_sync
    autocast = (not fused and not on_ops and cfg.dtype == "bf16" and train_loader.device.type == "cuda"
                and not _is_netresdeep(unwrap(model)))  # generic models train in bf16; NetResDeep torch path = fp32
    if cfg.check_sync:
        assert_params_in_sync(unwrap(model))
    if cfg.metrics_json and hasattr(model, "timing"):
        model.timing = True  # FlatBucketDDP: record the comm-stream span per step
    if cfg.metrics_json and fused:
        model.engine.comm_time(reset=True)
    eval_set = load_eval_dataset(cfg) if cfg.eval is not None else None
    if eval_set is not None:
        eval_set = (eval_set[0].to(train_loader.device), eval_set[1].to(train_loader.device))
    stack = ExitStack()
    prof = stack.enter_context(_profiler(cfg.profile, train_loader.device)) if cfg.profile else None
    start_time = time.time()
    for epoch in range(start_epoch, cfg.epochs + 1):
        train_loader.set_epoch(epoch)
        t0 = time.perf_counter()
        if fused:
            bs = train_loader.batch_size
            idx = train_loader.indices()[:steps_per_epoch * bs]
            if getattr(train_loader, "augment", None) is not None:
                # this epoch's crops and flips of the rows the epoch reads, on the engine's stream: after the last
                # epoch's steps and before set_indices, which stages the first batch from `data`
                train_loader.augment_epoch(idx, stream=model.engine.lib.dca_engine_stream(model.engine.h))
            if cfg.fail_at_step is not None and global_step < cfg.fail_at_step <= global_step + steps_per_epoch:
                done = cfg.fail_at_step - global_step - 1  # steps before the failing one still run, as on the
                if done:                                   # generic path (the failure is raised AT that step)
                    model.engine.run_epoch(idx[:done * bs], bs)
                raise _Fault(f"injected failure at step {cfg.fail_at_step} (rank {rank})")
            with record_function(f"epoch{epoch}:engine"):
                loss_sum, nsteps = model.engine.run_epoch(idx, bs)
        else:
            loss_sum, nsteps = 0.0, 0
            for imgs, labels in train_loader:
                if nsteps >= steps_per_epoch:
                    break
                if cfg.fail_at_step is not None and global_step + nsteps + 1 == cfg.fail_at_step:
                    raise _Fault(f"injected failure at step {cfg.fail_at_step} (rank {rank})")
                if table is not None:  # this step's learning rate (the fused engine reads the same table on the GPU)
                    last_lr = lr_at(table, opt_step + nsteps)
                    for group in optimizer.param_groups:
                        group["lr"] = last_lr
                with record_function("forward"), torch.autocast("cuda", torch.bfloat16, enabled=autocast):
                    outputs = model(imgs)
                    loss = loss_fn(outputs.float(), labels)
                optimizer.zero_grad()
                with record_function("backward+allreduce"):
                    loss.backward(_seed_grad(loss))
                with record_function("optimizer"):
                    optimizer.step()
                    if ema is not None:
                        ema.update(opt_step + nsteps)
                loss_sum += loss.item()
                nsteps += 1
        global_step += nsteps
        if table is not None:
            opt_step += nsteps
            if nsteps:
                last_lr = lr_at(table, opt_step - 1)
        dt = time.perf_counter() - t0
        if hasattr(model, "check_comm"):  # a peer timeout of the xGMI all-reduce must not go unnoticed
            model.check_comm()            # (rank-divergent gradients): raise before anything is saved
        mean = loss_sum / n_batches  # reference divides by len(train_loader) (main.py:44)
        history.append(mean)
        comm_us, comm_n = _comm_time(model) if cfg.metrics_json else (0.0, 0)
        eng = getattr(model, "engine", None)
        ev = run_eval(model, *eval_set, cfg) if eval_set is not None and (should_log(epoch) or epoch == cfg.epochs) \
            else None
        ev_rec = dict(eval_accuracy=ev.accuracy, eval_loss=ev.mean_loss, eval_images=ev.count) if ev else {}
        ema_ev = run_eval(model, *eval_set, cfg, ema=True if fused else ema) \
            if ev is not None and cfg.ema_decay is not None else None
        if ema_ev is not None:
            ev_rec.update(ema_eval_accuracy=ema_ev.accuracy, ema_eval_loss=ema_ev.mean_loss)
        mlog.write(epoch=epoch, loss=mean, steps=nsteps, seconds=dt, step_ms=1e3 * dt / max(nsteps, 1),
                   images_per_sec=nsteps * train_loader.batch_size / max(dt, 1e-9),
                   # exposed wait of the reduction kernel's gradient-segment exchanges, summed per step (xGMI)
                   allreduce_us_per_step=(comm_us / comm_n) if comm_n else None,
                   engine=getattr(eng, "kind_name", cfg.engine if not fused else None),
                   lr=last_lr,  # the learning rate of the epoch's last step
                   augment=_augment_record(train_loader),
                   # the decay of the epoch's last EMA update
                   ema_decay=ema_decay_at(opt_step - 1, cfg.ema_decay, cfg.ema_warmup)
                   if cfg.ema_decay is not None and opt_step > 0 else None,
                   dtype=cfg.dtype, fp32_mode=("3xbf16" if getattr(eng, "kind_name", "") == "sliced" else
                                               "fp32-mfma") if cfg.dtype == "fp32" and fused else None,
                   **ev_rec)
        if should_log(epoch):
            print(epoch_line(epoch, mean), flush=True)
            if cfg.checkpoint:
                meta = {"epoch": epoch, "step": global_step}
                if table is not None:  # optimiser sidecar: momentum buffers + the schedule position
                    meta["opt_step"] = opt_step
                    save_optimizer_state(model, optimizer, ckpt, rank, opt_step, cfg.optimizer)
                save_checkpoint(model, ckpt, rank, meta=meta)
                if cfg.ema_decay is not None and rank == 0:  # the averaged model, loadable like the checkpoint itself
                    save_ema_state(model.engine.ema_state_dict() if fused else ema.state_dict(), ckpt, rank)
        if ev is not None and rank == 0:
            print(eval_line(epoch, ev.accuracy, ev.mean_loss), flush=True)
            if ema_ev is not None:
                print(eval_line_ema(epoch, ema_ev.accuracy, ema_ev.mean_loss), flush=True)
        if cfg.check_sync and epoch % cfg.check_sync == 0:
            assert_params_in_sync(unwrap(model))
    total = time.time() - start_time
    stack.close()
    if prof is not None:
        _export_profile(prof, cfg.profile, rank, train_loader.device)
    print(time_line(total), flush=True)
    # end-of-run record (metrics JSON only): the BN step counter after the last epoch -- the last checkpoint is the
    # epoch-90 one (reference main.py:43-45), so the file holds an earlier count
    nbt = _num_batches_tracked(unwrap(model))
    mlog.write(final=True, steps_total=global_step, seconds_total=total, num_batches_tracked=nbt)
    return {"losses": history, "seconds": total, "steps": global_step, "num_batches_tracked": nbt}


def _augment_record(loader) -> Optional[dict]:
    a = getattr(loader, "augment", None)
    return None if a is None else {"pad": a.pad, "flip": bool(a.flip), "seed": a.seed}


def _num_batches_tracked(module) -> Optional[int]:
    for name, buf in module.named_buffers():
        if name.endswith("num_batches_tracked"):
            return int(buf.item())
    return None


_SEEDS = {}


def _seed_grad(loss: torch.Tensor) -> torch.Tensor:
    """The scalar loss's seed gradient (1.0), allocated once per device and dtype: ``loss.backward()`` would launch
    a fill kernel for it every step."""
    key = (loss.device, loss.dtype)
    if key not in _SEEDS:
        _SEEDS[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
    return _SEEDS[key]


def _comm_time(model) -> tuple:
    """(microseconds, steps) spent in the gradient all-reduce since the last call (per-rank metric)."""
    from .parallel.ddp import FusedDDPTrainer
    if isinstance(model, FusedDDPTrainer):
        return model.engine.comm_time(reset=True)
    if hasattr(model, "comm_time"):
        return model.comm_time(reset=True)
    return 0.0, 0


def _profiler(out_dir: str, device: torch.device):
    """torch.profiler over the training loop (CPU ops + HIP kernels through roctracer on ROCm)."""
    from torch.profiler import ProfilerActivity, profile
    acts = [ProfilerActivity.CPU] + ([ProfilerActivity.CUDA] if device.type == "cuda" else [])
    os.makedirs(out_dir, exist_ok=True)
    return profile(activities=acts, record_shapes=False)


def _export_profile(prof, out_dir: str, rank: int, device: torch.device) -> None:
    prof.export_chrome_trace(os.path.join(out_dir, f"trace_rank{rank}.json"))
    key = "self_cuda_time_total" if device.type == "cuda" else "self_cpu_time_total"
    with open(os.path.join(out_dir, f"summary_rank{rank}.txt"), "w") as f:
        f.write(prof.key_averages().table(sort_by=key, row_limit=40))


def build_model_for_rank(cfg: TrainConfig, rank: int, world_size: int, device: torch.device, data, labels,
                         loader: DeviceLoader):
    """The model wrapped for data parallelism on `device`: NetResDeep on the fused engine, or any model on
    FlatBucketDDP (``--model resnet50`` trains a 10-class ResNet-50 on the CIFAR tensors, channels-last, bf16)."""
    from .models.netresdeep import NetResDeep
    from .parallel.ddp import FusedDDPTrainer
    from .parallel.flat_ddp import FlatBucketDDP
    if cfg.model == "resnet50":
        from .models.resnet50 import resnet50
        torch.manual_seed(cfg.seed)
        model = resnet50(num_classes=10).to(device)
        if device.type == "cuda":
            model = model.to(memory_format=torch.channels_last)
        if cfg.engine == "fused":
            raise ValueError("the fused engine implements NetResDeep only; use --engine ops/torch/auto for resnet50")
    else:
        model = NetResDeep().to(device)
    meta = None
    if cfg.resume:
        meta = load_checkpoint(model, cfg.resume, strict=True, map_location=device)
        if meta:
            cfg.extra["start_epoch"] = int(meta.get("epoch", 0)) + 1
            cfg.extra["start_step"] = int(meta.get("step", 0))
            if "opt_step" in meta:
                cfg.extra["opt_step"] = int(meta["opt_step"])
    kind = resolve_engine(cfg, device, model)
    if kind == "ops":
        from .ops.models import OpsModel
        if device.type != "cuda":
            raise ValueError("--engine ops runs the HIP kernels: it needs a GPU")
        return FlatBucketDDP(OpsModel(model, fp8=cfg.fp8), bucket_cap_mb=cfg.bucket_mb)
    if kind == "fused":
        n_idx = len(loader) * loader.batch_size
        # loader.data: with --augment the per-epoch augmented view (fixed address); loader.source, the pristine
        # dataset, is then what engine.evaluate() reads by default
        return FusedDDPTrainer(model, loader.data, loader.labels, batch_max=loader.batch_size, lr=cfg.lr,
                               dtype=cfg.dtype, max_indices=max(n_idx, loader.batch_size), comm=cfg.allreduce,
                               optimizer=engine_optimizer(cfg, len(loader)), **eval_source(loader))
    return FlatBucketDDP(model, bucket_cap_mb=cfg.bucket_mb)

