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

``train_loop`` itself is engine-blind: how an epoch's steps run and who holds the optimiser state and the averaged
weights is behind one of the two step backends of ``backends.py``.

Options beyond the reference (all off by default): max_steps (per epoch), synthetic data, resume, metrics JSON,
fault injection (``fail_at_step``), process-group timeout, set_epoch reshuffling, bf16/fp32 engine precision,
momentum / weight decay / a per-step learning-rate schedule (``optimizer_active``; one table drives every engine),
``--augment`` (per-epoch random crop + flip of the training images, ``data/augment.py``), ``--ema-decay`` (an
exponential moving average of the weights, ``utils/ema.py``: kept by the fused engine's optimiser pass on the device, by
``ModelEma`` on the other engines; evaluated beside the live model and saved as ``<checkpoint>.ema.pt``),
``--optimizer adam`` / ``adamw`` (the Adam forms of the fused engine's optimiser pass, ``FlatAdam`` on ``ops``, torch's
own on ``torch`` and the CPU; ``utils/schedule.py adam_reference`` is the rule), ``--clip-grad-norm``, and
``--accumulate-steps K`` (gradient accumulation: every K-th step is followed by one optimiser step on the mean of K
gradients -- ``k_grad_accum`` and the ACC forms of the fused engine's pass, ``GradAccumulator`` on the other engines;
``utils/schedule.py accumulate_reference`` is the rule; micro-steps and optimiser steps are counted separately).
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
from .utils.checkpoint import CHECKPOINT_NAME, load_checkpoint, save_checkpoint, save_on_rank0, unwrap
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
    clip_grad_norm: Optional[float] = None  # None: off; X > 0: clip the gradient's global L2 norm to X before each update
    accumulate_steps: int = 1        # K > 1: every K-th step is followed by one optimiser step on the mean of K gradients
    extra: dict = field(default_factory=dict)


_D = TrainConfig()  # the defaults of the flags below: stated once, in the fields above


def add_cli_args(ap: argparse.ArgumentParser, batch_default: int = 32) -> argparse.ArgumentParser:
    ap.add_argument("--epochs", type=int, default=_D.epochs)
    ap.add_argument("--max-steps", type=int, default=_D.max_steps, help="cap on steps per epoch")
    ap.add_argument("--batch-size", type=int, default=batch_default)
    ap.add_argument("--lr", type=float, default=_D.lr)
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--synthetic", type=int, nargs="?", const=50000, default=_D.synthetic,
                    help="train on N synthetic CIFAR-shaped samples (default 50000)")
    ap.add_argument("--synthetic-learnable", action="store_true",
                    help="synthetic data whose label is a function of the image (blended class colour + random-phase "
                         "class stripes under noise, 10%% label noise), so the loss has a learning curve; implies "
                         "--synthetic 50000 unless given")
    ap.add_argument("--engine", default=_D.engine, choices=["auto", "fused", "ops", "torch"],
                    help="fused: NetResDeep native engine; ops: the framework's HIP layer kernels (any supported "
                         "model) + FlatBucketDDP; torch: stock PyTorch ops + FlatBucketDDP")
    ap.add_argument("--fp8", action="store_true", help="ops engine: fp8 e4m3 forward GEMMs (1x1 convs, fc)")
    ap.add_argument("--dtype", default=_D.dtype, choices=["bf16", "fp32"],
                    help="fp32 (default): fp32-accurate, the reference's dtype (the sliced engine computes every "
                         "product as 3 bf16 MFMA products, ~2^-17 relative error; the multi-kernel engine exact fp32 "
                         "MFMA); bf16: bf16 MFMA operands, fp32 accumulation")
    ap.add_argument("--no-checkpoint", action="store_true")
    ap.add_argument("--checkpoint-path", default=_D.checkpoint_path)
    ap.add_argument("--resume", default=_D.resume)
    ap.add_argument("--metrics-json", default=_D.metrics_json)
    ap.add_argument("--seed", type=int, default=_D.seed)
    ap.add_argument("--set-epoch", action="store_true", help="reshuffle every epoch (reference never does)")
    ap.add_argument("--fail-at-step", type=int, default=_D.fail_at_step,
                    help="fault injection: raise on this global step")
    ap.add_argument("--backend", default=_D.backend, choices=["nccl", "gloo"])
    ap.add_argument("--world-size", type=int, default=None, help="number of ranks (default: GPU count)")
    ap.add_argument("--port", type=int, default=_D.port)
    ap.add_argument("--timeout", type=float, default=_D.timeout_s, help="process-group timeout in seconds")
    ap.add_argument("--model", default=_D.model, choices=["netresdeep", "resnet50"])
    ap.add_argument("--bucket-mb", type=float, default=_D.bucket_mb, help="gradient bucket cap (generic DDP path)")
    ap.add_argument("--profile", default=_D.profile, metavar="DIR", help="write torch.profiler traces to DIR")
    ap.add_argument("--check-sync", type=int, default=_D.check_sync, metavar="N",
                    help="assert parameters are identical on all ranks at start and every N epochs")
    ap.add_argument("--allreduce", default=_D.allreduce, choices=["auto", "xgmi", "rccl"],
                    help="fused engine gradient all-reduce: one-shot xGMI peer reads (auto inside a node) or RCCL")
    ap.add_argument("--eval", type=int, nargs="?", const=0, default=_D.eval, metavar="N",
                    help="after every logged epoch (1, 10, 20, ...) and the last one, print the eval-mode accuracy and "
                         "loss on held-out data: the CIFAR-10 test split (its first N images if N is given), or with "
                         "--synthetic* N (default 10000) fresh synthetic images of the same kind")
    ap.add_argument("--eval-only", action="store_true",
                    help="load --resume, evaluate as --eval does, print the result and exit without training")
    ap.add_argument("--momentum", type=float, default=_D.momentum,
                    help="SGD momentum (dampening 0); default 0: plain SGD")
    ap.add_argument("--weight-decay", type=float, default=_D.weight_decay,
                    help="weight decay on every parameter tensor: an L2 term of the gradient (--optimizer sgd, adam) "
                         "or decoupled (adamw)")
    ap.add_argument("--optimizer", default=_D.optimizer, choices=["sgd", "adam", "adamw"],
                    help="update rule: SGD (default), or torch's Adam / AdamW (amsgrad off) with --adam-beta1, "
                         "--adam-beta2, --adam-eps; --momentum belongs to sgd")
    ap.add_argument("--adam-beta1", type=float, default=_D.adam_beta1,
                    help="Adam / AdamW: first-moment decay, in [0, 1)")
    ap.add_argument("--adam-beta2", type=float, default=_D.adam_beta2,
                    help="Adam / AdamW: second-moment decay, in [0, 1)")
    ap.add_argument("--adam-eps", type=float, default=_D.adam_eps, help="Adam / AdamW: the denominator's epsilon, > 0")
    ap.add_argument("--clip-grad-norm", type=float, default=_D.clip_grad_norm, metavar="X",
                    help="before every optimiser step, scale the (averaged) gradient so that its global L2 norm is at "
                         "most X > 0, as torch.nn.utils.clip_grad_norm_; the metrics record the norm and the number of "
                         "clipped steps (default: off)")
    ap.add_argument("--accumulate-steps", type=int, default=_D.accumulate_steps, metavar="K",
                    help="gradient accumulation: every step is a micro-step, and every K-th is followed by one optimiser "
                         "step on the mean of the K gradients (effective batch K x --batch-size per rank); schedules, "
                         "--lr-warmup-steps and the EMA count optimiser steps; micro-steps left over at the end of the "
                         "run are dropped (default 1: off)")
    ap.add_argument("--lr-schedule", default=_D.lr_schedule, choices=["constant", "step", "cosine"],
                    help="per-step learning-rate schedule over epochs x steps-per-epoch steps (default: constant --lr)")
    ap.add_argument("--lr-warmup-steps", type=int, default=_D.lr_warmup_steps,
                    help="linear warm-up over the first N steps")
    ap.add_argument("--lr-min", type=float, default=_D.lr_min, help="cosine schedule: the final learning rate")
    ap.add_argument("--lr-step-epochs", type=int, default=_D.lr_step_epochs,
                    help="step schedule: decay every N epochs")
    ap.add_argument("--lr-gamma", type=float, default=_D.lr_gamma, help="step schedule: decay factor")
    ap.add_argument("--augment", action="store_true",
                    help="training images only: every epoch a fresh random crop (zero padding --augment-pad) and "
                         "horizontal flip of each image, as one on-device pass over the uint8 dataset")
    ap.add_argument("--augment-pad", type=int, default=_D.augment_pad, metavar="N",
                    help="crop padding in pixels, 0..8 (default 4)")
    ap.add_argument("--augment-no-flip", action="store_true", help="--augment without the horizontal flip")
    ap.add_argument("--ema-decay", type=float, default=_D.ema_decay, metavar="D",
                    help="keep an exponential moving average of the parameters and BatchNorm running statistics with "
                         "decay D in [0, 1), updated after every optimiser step; --eval also reports it and every "
                         "checkpoint gets a <checkpoint>.ema.pt beside it (default: off)")
    ap.add_argument("--ema-warmup", action="store_true",
                    help="--ema-decay with the decay min(D, (1 + k) / (10 + k)) at optimiser step k")
    return ap


# flag (its argparse dest) -> TrainConfig field, where the two differ; every other flag sets the field of its own name
_RENAMED = {"data_root": "data_path", "timeout": "timeout_s"}
_NEGATED = {"no_checkpoint": "checkpoint", "augment_no_flip": "augment_flip"}


def config_from_args(a: argparse.Namespace, data_path_default: str) -> TrainConfig:
    """The run's ``TrainConfig``; a field whose flag the namespace lacks keeps its default.  Values no run can take
    exit here."""
    fields = TrainConfig.__dataclass_fields__
    kw = {}
    for dest, value in vars(a).items():
        if dest in _NEGATED:
            kw[_NEGATED[dest]] = not value
        elif _RENAMED.get(dest, dest) in fields:
            kw[_RENAMED.get(dest, dest)] = value
    kw["data_path"] = kw.get("data_path") or data_path_default
    cfg = TrainConfig(**kw)
    if cfg.synthetic_learnable and not cfg.synthetic:
        cfg.synthetic = 50000
    if cfg.eval_only and not cfg.resume:
        raise SystemExit("--eval-only requires --resume")
    if cfg.eval is not None and cfg.eval < 0:
        raise SystemExit("--eval N: N must not be negative")
    if cfg.eval_only and cfg.eval is None:
        cfg.eval = 0
    if cfg.ema_decay is not None and not 0.0 <= cfg.ema_decay < 1.0:
        raise SystemExit("--ema-decay must lie in [0, 1)")
    if cfg.clip_grad_norm is not None and not cfg.clip_grad_norm > 0.0:
        raise SystemExit("--clip-grad-norm must be positive")
    if isinstance(cfg.accumulate_steps, bool) or not isinstance(cfg.accumulate_steps, int) or cfg.accumulate_steps < 1:
        raise SystemExit("--accumulate-steps must be an integer >= 1")
    if cfg.optimizer != "sgd":  # values no Adam takes
        if cfg.momentum:
            raise SystemExit(f"--momentum belongs to --optimizer sgd; --optimizer {cfg.optimizer} takes --adam-beta1 / "
                             f"--adam-beta2")
        from .utils.schedule import check_adam
        try:
            check_adam(cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay)
        except ValueError as ex:
            raise SystemExit(f"--optimizer {cfg.optimizer}: {ex}")
    return cfg


def optimizer_active(cfg: TrainConfig) -> bool:
    """Whether any optimiser option beyond the reference's SGD(lr) is on.  Off (the default): the fused engine runs
    its own fused SGD (``optimizer=None``) and the other engines build FlatSGD(model, lr) / torch.optim.SGD(lr).
    ``--ema-decay`` alone turns it on too: the fused engine keeps the average in its optimiser pass, so it then takes
    the split step form (with a constant table if no schedule is given).  So does ``--optimizer adam`` / ``adamw``:
    the Adam rule is a form of that pass.  And so does ``--clip-grad-norm``: the norm needs the whole reduced gradient
    before any of it is applied, which is the split form plus one more kernel in front of the pass.  And so does
    ``--accumulate-steps K`` with K > 1: the accumulation is one more stage in front of that pass (K = 1 is off in
    every respect)."""
    return bool(cfg.momentum or cfg.weight_decay or cfg.lr_schedule is not None or cfg.lr_warmup_steps
                or cfg.ema_decay is not None or cfg.optimizer != "sgd" or cfg.clip_grad_norm is not None
                or cfg.accumulate_steps > 1)


def steps_per_epoch_of(cfg: TrainConfig, n_batches: int) -> int:
    return min(n_batches, cfg.max_steps) if cfg.max_steps else n_batches


def lr_table_for(cfg: TrainConfig, n_batches: int):
    """The run's learning-rate table (one value per optimiser step: epochs x steps per epoch, with
    ``--accumulate-steps K`` that many // K, windows being counted over the whole run), or None when no optimiser option
    is on.  The same table drives every engine.  ``--lr-warmup-steps`` counts optimiser steps; ``--lr-step-epochs E``
    is E x steps per epoch // K of them."""
    if not optimizer_active(cfg):
        return None
    from .utils.schedule import lr_table
    spe = steps_per_epoch_of(cfg, n_batches)
    kind = cfg.lr_schedule or "constant"
    if kind == "step" and not cfg.lr_step_epochs:
        raise ValueError("--lr-schedule step needs --lr-step-epochs")
    k = cfg.accumulate_steps
    return lr_table(kind, cfg.lr, max(cfg.epochs * spe // k, 1), warmup_steps=cfg.lr_warmup_steps, min_lr=cfg.lr_min,
                    step_size=cfg.lr_step_epochs * spe // k if cfg.lr_step_epochs else None, gamma=cfg.lr_gamma)


def engine_optimizer(cfg: TrainConfig, n_batches: int):
    """The fused engine's ``OptimizerConfig`` for `cfg` (None when no optimiser option is on)."""
    table = lr_table_for(cfg, n_batches)
    if table is None:
        return None
    from .runtime.engine import OptimizerConfig
    # (accumulate_steps is passed only when set: the default call stays what it was)
    extra = dict(accumulate_steps=cfg.accumulate_steps) if cfg.accumulate_steps > 1 else {}
    return OptimizerConfig(momentum=cfg.momentum, weight_decay=cfg.weight_decay, lr_table=table,
                           ema_decay=cfg.ema_decay, ema_warmup=cfg.ema_warmup, kind=cfg.optimizer,
                           betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps,
                           max_grad_norm=cfg.clip_grad_norm, **extra)


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
                        decoupled=cfg.optimizer == "adamw", max_grad_norm=cfg.clip_grad_norm)
    cls = torch.optim.AdamW if cfg.optimizer == "adamw" else torch.optim.Adam
    return cls(model.parameters(), lr=cfg.lr, betas=betas, eps=cfg.adam_eps, weight_decay=cfg.weight_decay)


def make_optimizer(model, cfg: TrainConfig, table):
    """The generic engines' optimiser: ``FlatSGD`` / ``FlatAdam`` over a ``FlatBucketDDP``, torch's own for a plain
    module.  No optimiser option on (`table` None): the reference's SGD(lr), built with nothing else."""
    from .parallel import flat_ddp  # (the classes are looked up when called: tests spy on them)
    flat = isinstance(model, flat_ddp.FlatBucketDDP)
    if table is None:
        return flat_ddp.FlatSGD(model, cfg.lr) if flat else torch.optim.SGD(model.parameters(), lr=cfg.lr)
    if cfg.optimizer != "sgd":
        return make_adam(model, cfg)
    args = dict(momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    if flat:
        if cfg.clip_grad_norm is not None:  # (passed only when set: the default call stays what it was)
            args["max_grad_norm"] = cfg.clip_grad_norm
        return flat_ddp.FlatSGD(model, cfg.lr, **args)
    return torch.optim.SGD(model.parameters(), lr=cfg.lr, **args)


# the sidecar's {parameter name: tensor} entries ("accum": --accumulate-steps, the open window's gradient sum)
_STATE_TENSORS = ("momentum_buffer", "exp_avg", "exp_avg_sq", "accum")


def save_optimizer_state(backend, path: str, rank: int, step: int) -> None:
    """Rank 0 writes ``<checkpoint>.optim.pt`` (atomically): ``{"step", "momentum_buffer": {name: CPU tensor}}``, or
    with ``--optimizer adam`` / ``adamw`` ``{"step", "kind", "exp_avg": {...}, "exp_avg_sq": {...}}``; the fused
    engine adds ``"engine"``, its step kernels' carried state.  With ``--accumulate-steps K`` also ``"accum"`` (the
    open window's accumulated gradient, by name) and ``"accumulate_steps"``."""
    if rank != 0:
        return
    state = {"step": int(step)}
    for key, value in backend.optimizer_state().items():
        state[key] = {k: v.detach().to("cpu", copy=True) for k, v in value.items()} if key in _STATE_TENSORS else value
    save_on_rank0(state, optim_path(path))


def load_optimizer_state(backend, path: str, step: int, kind: str = "sgd", accumulate_steps: int = 1,
                         micro: int = 0) -> bool:
    """Restore ``<checkpoint>.optim.pt`` if present (momentum buffers or Adam moments; the step counter <- `step`).
    A sidecar written by another optimiser kind than `kind` ends the run (one without ``"kind"`` is SGD's), and so does
    one written with another ``--accumulate-steps`` than `accumulate_steps` (one without the entry: 1).  `micro`: the
    window phase the checkpoint was written in; the accumulated gradient is the sidecar's ``"accum"``."""
    from .runtime.engine import optimizer_state_kind
    if not os.path.exists(optim_path(path)):
        backend.load_optimizer_state(None, step)
        return False
    state = torch.load(optim_path(path), map_location="cpu", weights_only=True)
    theirs = optimizer_state_kind(state)
    if theirs != kind:
        raise SystemExit(f"--resume: {optim_path(path)} holds the state of --optimizer {theirs}, this run uses "
                         f"--optimizer {kind}; resume with --optimizer {theirs}, or remove the file to restart the "
                         f"optimiser state")
    theirs_k = int(state.get("accumulate_steps", 1))
    if theirs_k != accumulate_steps:
        raise SystemExit(f"--resume: {optim_path(path)} was written with --accumulate-steps {theirs_k}, this run uses "
                         f"--accumulate-steps {accumulate_steps}; resume with --accumulate-steps {theirs_k}, or remove "
                         f"the file to restart the optimiser state")
    if accumulate_steps > 1:
        backend.load_optimizer_state(state, step, micro)
    else:
        backend.load_optimizer_state(state, step)
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
    from .backends import evaluate_model
    return evaluate_model(model, data, labels, cfg.dtype, kernel=kernel, ema=ema)


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
    return "fused" if is_netresdeep(model) and cfg.batch_size <= FUSED_BATCH_MAX else "ops"


def is_netresdeep(model: nn.Module) -> bool:
    return getattr(model, "n_chans1", None) == 32 and getattr(model, "n_blocks", None) == 10


def train_loop(model, train_loader: DeviceLoader, rank: int, cfg: Optional[TrainConfig] = None,
               optimizer=None) -> dict:
    """Reference ``main.py:26-49`` / ``main_no_ddp.py:36-59``.  `model` is a ``FusedDDPTrainer`` (engine path),
    a ``FlatBucketDDP`` or a plain module (torch path).  Returns a summary dict."""
    from contextlib import ExitStack
    from .backends import step_backend
    from .parallel.dist import assert_params_in_sync
    from .utils.ema import ema_decay_at, load_ema_state, save_ema_state
    cfg = cfg or TrainConfig()
    mlog = MetricsLog(cfg.metrics_json, rank)
    ckpt = cfg.checkpoint_path or os.path.join(cfg.data_path, CHECKPOINT_NAME)
    n_batches = len(train_loader)
    steps_per_epoch = steps_per_epoch_of(cfg, n_batches)
    table = lr_table_for(cfg, n_batches)  # None: no optimiser option on, everything below as in the reference
    start_epoch = int(cfg.extra.get("start_epoch", 1))
    global_step = int(cfg.extra.get("start_step", 0))
    opt_step = int(cfg.extra.get("opt_step", global_step))
    history = []
    backend = step_backend(model, cfg, rank, table, optimizer, lambda m: make_optimizer(m, cfg, table))
    if table is not None:
        if cfg.resume:  # momentum buffers of the run being resumed (absent file: they start at zero)
            load_optimizer_state(backend, cfg.resume, opt_step, cfg.optimizer, cfg.accumulate_steps,
                                 int(cfg.extra.get("accum_micro", 0)))
        else:
            backend.load_optimizer_state(None, opt_step)  # only the schedule position
    if cfg.ema_decay is not None and cfg.resume:
        avg = load_ema_state(cfg.resume)  # the average of the run being resumed
        if avg is None:  # absent file: it restarts from the loaded parameters
            print(f"warning: no {cfg.resume}.ema.pt: the EMA restarts from the loaded parameters", file=sys.stderr)
        else:
            backend.load_ema_state(avg)
    if cfg.check_sync:
        assert_params_in_sync(unwrap(model))
    eval_set = load_eval_dataset(cfg) if cfg.eval is not None else None
    if eval_set is not None:
        eval_set = (eval_set[0].to(train_loader.device), eval_set[1].to(train_loader.device))
    stack = ExitStack()
    prof = stack.enter_context(_profiler(cfg.profile, train_loader.device)) if cfg.profile else None
    start_time = time.time()
    for epoch in range(start_epoch, cfg.epochs + 1):
        train_loader.set_epoch(epoch)
        t0 = time.perf_counter()
        fail_after = None  # --fail-at-step inside this epoch: the steps before the failing one still run
        if cfg.fail_at_step is not None and global_step < cfg.fail_at_step <= global_step + steps_per_epoch:
            fail_after = cfg.fail_at_step - global_step - 1
        loss_sum, nsteps, last_lr = backend.run_epoch(train_loader, steps_per_epoch, opt_step, fail_after)
        global_step += nsteps
        if table is not None:
            opt_step += backend.optimizer_steps  # (the epoch's steps, unless --accumulate-steps groups them)
        dt = time.perf_counter() - t0
        backend.check_comm()  # a peer timeout (rank-divergent gradients): raise before anything is saved
        mean = loss_sum / n_batches  # reference divides by len(train_loader) (main.py:44)
        history.append(mean)
        comm_us, comm_n = backend.comm_time() if cfg.metrics_json else (0.0, 0)
        clip = backend.grad_norm()  # --clip-grad-norm: (the last step's norm, the epoch's clipped steps), else None
        ev = ema_ev = None
        ev_rec = {}
        if eval_set is not None and (should_log(epoch) or epoch == cfg.epochs):
            ev = backend.evaluate(*eval_set)
            ev_rec = dict(eval_accuracy=ev.accuracy, eval_loss=ev.mean_loss, eval_images=ev.count)
            if cfg.ema_decay is not None:
                ema_ev = backend.evaluate(*eval_set, ema=True)
                ev_rec.update(ema_eval_accuracy=ema_ev.accuracy, ema_eval_loss=ema_ev.mean_loss)
        mlog.write(epoch=epoch, loss=mean, steps=nsteps, seconds=dt, step_ms=1e3 * dt / max(nsteps, 1),
                   images_per_sec=nsteps * train_loader.batch_size / max(dt, 1e-9),
                   # exposed wait of the reduction kernel's gradient-segment exchanges, summed per step (xGMI)
                   allreduce_us_per_step=(comm_us / comm_n) if comm_n else None,
                   engine=backend.engine_name,
                   lr=last_lr,  # the learning rate of the last optimiser step taken
                   # --accumulate-steps: K (null when off) and the optimiser steps among this epoch's steps
                   accumulate_steps=cfg.accumulate_steps if cfg.accumulate_steps > 1 else None,
                   optimizer_steps=backend.optimizer_steps if table is not None else nsteps,
                   augment=_augment_record(train_loader),
                   # the decay of the epoch's last EMA update
                   ema_decay=ema_decay_at(opt_step - 1, cfg.ema_decay, cfg.ema_warmup)
                   if cfg.ema_decay is not None and opt_step > 0 else None,
                   # the last step's gradient norm before clipping, the epoch's clipped steps, the limit
                   grad_norm=clip[0] if clip else None, clipped_steps=clip[1] if clip else None,
                   clip_grad_norm=cfg.clip_grad_norm,
                   dtype=cfg.dtype, fp32_mode=backend.fp32_mode, **ev_rec)
        if should_log(epoch):
            print(epoch_line(epoch, mean), flush=True)
            if cfg.checkpoint:
                meta = {"epoch": epoch, "step": global_step}
                if table is not None:  # optimiser sidecar: momentum buffers + the schedule position
                    meta["opt_step"] = opt_step
                    if cfg.accumulate_steps > 1:  # the window phase; the window's sum is in the sidecar
                        meta["accum_micro"] = backend.micro
                    save_optimizer_state(backend, ckpt, rank, opt_step)
                save_checkpoint(model, ckpt, rank, meta=meta)
                if cfg.ema_decay is not None and rank == 0:  # the averaged model, loadable like the checkpoint itself
                    save_ema_state(backend.ema_state(), ckpt, rank)
        if ev is not None and rank == 0:
            print(eval_line(epoch, ev.accuracy, ev.mean_loss), flush=True)
            if ema_ev is not None:
                print(eval_line_ema(epoch, ema_ev.accuracy, ema_ev.mean_loss), flush=True)
        if cfg.check_sync and epoch % cfg.check_sync == 0:
            assert_params_in_sync(unwrap(model))
    if cfg.accumulate_steps > 1 and backend.micro:
        print(f"--accumulate-steps {cfg.accumulate_steps}: the run ends in mid-window, the last {backend.micro} "
              f"micro-step(s) are dropped (no optimiser step follows them)", file=sys.stderr, flush=True)
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
            if "accum_micro" in meta:
                cfg.extra["accum_micro"] = int(meta["accum_micro"])
    return wrap_model(cfg, model, loader, device)


def wrap_model(cfg: TrainConfig, model: nn.Module, loader: DeviceLoader, device: torch.device,
               full_device: bool = False):
    """`model` as ``train_loop`` takes it, by ``resolve_engine``: a ``FusedDDPTrainer``, a ``FlatBucketDDP`` around an
    ``OpsModel``, or for stock torch ops a ``FlatBucketDDP`` around the module.  `full_device`: one process on a
    dedicated device (``main_no_ddp.py``) -- the fused engine may take every CU, and stock torch ops need no wrapper:
    the plain module."""
    from .parallel.ddp import FusedDDPTrainer
    from .parallel.flat_ddp import FlatBucketDDP
    kind = resolve_engine(cfg, device, model)
    if kind == "ops":  # the ops-layer HIP kernels (flat parameters, packed weights, HIP SGD)
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
                               full_device=full_device, optimizer=engine_optimizer(cfg, len(loader)),
                               **eval_source(loader))
    return model if full_device else FlatBucketDDP(model, bucket_cap_mb=cfg.bucket_mb)
