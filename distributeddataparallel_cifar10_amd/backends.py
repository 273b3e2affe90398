"""The two step backends of ``train.train_loop``: what differs between the fused engine and the generic engines.

``train_loop`` is the reference's loop plus logging and checkpointing; everything that depends on *how* a step runs and
on *who* holds the optimiser state and the average of the weights is behind one of two objects with the same
operations:

* ``FusedBackend`` around a ``FusedDDPTrainer``: an epoch is one ``engine.run_epoch`` call; the optimiser state, the
  learning-rate table and the EMA live in the engine's optimiser pass;
* ``GenericBackend`` around a ``FlatBucketDDP`` or a plain module, its optimiser (``FlatSGD`` / ``FlatAdam`` /
  torch's own) and, with ``--ema-decay``, a ``ModelEma``: an epoch is the reference's step loop.

Operations: ``run_epoch``, ``optimizer_state`` / ``load_optimizer_state``, ``ema_state`` / ``load_ema_state``,
``evaluate``, ``comm_time``, ``check_comm``, ``grad_norm`` (``--clip-grad-norm``); attributes ``engine_name`` and ``fp32_mode`` for the metrics records.
The optimiser state travels in the sidecar's own shape: ``{"momentum_buffer": {name: tensor}}`` or ``{"kind",
"exp_avg": {...}, "exp_avg_sq": {...}}`` (the fused engine adds ``"engine"``, the step kernels' carried state).
With ``--accumulate-steps K`` every step is a micro-step: ``micro`` is the open window's phase, ``optimizer_steps`` the
optimiser steps of the last ``run_epoch``, and the state gains ``"accum"`` and ``"accumulate_steps"``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .parallel.ddp import FusedDDPTrainer
from .parallel.flat_ddp import FlatAdam, FlatBucketDDP, FlatSGD
from .runtime.evaluate import evaluate_distributed, evaluate_module
from .train import is_netresdeep
from .utils.checkpoint import unwrap
from .utils.schedule import lr_at
from .utils.trace import trace_range as record_function  # torch.profiler + roctx ranges


class Fault(RuntimeError):
    """``--fail-at-step``: the injected failure."""


class TorchOptimizerState:
    """The sidecar form of a stock ``torch.optim.SGD`` / ``Adam`` / ``AdamW``'s state, by parameter name: the two
    operations ``FlatSGD`` and ``FlatAdam`` have themselves."""

    def __init__(self, model, optimizer):
        self.named = dict(unwrap(model).named_parameters())
        self.optimizer = optimizer

    def _buffers(self, key: str) -> dict:
        """{parameter name: the per-parameter state tensor `key`} (tensors absent before the first step)."""
        state = self.optimizer.state
        return {name: state[p][key] for name, p in self.named.items() if state.get(p, {}).get(key) is not None}

    def sidecar_state(self) -> dict:
        if "betas" not in self.optimizer.defaults:
            return {"momentum_buffer": self._buffers("momentum_buffer")}
        return {"kind": "adamw" if isinstance(self.optimizer, torch.optim.AdamW) else "adam",
                "exp_avg": self._buffers("exp_avg"), "exp_avg_sq": self._buffers("exp_avg_sq")}

    @torch.no_grad()
    def load_sidecar_state(self, state: dict, step: int = 0) -> None:
        """An empty state (written before the first step) leaves the optimiser as it is."""
        st = self.optimizer.state
        if "momentum_buffer" in state:
            for name, buf in state["momentum_buffer"].items():
                p = self.named[name]
                st[p]["momentum_buffer"] = buf.to(p.device, p.dtype).clone()
        elif state["exp_avg"]:
            for name, p in self.named.items():
                st[p] = {"step": torch.tensor(float(step)),
                         "exp_avg": state["exp_avg"][name].to(p.device, p.dtype).clone(),
                         "exp_avg_sq": state["exp_avg_sq"][name].to(p.device, p.dtype).clone()}


class _Backend:
    def __init__(self, model, cfg, rank: int, table):
        self.model, self.cfg, self.rank, self.table = model, cfg, rank, table
        self.last_lr = cfg.lr  # the learning rate of the last optimiser step taken
        # --accumulate-steps K: every K-th micro-step is followed by an optimiser step; windows carry across epochs
        self.accumulate_steps = int(getattr(cfg, "accumulate_steps", 1) or 1)
        self.micro = 0            # micro-steps in the window that is open now, in [0, K)
        self.optimizer_steps = 0  # optimiser steps taken by the last run_epoch (its micro-steps when K = 1)

    def _stepped(self, loss_sum: float, nsteps: int, opt_step: int) -> tuple:
        """`nsteps` micro-steps were run from optimiser step `opt_step` on: count the optimiser steps among them."""
        self.optimizer_steps, self.micro = divmod(self.micro + nsteps, self.accumulate_steps)
        if self.table is not None and self.optimizer_steps:
            self.last_lr = lr_at(self.table, opt_step + self.optimizer_steps - 1)
        return loss_sum, nsteps, self.last_lr

    def _fault(self) -> Fault:
        return Fault(f"injected failure at step {self.cfg.fail_at_step} (rank {self.rank})")


class FusedBackend(_Backend):
    def __init__(self, model: FusedDDPTrainer, cfg, rank: int, table):
        super().__init__(model, cfg, rank, table)
        self.engine = eng = model.engine
        if table is not None and eng.cfg.optimizer is None:
            raise ValueError("optimiser options are on but the fused trainer was built without optimizer= "
                             "(train.engine_optimizer)")
        if cfg.ema_decay is not None and eng.ema is None:
            raise ValueError("--ema-decay is on but the fused trainer was built without it (train.engine_optimizer)")
        if cfg.clip_grad_norm is not None and eng.clip_part is None:
            raise ValueError("--clip-grad-norm is on but the fused trainer was built without it "
                             "(train.engine_optimizer)")
        if self.accumulate_steps > 1 and eng.accum is None:
            raise ValueError("--accumulate-steps is on but the fused trainer was built without it "
                             "(train.engine_optimizer)")
        self.engine_name = eng.kind_name
        self.fp32_mode = ("3xbf16" if eng.kind_name == "sliced" else "fp32-mfma") if cfg.dtype == "fp32" else None
        if cfg.metrics_json:
            eng.comm_time(reset=True)

    def run_epoch(self, loader, steps: int, opt_step: int, fail_after: Optional[int] = None) -> tuple:
        """`steps` steps over the loader's order of this epoch, as one engine call (the learning rates come from the
        engine's table on the device); `fail_after`: that many steps, then the injected failure."""
        eng, bs = self.engine, loader.batch_size
        idx = loader.indices()[:steps * bs]
        if getattr(loader, "augment", None) is not None:
            # this epoch's crops and flips of the rows the epoch reads, on the engine's stream: after the last
            # epoch's steps and before set_indices, which stages the first batch from `data`
            loader.augment_epoch(idx, stream=eng.lib.dca_engine_stream(eng.h))
        if fail_after is not None:  # steps before the failing one still run, as on the generic path
            if fail_after:
                eng.run_epoch(idx[:fail_after * bs], bs)
            raise self._fault()
        with record_function(f"epoch{loader.epoch}:engine"):
            loss_sum, nsteps = eng.run_epoch(idx, bs)
        return self._stepped(loss_sum, nsteps, opt_step)

    def optimizer_state(self) -> dict:
        state = self.engine.optimizer_state()
        del state["step"]
        state.pop("micro", None)  # (the window phase travels in the checkpoint's meta, like the step)
        return {**state, "engine": self.engine.step_state()}  # the step kernels' carried BN shifts (bitwise resume)

    def load_optimizer_state(self, state: Optional[dict], step: int, micro: int = 0) -> None:
        """`state` None (no sidecar): only the schedule position moves to `step`.  `micro`: the window phase of
        ``--accumulate-steps`` (the accumulated gradient is the sidecar's ``"accum"``)."""
        eng = self.engine
        if state is None:
            if step != eng.optimizer_step():
                eng.load_optimizer_state({**eng.optimizer_state(), "step": step})
            return
        eng.load_optimizer_state({**{k: v for k, v in state.items() if k != "engine"}, "step": int(step),
                                  "micro": int(micro)})
        self.micro = int(micro)
        if "engine" in state:
            eng.load_step_state(state["engine"])

    def grad_norm(self) -> Optional[tuple]:
        """``(the last step's gradient norm before clipping, steps clipped since the last call)``, read from the device
        once per epoch with the loss; None without ``--clip-grad-norm``."""
        return self.engine.grad_norm(reset=True) if self.cfg.clip_grad_norm is not None else None

    def ema_state(self) -> dict:
        return self.engine.ema_state_dict()

    def load_ema_state(self, state: dict) -> None:
        self.engine.load_ema_state_dict(state)

    def evaluate(self, data, labels, ema: bool = False):
        return evaluate_fused(self.model, data, labels, ema)

    def comm_time(self) -> tuple:
        return self.engine.comm_time(reset=True)

    def check_comm(self) -> None:
        self.model.check_comm()


class GenericBackend(_Backend):
    def __init__(self, model, optimizer, cfg, rank: int, table):
        from .ops.models import OpsModel
        super().__init__(model, cfg, rank, table)
        self.engine_name, self.fp32_mode = cfg.engine, None
        self.optimizer = optimizer
        self.opt_state = optimizer if isinstance(optimizer, (FlatSGD, FlatAdam)) else \
            TorchOptimizerState(model, optimizer)
        # --clip-grad-norm: FlatSGD / FlatAdam clip inside step(); a stock optimiser gets torch's clip_grad_norm_
        self.clip_torch = cfg.clip_grad_norm is not None and self.opt_state is not optimizer
        if cfg.clip_grad_norm is not None and not self.clip_torch and optimizer.max_grad_norm is None:
            raise ValueError("--clip-grad-norm is on but the flat optimiser was built without max_grad_norm "
                             "(train.make_optimizer)")
        self._last_norm, self._clipped = 0.0, 0
        self.accum = None  # --accumulate-steps K > 1: the window's gradient sum beside the model's gradients
        if self.accumulate_steps > 1:
            from .parallel.flat_ddp import GradAccumulator
            self.accum = GradAccumulator(model, self.accumulate_steps)
        self.loss_fn = nn.CrossEntropyLoss()
        on_ops = isinstance(getattr(model, "module", None), OpsModel)
        if on_ops:
            from .ops.functional import cross_entropy
            self.loss_fn = cross_entropy
        # generic models train in bf16; NetResDeep torch path = fp32
        self.autocast = not on_ops and cfg.dtype == "bf16" and not is_netresdeep(unwrap(model))
        self.ema = None
        if cfg.ema_decay is not None:
            from .utils.ema import ModelEma
            self.ema = ModelEma(model, cfg.ema_decay, cfg.ema_warmup)
        if cfg.metrics_json and hasattr(model, "timing"):
            model.timing = True  # FlatBucketDDP: record the comm-stream span per step

    def run_epoch(self, loader, steps: int, opt_step: int, fail_after: Optional[int] = None) -> tuple:
        """The reference's step loop over the first `steps` batches; `fail_after`: the injected failure is raised at
        the step after that many.  With ``--accumulate-steps`` every step is a micro-step: its gradient is folded into
        the window, and only the window's last one sets the learning rate (by optimiser step), clips, steps the
        optimiser and updates the EMA."""
        model, optimizer, table, accum = self.model, self.optimizer, self.table, self.accum
        autocast = self.autocast and loader.device.type == "cuda"
        loss_sum, nsteps, nopt = 0.0, 0, 0
        for imgs, labels in loader:
            if nsteps >= steps:
                break
            if nsteps == fail_after:
                raise self._fault()
            last = accum is None or accum.micro == accum.steps - 1  # an optimiser step follows this backward
            if table is not None and last:  # its learning rate (the fused engine reads the same table on the GPU)
                lr = lr_at(table, opt_step + nopt)
                for group in optimizer.param_groups:
                    group["lr"] = lr
            with record_function("forward"), torch.autocast("cuda", torch.bfloat16, enabled=autocast):
                outputs = model(imgs)
                loss = self.loss_fn(outputs.float(), labels)
            optimizer.zero_grad()
            with record_function("backward+allreduce"):
                loss.backward(_seed_grad(loss))
            with record_function("optimizer"):
                norm = None
                if accum is not None:
                    accum.accumulate()
                if last:
                    if self.clip_torch:
                        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), self.cfg.clip_grad_norm)
                    optimizer.step()
                    if self.ema is not None:
                        self.ema.update(opt_step + nopt)
                    nopt += 1
            loss_sum += loss.item()
            if norm is not None:
                self._last_norm = float(norm)
                self._clipped += int(self.cfg.clip_grad_norm / (self._last_norm + 1e-6) < 1.0)
            nsteps += 1
        return self._stepped(loss_sum, nsteps, opt_step)

    def optimizer_state(self) -> dict:
        state = self.opt_state.sidecar_state()
        if self.accum is not None:
            state = {**state, "accum": self.accum.state(), "accumulate_steps": self.accumulate_steps}
        return state

    def load_optimizer_state(self, state: Optional[dict], step: int, micro: int = 0) -> None:
        if state is not None:
            self.opt_state.load_sidecar_state(state, step)
            if self.accum is not None:
                self.accum.load_state(state.get("accum", {}), micro)
                self.micro = int(micro)

    def grad_norm(self) -> Optional[tuple]:
        """As ``FusedBackend.grad_norm``."""
        if self.cfg.clip_grad_norm is None:
            return None
        if not self.clip_torch:
            return self.optimizer.last_grad_norm(), self.optimizer.clipped_steps(reset=True)
        out, self._clipped = (self._last_norm, self._clipped), 0
        return out

    def ema_state(self) -> dict:
        return self.ema.state_dict()

    def load_ema_state(self, state: dict) -> None:
        self.ema.load_state_dict(state)

    def evaluate(self, data, labels, ema: bool = False):
        return evaluate_generic(self.model, data, labels, self.cfg.dtype, ema=self.ema if ema else None)

    def comm_time(self) -> tuple:
        return self.model.comm_time(reset=True) if hasattr(self.model, "comm_time") else (0.0, 0)

    def check_comm(self) -> None:
        if hasattr(self.model, "check_comm"):  # a peer timeout of the xGMI all-reduce must not go unnoticed
            self.model.check_comm()


def step_backend(model, cfg, rank: int, table, optimizer, make_optimizer):
    """The backend of `model`; a generic one takes `optimizer`, or builds it with ``make_optimizer(model)``."""
    if isinstance(model, FusedDDPTrainer):
        return FusedBackend(model, cfg, rank, table)
    return GenericBackend(model, optimizer if optimizer is not None else make_optimizer(model), cfg, rank, table)


# ---- evaluation ------------------------------------------------------------------------------------------------
def evaluate_fused(trainer: FusedDDPTrainer, data, labels, ema: bool = False):
    """The fused kernel on the engine's stream; `ema`: the engine's average, read in place."""
    eng = trainer.engine
    if not ema:
        return evaluate_distributed(trainer.module, data, labels, evaluate=eng.evaluate)
    from .runtime.engine import OFF_RS
    avg = eng.ema
    return evaluate_distributed(trainer.module, data, labels,
                                bn_stats_src=(avg[OFF_RS:OFF_RS + 32], avg[OFF_RS + 32:OFF_RS + 64]),
                                evaluate=lambda d, l, i, **kw: eng.evaluate(d, l, i, ema=True, **kw))


def evaluate_generic(model, data, labels, dtype: str, kernel: bool = False, ema=None):
    """`kernel`: a bare NetResDeep on a GPU, the fused eval kernel with no engine; every other model (``FlatBucketDDP``,
    ``OpsModel``, stock ops) runs as the module in eval mode.  `ema`: a ``ModelEma``, swapped in for the call."""
    if ema is not None:
        with ema.swapped_in():
            return evaluate_generic(model, data, labels, dtype, kernel=kernel)
    if kernel:
        return evaluate_distributed(model, data, labels, dtype=dtype)
    fwd = model
    if isinstance(model, FlatBucketDDP):
        fwd = model.module  # an OpsModel stays wrapped: its HIP kernels
        if model.broadcast_buffers:  # rank 0's buffers, as the wrapper's next forward would install them anyway
            model.sync_buffers()
    return evaluate_distributed(unwrap(model), data, labels, sync_bn_stats=False,
                                evaluate=lambda d, l, i: evaluate_module(fwd, d, l, i))


def evaluate_model(model, data, labels, dtype: str, kernel: bool = False, ema=None):
    """``train.run_eval``: any model the training application handles."""
    if isinstance(model, FusedDDPTrainer):
        return evaluate_fused(model, data, labels, bool(ema))
    return evaluate_generic(model, data, labels, dtype, kernel=kernel, ema=ema)


_SEEDS = {}


def _seed_grad(loss: torch.Tensor) -> torch.Tensor:
    """The scalar loss's seed gradient (1.0), allocated once per device and dtype: ``loss.backward()`` would launch
    a fill kernel for it every step."""
    key = (loss.device, loss.dtype)
    if key not in _SEEDS:
        _SEEDS[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
    return _SEEDS[key]
