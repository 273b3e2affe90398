"""Generic flat-bucket data parallelism for any ``nn.Module`` (the stock-op path of the framework).

Reference: ``DDP(model, device_ids=[rank], output_device=rank)`` (``main.py:63``), whose implicit behaviour is
pinned down in SURVEY.md section 2.4:
  * CC3 -- at construction rank 0's parameters and buffers are broadcast to every rank;
  * CC4 -- at every forward rank 0's buffers (BN running stats, num_batches_tracked) are broadcast
    (``broadcast_buffers=True``);
  * CC5 -- during backward, gradients are averaged over ranks bucket by bucket.

Design (not a copy of the c10d Reducer):
  * all unique parameters live in ONE flat buffer and all gradients in ONE flat gradient buffer; ``p.data`` /
    ``p.grad`` are views, so there is no bucket copy-in/copy-out and the SGD update is one fused op over the flat
    buffer (``FlatSGD``);
  * the flat layout is REVERSE registration order (approximately gradient-ready order), so every bucket is a
    contiguous slice that becomes ready as a unit;
  * a bucket's all-reduce is launched asynchronously from the gradient hook of its last parameter, so it
    overlaps the rest of the backward (RCCL runs on its own HIP stream); the backward's final callback waits
    for all buckets;
  * bucket sizes default to a cap sized for xGMI (``bucket_cap_mb``): big enough that a ring step moves well over
    64 KB per link, small enough that the first bucket fires early.  With ``first_bucket_mb`` the first (earliest
    ready) bucket can be made smaller, like DDP's 1 MiB first bucket.

  * the bucket all-reduce is either the process group's (RCCL over xGMI on GPUs, gloo on CPU) or, for CUDA
    models inside one node, the framework's own xGMI peer-read all-reduce (``parallel/xgmi.py``: one-shot for
    small buckets, two-shot reduce-scatter/all-gather for large ones, fp32 or bf16 on the wire), launched on a
    dedicated comm stream with the 1/W average fused into the kernel.  Every bucket starts on a 16-byte
    boundary (parameters are padded to 4 elements) so buckets can be handed to the kernel as they are.

The fused NetResDeep engine (``parallel/ddp.py``) implements the same semantics inside its graph-captured step;
this wrapper is the path for arbitrary models and for CPU/gloo testing.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from ..utils.checkpoint import unwrap


def _zero_flat(t: torch.Tensor) -> None:
    """Zero a flat (contiguous) gradient buffer: on a GPU one runtime fill on the current stream (no ATen kernel in
    the training step), else torch's zero_."""
    if t.is_cuda:
        from ..ops import _native as N
        N.check(N.lib().dca_ops_zero(N.ptr(t), t.numel() * t.element_size(), N.stream(t.device)), "zero")
    else:
        t.zero_()


def _dist_on(group=None) -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1


class FlatBucketDDP(nn.Module):
    def __init__(self, module: nn.Module, bucket_cap_mb: float = 4.0, first_bucket_mb: Optional[float] = 1.0,
                 broadcast_buffers: bool = True, process_group=None, device_ids=None, output_device=None,
                 comm: str = "auto", wire: str = "fp32", algo: str = "auto", loopback: bool = False):
        """``comm``: "auto" (xGMI for CUDA models when every rank is on this node, else the process group),
        "xgmi", or "process_group".  ``wire`` ("fp32" | "bf16") and ``algo`` ("auto" | "oneshot" | "twoshot")
        apply to the xGMI path.  ``loopback`` (one rank, CUDA): every bucket still goes through the xGMI
        communicator on the comm stream -- the rank is its own only peer -- so the per-bucket kernel's cost beside
        the backward is measurable on one device (``bench/resnet50.py --loopback``)."""
        super().__init__()
        if comm not in ("auto", "xgmi", "process_group"):
            raise ValueError("comm must be 'auto', 'xgmi' or 'process_group'")
        self.module = module
        self.process_group = process_group
        self.world_size = dist.get_world_size(process_group) if _dist_on(process_group) else 1
        self.broadcast_buffers = broadcast_buffers
        params = [p for _, p in module.named_parameters() if p.requires_grad]
        if not params:
            raise ValueError("module has no trainable parameters")
        dev, dtype = params[0].device, params[0].dtype
        if any(p.device != dev or p.dtype != dtype for p in params):
            raise ValueError("FlatBucketDDP needs all parameters on one device with one dtype")
        order = list(reversed(params))  # approximately gradient-ready order
        total = sum((p.numel() + 3) // 4 * 4 for p in order)  # every parameter starts 16-byte aligned
        self.flat = torch.zeros(total, dtype=dtype, device=dev)
        self.flat_grad = torch.zeros(total, dtype=dtype, device=dev)
        self._views = {}
        off = 0
        with torch.no_grad():
            for p in order:
                n = p.numel()
                self.flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + n].view_as(p)
                g = self.flat_grad[off:off + n].view_as(p)
                p.grad = g
                self._views[p] = (off, n, g)
                off += (n + 3) // 4 * 4
        # bucket plan: contiguous slices of the flat buffer
        esz = self.flat.element_size()
        cap = max(1, int(bucket_cap_mb * 2 ** 20 / esz))
        first_cap = max(1, int(first_bucket_mb * 2 ** 20 / esz)) if first_bucket_mb else cap
        self.buckets: List[tuple] = []  # (start, end, n_params)
        start, count, limit = 0, 0, first_cap
        cursor = 0
        for p in order:
            n = (p.numel() + 3) // 4 * 4
            if count and cursor + n - start > limit:
                self.buckets.append((start, cursor, count))
                start, count, limit = cursor, 0, cap
            cursor += n
            count += 1
        self.buckets.append((start, cursor, count))
        self._bucket_of = {}
        for bi, (s, e, _) in enumerate(self.buckets):
            for p in order:
                o = self._views[p][0]
                if s <= o < e:
                    self._bucket_of[p] = bi
        self._pending = [0] * len(self.buckets)
        self._ready = set()
        self._fused_opt = None  # FlatSGD(overlap=True): each bucket is updated as soon as it is reduced
        self._works: list = []
        self._callback_queued = False
        self.bucket_fire_order: List[int] = []  # for tests: order in which buckets were launched
        self._sync_next_forward = True
        self.timing = False  # True: record the comm-stream span of every step (comm_time(); metrics)
        self._comm_events: list = []
        self._flat_buffers = self._rehome_buffers(dev)
        self._sync_module_states()  # CC3
        self.comm, self.xgmi, self._comm_stream = "process_group" if self.world_size > 1 else "none", None, None
        self._wire, self._algo = wire, algo
        if loopback:
            if self.world_size != 1 or dev.type != "cuda" or dtype != torch.float32:
                raise ValueError("loopback: one rank, fp32 parameters on a GPU")
            from .xgmi import XgmiComm
            self.xgmi = XgmiComm.create(max(e - s for s, e, _ in self.buckets), group=process_group, device=dev,
                                        wire=wire)
            if self.xgmi is None:
                raise RuntimeError("xGMI loopback communicator unavailable")
            self.comm = "xgmi-loopback"
            self._comm_stream = torch.cuda.Stream(dev)
        elif self.world_size > 1 and dev.type == "cuda" and dtype == torch.float32 and comm != "process_group":
            local = int(os.environ.get("LOCAL_WORLD_SIZE", str(self.world_size)))
            if comm == "xgmi" or (local == self.world_size and self.world_size <= 8):
                from .xgmi import XgmiComm
                self.xgmi = XgmiComm.create(max(e - s for s, e, _ in self.buckets), group=process_group,
                                            device=dev, wire=wire)
                if self.xgmi is not None:
                    self.comm = "xgmi"
                    self._comm_stream = torch.cuda.Stream(dev)
        for p in order:
            p.register_post_accumulate_grad_hook(self._make_hook(p))
            # direct-write protocol (ops/functional.py grad_sink): a kernel that produces a parameter's whole
            # gradient for the step accumulates it into the flat view and reports readiness itself
            p._dca_grad_sink = (self._views[p][2], self._make_ready(p))

    # ---- collectives ------------------------------------------------------------------------------------------
    def _sync_module_states(self) -> None:
        if self.world_size == 1:
            return
        with torch.no_grad():
            dist.broadcast(self.flat, 0, group=self.process_group)
        self._broadcast_buffers_now()

    def _rehome_buffers(self, dev) -> list:
        """Module buffers (BN running mean / var, num_batches_tracked) become views of ONE flat tensor per dtype,
        like the parameters: CC4 is then one in-place broadcast per dtype -- no concatenation before it and no
        per-buffer copy after it (torch DDP coalesces into a temporary and copies back).  A buffer shared by
        several modules (NetResDeep's one ResBlock applied 10x) is re-homed once and stays shared.  Buffers on
        another device than the parameters keep their own storage (broadcast as they are)."""
        seen, groups = {}, {}
        for mod in self.module.modules():
            for name, b in mod._buffers.items():
                if b is None:
                    continue
                key = id(b)
                if key not in seen:
                    seen[key] = (b, [])
                    if b.device == dev:
                        groups.setdefault(b.dtype, []).append(key)
                seen[key][1].append((mod, name))
        flats = []
        with torch.no_grad():
            for dtype, keys in groups.items():
                total = sum(seen[k][0].numel() for k in keys)
                flat = torch.empty(total, dtype=dtype, device=dev)
                o = 0
                for k in keys:
                    b, users = seen[k]
                    n = b.numel()
                    v = flat[o:o + n].view_as(b)
                    v.copy_(b)
                    for mod, name in users:
                        mod._buffers[name] = v
                    o += n
                flats.append(flat)
        self._loose_buffers = [seen[k][0] for k in seen if seen[k][0].device != dev]
        return flats

    def _broadcast_buffers_now(self) -> None:
        if self.world_size == 1:
            return
        with torch.no_grad():
            for flat in self._flat_buffers:  # one in-place broadcast per dtype (the buffers are views of it)
                dist.broadcast(flat, 0, group=self.process_group)
            for b in self._loose_buffers:
                dist.broadcast(b, 0, group=self.process_group)

    sync_buffers = _broadcast_buffers_now  # public: rank 0's buffers now (evaluation outside a forward)

    def _make_hook(self, p):
        ready = self._make_ready(p)

        def hook(param):
            off, n, view = self._views[p]
            if param.grad is None or param.grad.data_ptr() != view.data_ptr():
                # optimizer.zero_grad(set_to_none=True) dropped the view; fold the fresh grad back in
                if param.grad is not None:
                    view.copy_(param.grad)
                param.grad = view
            ready()
        return hook

    def _make_ready(self, p):
        def ready():
            if self.world_size == 1 and self._fused_opt is None and self.xgmi is None:
                return
            # idempotent per step: a kernel-written (sink) gradient reports readiness itself, and autograd may
            # still run the parameter's AccumulateGrad with an undefined gradient, firing the hook as well
            if p in self._ready:
                return
            self._ready.add(p)
            if not self._callback_queued:
                torch.autograd.Variable._execution_engine.queue_callback(self._finish_backward)
                self._callback_queued = True
            bi = self._bucket_of[p]
            self._pending[bi] -= 1
            if self._pending[bi] == 0:
                self._launch(bi)
        return ready

    def _launch(self, bi: int) -> None:
        s, e, _ = self.buckets[bi]
        seg = self.flat_grad[s:e]
        if self.timing and seg.is_cuda and (self.world_size > 1 or self.xgmi is not None) and not self.bucket_fire_order:
            ev = torch.cuda.Event(enable_timing=True)  # first bucket of the step: comm span starts
            cs = self._side_stream()
            cs.wait_stream(torch.cuda.current_stream(seg.device))
            ev.record(cs)
            self._comm_events.append([ev, None])
        if self.world_size == 1 and self.xgmi is None:  # nothing to reduce: only the fused update (side stream on a GPU)
            if seg.is_cuda:
                cs = self._side_stream()
                cs.wait_stream(torch.cuda.current_stream(seg.device))
                with torch.cuda.stream(cs):
                    self._fused_opt._update_slice(s, e)
            else:
                self._fused_opt._update_slice(s, e)
        elif self.xgmi is not None:  # own xGMI all-reduce on the comm stream, average fused, no host sync
            cs = self._comm_stream
            cs.wait_stream(torch.cuda.current_stream(seg.device))
            self.xgmi.all_reduce_(seg, average=True, algo=self._algo, wire=self._wire, stream=cs)
            if self._fused_opt is not None:  # the bucket's SGD update right behind its all-reduce
                with torch.cuda.stream(cs):
                    self._fused_opt._update_slice(s, e)
        else:
            seg.div_(self.world_size)  # average: pre-divide, then sum
            work = dist.all_reduce(seg, group=self.process_group, async_op=True)
            if self._fused_opt is not None:
                if seg.is_cuda:  # ordered behind the collective on a side stream, overlapping the backward
                    with torch.cuda.stream(self._side_stream()):
                        work.wait()  # RCCL: a stream-level wait on the side stream, the host does not block
                        self._fused_opt._update_slice(s, e)
                    work = None
                else:
                    self._works.append((work, s, e))
                    work = None
            if work is not None:
                self._works.append((work, None, None))
        self.bucket_fire_order.append(bi)

    def _side_stream(self):
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(self.flat.device)
        return self._comm_stream

    def _finish_backward(self) -> None:
        # parameters that received no gradient this step: reduce their (zero) slices too, in bucket order
        for bi, left in enumerate(self._pending):
            if left:
                self._launch(bi)
        for w, s, e in self._works:
            w.wait()
            if s is not None:  # CPU: the fused update of a bucket after its (gloo) all-reduce
                self._fused_opt._update_slice(s, e)
        if self._comm_stream is not None:
            if self._comm_events and self._comm_events[-1][1] is None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(self._comm_stream)
                self._comm_events[-1][1] = ev
            torch.cuda.current_stream(self.flat_grad.device).wait_stream(self._comm_stream)
        self._works = []
        self._callback_queued = False
        self._reset_pending()

    def _reset_pending(self) -> None:
        self._pending = [b[2] for b in self.buckets]
        self._ready = set()

    # ---- module API -------------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        # CC4 with torch DDP's exact rule (nn/parallel/distributed.py require_forward_param_sync): a forward
        # broadcasts rank 0's buffers unless the PREVIOUS forward ran without autograd, so in an eval loop under
        # no_grad only the first batch runs a collective (a rank evaluating alone must use .module)
        if self.world_size > 1 and self.broadcast_buffers and self._sync_next_forward:
            self._broadcast_buffers_now()
        self._reset_pending()
        self.bucket_fire_order = []
        out = self.module(*args, **kwargs)
        self._sync_next_forward = torch.is_grad_enabled()
        return out

    def zero_grad(self, set_to_none: bool = False) -> None:  # grads stay views of the flat buffer
        _zero_flat(self.flat_grad)

    def comm_time(self, reset: bool = True) -> tuple:
        """(microseconds, steps) the gradient collectives spanned on the comm stream -- first bucket launched to
        backward finished -- over the timed steps since the last reset (``timing=True``; synchronises)."""
        tot, n = 0.0, 0
        for a, b in self._comm_events:
            if b is not None:
                b.synchronize()
                tot += a.elapsed_time(b) * 1e3
                n += 1
        if reset:
            self._comm_events = []
        return tot, n

    def named_views(self, buf: torch.Tensor) -> dict:
        """{parameter name: view of `buf`}, `buf` laid out like ``flat`` (a momentum buffer, an Adam moment, an
        average of the parameters); the names are the innermost module's, as in its ``state_dict``."""
        base, esz, out = self.flat.data_ptr(), self.flat.element_size(), {}
        for name, p in unwrap(self.module).named_parameters():
            off = (p.data_ptr() - base) // esz
            out[name] = buf[off:off + p.numel()].view(p.shape)
        return out

    def check_comm(self) -> None:
        """Raise if the xGMI all-reduce recorded a peer timeout (synchronous; call at log points)."""
        if self.xgmi is not None:
            self.xgmi.check()

    def close(self) -> None:
        """Release the xGMI communicator (collective: every rank must call it)."""
        if self.xgmi is not None:
            self.xgmi.close()
            self.xgmi = None


class GradAccumulator:
    """Gradient accumulation over windows of ``steps`` micro-steps for the generic engines
    (``utils/schedule.py accumulate_reference`` is the rule).  After each backward (its gradient reduced and averaged as
    usual, into buffers zeroed before it) ``accumulate()`` folds the gradient into an accumulation buffer -- the first
    micro-step of a window overwrites it -- and returns whether the window is complete; on that last micro-step the
    sum is multiplied by fp32(1 / steps) and written back into the gradient, so clipping and ``optimizer.step()`` then
    read the window's mean where they read a step's gradient.  The caller steps the optimiser only then.

    Over a ``FlatBucketDDP`` it is one buffer beside ``flat_grad``; for a plain module one buffer per parameter.  On a
    GPU contiguous fp32 gradients go through the HIP kernel (``ops/functional.py grad_accum_``); on the CPU, and for a
    plain module's gradients of another dtype or memory format, the same two torch operations.  Not with an
    ``overlap=True`` optimiser: a bucket cannot be updated before the window's last micro-step."""

    def __init__(self, model, steps: int):
        from ..utils.schedule import check_accumulate_steps
        self.steps = check_accumulate_steps(steps)
        self.model = model
        self.ddp = model if isinstance(model, FlatBucketDDP) else None
        self._check_overlap()
        self.micro = 0  # micro-steps already folded into the current window, in [0, steps)
        self._scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(self.steps), dtype=torch.float32))
        if self.ddp is not None:
            self._named = None
            self._acc = {None: torch.zeros_like(self.ddp.flat_grad)}
        else:
            self._named = {name: p for name, p in unwrap(model).named_parameters() if p.requires_grad}
            self._acc = {name: torch.zeros_like(p, memory_format=torch.preserve_format)
                         for name, p in self._named.items()}

    def _check_overlap(self) -> None:
        if self.ddp is not None and self.ddp._fused_opt is not None:
            raise ValueError("gradient accumulation cannot be combined with an overlap=True optimiser: a bucket cannot "
                             "be updated before the window's last micro-step")

    @staticmethod
    def _fold(acc: torch.Tensor, grad: torch.Tensor, first: bool, scale: Optional[float]) -> None:
        if grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous() and acc.is_contiguous():
            from ..ops.functional import grad_accum_
            grad_accum_(acc.view(-1), grad.view(-1), first, scale)
            return
        if first:
            acc.copy_(grad)
        else:
            acc.add_(grad)
        if scale is not None:
            acc.mul_(scale)
            grad.copy_(acc)

    @torch.no_grad()
    def accumulate(self) -> bool:
        """Fold the gradient of the backward just run into the window; True on the window's last micro-step (the
        gradient then holds the window's mean: clip and step now)."""
        self._check_overlap()
        first, last = self.micro == 0, self.micro == self.steps - 1
        scale = self._scale if last else None
        if self.ddp is not None:
            self._fold(self._acc[None], self.ddp.flat_grad, first, scale)
        else:
            for name, p in self._named.items():
                acc = self._acc[name]
                if p.grad is None:  # no gradient this micro-step: a zero
                    if first:
                        acc.zero_()
                    if last:
                        p.grad = acc.mul_(scale).clone()
                    continue
                self._fold(acc, p.grad, first, scale)
        self.micro = 0 if last else self.micro + 1
        return last

    def state(self) -> dict:
        """``{parameter name: accumulation buffer (a view)}`` -- the optimiser sidecar's ``"accum"``."""
        if self.ddp is not None:
            return self.ddp.named_views(self._acc[None])
        return dict(self._acc)

    @torch.no_grad()
    def load_state(self, accum: dict, micro: int) -> None:
        """Restore ``state()`` output (tensors on any device) and the window phase `micro`."""
        if not 0 <= int(micro) < self.steps:
            raise ValueError(f"micro must lie in [0, {self.steps}), got {micro}")
        for name, view in self.state().items():
            if name in accum:
                view.copy_(accum[name])
            elif micro:
                raise ValueError(f"accumulation state lacks {name}")
        self.micro = int(micro)


class _GradClip:
    """Global gradient-norm clipping of the flat gradient for ``FlatSGD`` / ``FlatAdam``
    (``torch.nn.utils.clip_grad_norm_``; ``utils/schedule.py clip_reference`` is the rule).  On a GPU the norm and the
    coefficient are formed on the device (``ops/functional.py clip_coef_``) and the update kernel multiplies the
    gradient by the coefficient, with no host synchronisation; on the CPU it is torch ops on ``flat_grad``."""

    def _init_clip(self, max_grad_norm, overlap: bool) -> None:
        if max_grad_norm is not None:
            from ..utils.schedule import check_max_norm
            max_grad_norm = check_max_norm(max_grad_norm)
            if overlap:
                raise ValueError("max_grad_norm cannot be combined with overlap=True: a bucket cannot be updated "
                                 "before the norm of all buckets is known")
        self.max_grad_norm = max_grad_norm
        self._clip_state = None   # GPU: the device state of clip_coef_
        self._last_norm = 0.0     # CPU: the last norm and the clipped steps
        self._clipped = 0

    @torch.no_grad()
    def _clip(self):
        """Before an update: GPU -> the ``gscale`` tensor of the update kernel; CPU -> ``flat_grad`` scaled in place
        (None).  None without a limit."""
        if self.max_grad_norm is None:
            return None
        grad = self.ddp.flat_grad
        if grad.is_cuda:
            from ..ops.functional import clip_coef_, clip_state
            if self._clip_state is None:
                self._clip_state = clip_state(grad.device)
            return clip_coef_(grad, self.max_grad_norm, self._clip_state)
        norm = grad.norm()
        coef = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        grad.mul_(coef)
        self._last_norm = float(norm)
        self._clipped += int(float(coef) < 1.0)
        return None

    def last_grad_norm(self) -> float:
        """The L2 norm of the last step's gradient before clipping (0.0 before the first).  GPU: synchronises."""
        if self._clip_state is not None:
            from ..ops.functional import clip_readout
            return clip_readout(self._clip_state)[0]
        return self._last_norm

    def clipped_steps(self, reset: bool = False) -> int:
        """Steps whose norm exceeded the limit since the last reset.  GPU: synchronises."""
        if self._clip_state is not None:
            from ..ops.functional import clip_readout
            return clip_readout(self._clip_state, reset)[1]
        n = self._clipped
        if reset:
            self._clipped = 0
        return n


class FlatSGD(_GradClip, torch.optim.Optimizer):
    """``optim.SGD`` over the flat buffer in one or two fused ops.

    Default = reference ``main.py:27`` (lr only).  ``momentum`` / ``weight_decay`` follow torch.optim.SGD's
    formulas (buf = m * buf + (g + wd * p); p -= lr * buf), e.g. the ppe_main_ddp.py setting SGD(1e-3, 0.9).

    ``overlap=True`` (BASELINE config 5, "fused SGD + all-reduce overlap"): every gradient bucket is updated as
    soon as it is complete -- right behind its all-reduce on the comm stream (HIP SGD kernel), or on a side
    stream with one rank -- so the update overlaps the rest of the backward; ``step()`` then has nothing left
    to do.  The momentum buffer starts at zero, so its first update equals the gradient (torch's semantics).

    ``max_grad_norm``: ``step()`` first clips the flat gradient to this global L2 norm (``_GradClip``; not with
    ``overlap``); ``last_grad_norm()`` / ``clipped_steps()`` report it."""

    def __init__(self, ddp: FlatBucketDDP, lr: float = 1e-2, momentum: float = 0.0, weight_decay: float = 0.0,
                 overlap: bool = False, max_grad_norm: Optional[float] = None):
        super().__init__(list(ddp.module.parameters()), dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._init_clip(max_grad_norm, overlap)
        self.ddp = ddp
        self._buf = None    # the flat momentum buffer; None before the first momentum step
        self._first = None  # GPU: the HIP kernel's "buffer not initialised yet" flag (an int32 on the device)
        self.overlap = overlap
        if overlap:
            if ddp._fused_opt is not None:
                raise ValueError("FlatBucketDDP already has a fused optimizer")
            if momentum:
                self._buf = torch.zeros_like(ddp.flat)
            ddp._fused_opt = self

    @torch.no_grad()
    def _update_slice(self, s: int, e: int) -> None:
        g = self.param_groups[0]
        p, grad = self.ddp.flat[s:e], self.ddp.flat_grad[s:e]
        buf = self._buf[s:e] if self._buf is not None else None
        if p.is_cuda:
            from ..ops.functional import sgd_step_
            sgd_step_(p, grad, g["lr"], g["momentum"], g["weight_decay"], buf=buf, first=None)
            return
        d = grad.add(p, alpha=g["weight_decay"]) if g["weight_decay"] else grad
        if buf is not None:
            buf.mul_(g["momentum"]).add_(d)
            d = buf
        p.add_(d, alpha=-g["lr"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self.overlap:  # already applied bucket by bucket during the backward
            return loss
        g = self.param_groups[0]
        gscale = self._clip()
        if self.ddp.flat.is_cuda:  # one HIP kernel over the flat buffer (ops/functional.py sgd_step_)
            from ..ops.functional import sgd_step_
            if g["momentum"] and self._buf is None:
                self._buf = torch.empty_like(self.ddp.flat)
                self._first = torch.ones(1, dtype=torch.int32, device=self.ddp.flat.device)
            sgd_step_(self.ddp.flat, self.ddp.flat_grad, g["lr"], g["momentum"], g["weight_decay"], buf=self._buf,
                      first=self._first, gscale=gscale)
            return loss
        grad = self.ddp.flat_grad
        if g["weight_decay"]:
            grad = grad.add(self.ddp.flat, alpha=g["weight_decay"])
        if g["momentum"]:
            if self._buf is None:
                self._buf = grad.clone()
            else:
                self._buf.mul_(g["momentum"]).add_(grad)
            grad = self._buf
        self.ddp.flat.add_(grad, alpha=-g["lr"])
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        _zero_flat(self.ddp.flat_grad)

    def sidecar_state(self) -> dict:
        """``{"momentum_buffer": {parameter name: view of the flat buffer}}`` -- the optimiser sidecar's shape; empty
        before the first momentum step."""
        return {"momentum_buffer": {} if self._buf is None else self.ddp.named_views(self._buf)}

    @torch.no_grad()
    def load_sidecar_state(self, state: dict, step: int = 0) -> None:
        """Restore ``sidecar_state()`` output (tensors on any device); an empty one leaves the optimiser as it is."""
        bufs = state["momentum_buffer"]
        if not bufs:
            return
        flat = self.ddp.flat
        self._buf = torch.zeros_like(flat)
        if flat.is_cuda:  # the buffer is initialised now
            self._first = torch.zeros(1, dtype=torch.int32, device=flat.device)
        for name, view in self.ddp.named_views(self._buf).items():
            view.copy_(bufs[name])


class FlatAdam(_GradClip, torch.optim.Optimizer):
    """``optim.AdamW`` (``decoupled=True``, the default) or ``optim.Adam`` (``False``: weight decay as an L2 term of
    the gradient) over the flat buffer, amsgrad off -- ``utils/schedule.py adam_reference`` is the rule.  On a GPU the
    update is one HIP kernel (``ops/functional.py adam_step_``) and the step counter with its bias-correction products
    lives in device memory, so a captured whole-step graph replays correctly; on the CPU it is torch ops in the order
    of torch's own implementation.  ``overlap=True``: as for ``FlatSGD``, every gradient bucket is updated as soon as
    it is reduced and ``step()`` only moves the step counter on.  ``max_grad_norm``: as for ``FlatSGD``."""

    def __init__(self, ddp: FlatBucketDDP, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled: bool = True, overlap: bool = False,
                 max_grad_norm: Optional[float] = None):
        from ..utils.schedule import check_adam
        check_adam(betas[0], betas[1], eps, weight_decay)
        self._init_clip(max_grad_norm, overlap)
        if ddp.flat.dtype != torch.float32:
            raise TypeError("FlatAdam: fp32 parameters")
        super().__init__(list(ddp.module.parameters()),
                         dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                              weight_decay=float(weight_decay)))
        self.ddp = ddp
        self.decoupled = bool(decoupled)
        self.overlap = overlap
        self.exp_avg = torch.zeros_like(ddp.flat)
        self.exp_avg_sq = torch.zeros_like(ddp.flat)
        self._t = 0  # CPU: optimiser steps taken
        self._state = None  # GPU: the device step state of adam_step_
        if ddp.flat.is_cuda:
            from ..ops.functional import adam_state
            self._state = adam_state(ddp.flat.device)
        if overlap:
            if ddp._fused_opt is not None:
                raise ValueError("FlatBucketDDP already has a fused optimizer")
            ddp._fused_opt = self

    def steps_taken(self) -> int:
        """Optimiser steps taken so far (GPU: reads the device counter, synchronises)."""
        return int(self._state[0].item()) if self._state is not None else self._t

    def set_steps_taken(self, step: int) -> None:
        """Resume: the step counter (and with it the bias corrections) as after `step` steps."""
        if self._state is not None:
            from ..ops.functional import adam_state_at
            b1, b2 = self.param_groups[0]["betas"]
            self._state.copy_(adam_state_at(step, b1, b2, self._state.device))
        self._t = int(step)

    @torch.no_grad()
    def _update_slice(self, s: int, e: int, advance: bool = False, gscale=None) -> None:
        g = self.param_groups[0]
        p, grad = self.ddp.flat[s:e], self.ddp.flat_grad[s:e]
        m, v = self.exp_avg[s:e], self.exp_avg_sq[s:e]
        (b1, b2), lr, eps, wd = g["betas"], g["lr"], g["eps"], g["weight_decay"]
        if p.is_cuda:
            from ..ops.functional import adam_step_
            adam_step_(p, grad, m, v, self._state, lr, (b1, b2), eps, wd, decoupled=self.decoupled, advance=advance,
                       gscale=gscale)
            return
        t = self._t + 1  # (the order of torch/optim/adam.py _single_tensor_adam)
        if wd:
            if self.decoupled:
                p.mul_(1 - lr * wd)
            else:
                grad = grad.add(p, alpha=wd)
        m.lerp_(grad, 1 - b1)
        v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        denom = (v.sqrt() / (1 - b2 ** t) ** 0.5).add_(eps)
        p.addcdiv_(m, denom, value=-(lr / (1 - b1 ** t)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self.overlap:  # already applied bucket by bucket during the backward: only the counter moves
            if self._state is not None:
                from ..ops.functional import adam_advance_
                adam_advance_(self._state, self.param_groups[0]["betas"])
        else:
            self._update_slice(0, self.ddp.flat.numel(), advance=True, gscale=self._clip())
        self._t += 1
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        _zero_flat(self.ddp.flat_grad)

    def sidecar_state(self) -> dict:
        """``{"kind", "exp_avg": {parameter name: view}, "exp_avg_sq": {...}}`` -- the optimiser sidecar's shape."""
        return {"kind": "adamw" if self.decoupled else "adam", "exp_avg": self.ddp.named_views(self.exp_avg),
                "exp_avg_sq": self.ddp.named_views(self.exp_avg_sq)}

    @torch.no_grad()
    def load_sidecar_state(self, state: dict, step: int = 0) -> None:
        """Restore ``sidecar_state()`` output (tensors on any device; empty moments stay as they are) and the step
        counter, with its bias corrections, as after `step` steps."""
        for key, dst in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            if state[key]:
                for name, view in self.ddp.named_views(dst).items():
                    view.copy_(state[key][name])
        self.set_steps_taken(int(step))
