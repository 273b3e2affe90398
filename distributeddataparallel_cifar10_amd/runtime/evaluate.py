"""Eval-mode NetResDeep: test accuracy and loss of a model, a checkpoint or a running engine.

On a GPU model ``evaluate_netresdeep`` runs the fused forward-only kernel (``csrc/netresdeep_eval.hip``: one
workgroup per image, BatchNorm as the fixed affine of its running statistics, operands built from the fp32 master
tensors, per-image ``pred`` / ``loss`` arrays and no device-side sum); on a CPU model it runs ``model.eval()`` with
stock PyTorch ops.  Either way the per-image arrays are reduced with torch (loss in float64), so the result does not
depend on the grid or on the chunking, and a call costs one host synchronisation.

``eval_shard`` / ``evaluate_distributed`` split an evaluation over the ranks of ``torch.distributed`` without
padding, so every image is counted exactly once.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from ..utils.checkpoint import unwrap
from ..utils.oracle import normalize_u8

CPU_CHUNK = 1000  # images per forward of the CPU path


class _DcaEvalArgs(ctypes.Structure):  # csrc/engine.hip DcaEvalArgs, field by field
    _fields_ = [(n, ctypes.c_void_p) for n in ("conv1_w", "conv1_b", "conv_w", "bn_w", "bn_b", "bn_rm", "bn_rv",
                                               "fc1_w", "fc1_b", "fc2_w", "fc2_b")] + [
        ("bn_eps", ctypes.c_float),
        ("data", ctypes.c_void_p),
        ("labels", ctypes.c_void_p),
        ("n_data", ctypes.c_int),
        ("indices", ctypes.c_void_p),
        ("n", ctypes.c_int),
        ("bf16", ctypes.c_int),
        ("max_workgroups", ctypes.c_int),
        ("logits", ctypes.c_void_p),
        ("pred", ctypes.c_void_p),
        ("loss", ctypes.c_void_p),
    ]


@dataclass
class EvalResult:
    correct: int
    count: int
    loss_sum: float
    accuracy: float
    mean_loss: float
    pred: Optional[torch.Tensor] = None    # [count] predicted class per evaluated image (this rank's, if sharded)
    logits: Optional[torch.Tensor] = None  # [count, 10] fp32 (return_logits=True)
    loss: Optional[torch.Tensor] = None    # [count] fp32 cross-entropy per evaluated image


def _result(correct: int, count: int, loss_sum: float, pred=None, logits=None, loss=None) -> EvalResult:
    return EvalResult(int(correct), int(count), float(loss_sum), correct / count if count else float("nan"),
                      loss_sum / count if count else float("nan"), pred, logits, loss)


def _checked_indices(indices, n_data: int) -> np.ndarray:
    """`indices` (None: the whole dataset) as int32, every entry inside [0, n_data): ValueError otherwise, before
    anything is launched."""
    if indices is None:
        return np.arange(n_data, dtype=np.int32)
    if isinstance(indices, torch.Tensor):
        indices = indices.detach().cpu().numpy()
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if idx.size and (idx.min() < 0 or idx.max() >= n_data):
        raise ValueError(f"evaluation index out of range [0, {n_data})")
    return idx.astype(np.int32)


def _stream_of(stream, device):
    """None -> torch's current stream; a torch stream; or a raw hipStream_t handle (e.g. ``dca_engine_stream``)."""
    if stream is None:
        return torch.cuda.current_stream(device)
    if isinstance(stream, torch.cuda.Stream):
        return stream
    return torch.cuda.ExternalStream(int(stream), device=device)


def evaluate_netresdeep(model, data_u8: torch.Tensor, labels: torch.Tensor, indices=None, dtype: str = "fp32",
                        return_logits: bool = False, max_workgroups: int = 0, stream=None,
                        bn_stats=None, params=None) -> EvalResult:
    """Evaluate NetResDeep `model` in eval mode (BatchNorm running statistics) on ``data_u8[indices]``.

    `dtype` selects the kernel's precision on a GPU model ("bf16": bf16 conv operands and fc1 weight; "fp32":
    3xbf16 conv, fp32 elsewhere); the CPU path is plain fp32.  `max_workgroups` caps the grid (0: the whole device);
    the result does not depend on it.  `bn_stats` = (running_mean, running_var) replaces the module's own running
    statistics for this call (``evaluate_distributed``: rank 0's); `params` = {parameter name: tensor}, all nine of
    ``named_parameters()``, replaces the module's parameters in the same way (an averaged copy, ``utils/ema.py``).
    Nothing of the model is modified: parameters, buffers and training flags are as before."""
    if dtype not in ("bf16", "fp32"):
        raise ValueError("dtype must be 'bf16' or 'fp32'")
    net = unwrap(model)
    if getattr(net, "n_chans1", None) != 32 or getattr(net, "n_blocks", None) != 10:
        raise ValueError("evaluate_netresdeep is specialised for NetResDeep(n_chans1=32, n_blocks=10)")
    if data_u8.dtype != torch.uint8 or data_u8.dim() != 4 or tuple(data_u8.shape[1:]) != (3, 32, 32):
        raise ValueError("data must be uint8 [N, 3, 32, 32]")
    n_data = int(data_u8.shape[0])
    if labels.numel() != n_data:
        raise ValueError("one label per image")
    idx = _checked_indices(indices, n_data)
    if idx.size == 0:
        raise ValueError("nothing to evaluate")
    dev = net.fc1.weight.device
    if params is not None:
        named = dict(net.named_parameters())
        if set(params) != set(named):
            raise ValueError(f"params must cover exactly {sorted(named)}")
        for name, p in named.items():
            if tuple(params[name].shape) != tuple(p.shape):
                raise ValueError(f"params[{name!r}] has shape {tuple(params[name].shape)}, expected {tuple(p.shape)}")
    if dev.type != "cuda":
        return _evaluate_cpu(net, data_u8, labels, idx, return_logits, bn_stats, params)
    return _evaluate_gpu(net, data_u8, labels, idx, dtype, return_logits, int(max_workgroups), stream, dev, bn_stats,
                         params)


def _evaluate_cpu(net, data_u8, labels, idx, return_logits, bn_stats, params=None) -> EvalResult:
    flags = [(m, m.training) for m in net.modules()]
    bn = net.resblocks[0].batch_norm
    own = (bn.running_mean, bn.running_var)
    own_p = [(p, p.data) for _, p in net.named_parameters()] if params is not None else []
    data_u8, labels = data_u8.cpu(), labels.cpu().long()
    sel = torch.from_numpy(idx.astype(np.int64))
    outs = []
    try:
        net.eval()
        if bn_stats is not None:
            bn.running_mean, bn.running_var = (t.to(own[0].device, torch.float32) for t in bn_stats)
        if params is not None:
            for name, p in net.named_parameters():
                p.data = params[name].detach().to(p.device, p.dtype)
        with torch.no_grad():
            for s in range(0, len(sel), CPU_CHUNK):
                outs.append(net(normalize_u8(data_u8.index_select(0, sel[s:s + CPU_CHUNK]))).float())
    finally:
        bn.running_mean, bn.running_var = own
        for p, was in own_p:
            p.data = was
        for m, was in flags:
            m.training = was
    logits = torch.cat(outs)
    want = labels.index_select(0, sel)
    pred = logits.argmax(1).to(torch.int32)
    loss = F.cross_entropy(logits, want, reduction="none")
    return _result(int((pred == want).sum()), len(sel), float(loss.double().sum()), pred,
                   logits if return_logits else None, loss)


def _evaluate_gpu(net, data_u8, labels, idx, dtype, return_logits, max_workgroups, stream, dev, bn_stats,
                  params=None) -> EvalResult:
    from . import native
    lib = native.require_native()
    bn = net.resblocks[0].batch_norm
    st = _stream_of(stream, dev)
    # inputs made on torch's current stream (uploads, casts) are ordered before the kernel on `st`; the outputs are
    # allocated, written and reduced on `st`, and the one host copy at the end waits for all of it
    with torch.cuda.device(dev):
        par = params if params is not None else dict(net.named_parameters())
        tensors = [par["conv1.weight"], par["conv1.bias"], par["resblocks.0.conv.weight"],
                   par["resblocks.0.batch_norm.weight"], par["resblocks.0.batch_norm.bias"],
                   *(bn_stats or (bn.running_mean, bn.running_var)), par["fc1.weight"], par["fc1.bias"],
                   par["fc2.weight"], par["fc2.bias"]]
        shapes = [(32, 3, 3, 3), (32,), (32, 32, 3, 3), (32,), (32,), (32,), (32,), (32, 2048), (32,), (10, 32), (10,)]
        held = []
        for t, shape in zip(tensors, shapes):
            if tuple(t.shape) != shape:
                raise ValueError(f"NetResDeep tensor of shape {tuple(t.shape)}, expected {shape}")
            held.append(t.detach().to(device=dev, dtype=torch.float32).contiguous())
        data = data_u8.to(dev).contiguous()
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        didx = torch.from_numpy(idx).to(dev)
        n = int(idx.size)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            pred = torch.empty(n, dtype=torch.int32, device=dev)
            loss = torch.empty(n, dtype=torch.float32, device=dev)
            logits = torch.empty(n, 10, dtype=torch.float32, device=dev) if return_logits else None
            args = _DcaEvalArgs(*[t.data_ptr() for t in held], float(bn.eps), data.data_ptr(), lab.data_ptr(),
                                int(data.shape[0]), didx.data_ptr(), n, 1 if dtype == "bf16" else 0, max_workgroups,
                                logits.data_ptr() if logits is not None else None, pred.data_ptr(), loss.data_ptr())
            native.check(lib.dca_eval_netresdeep(ctypes.byref(args), ctypes.c_void_p(st.cuda_stream)),
                         "dca_eval_netresdeep")
            want = lab.index_select(0, didx.long())
            sums = torch.stack([(pred == want).sum().double(), loss.double().sum()]).cpu()  # the one host sync
    return _result(int(sums[0]), n, float(sums[1]), pred, logits, loss)


def evaluate_module(module, data_u8: torch.Tensor, labels: torch.Tensor, indices=None, batch: int = CPU_CHUNK) -> EvalResult:
    """Any classifier module (stock torch ops, or an ``ops.OpsModel``) in eval mode under ``no_grad``, `batch` images
    per forward, on the device of its parameters; the training flags are restored.  One host sync."""
    from ..data.cifar import normalize_u8 as loader_normalize
    dev = next(module.parameters()).device
    idx = torch.from_numpy(_checked_indices(indices, int(data_u8.shape[0])).astype(np.int64)).to(dev)
    if idx.numel() == 0:
        raise ValueError("nothing to evaluate")
    data_u8, labels = data_u8.to(dev), labels.to(device=dev, dtype=torch.int64)
    flags = [(m, m.training) for m in module.modules()]
    correct = torch.zeros((), dtype=torch.float64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    preds = []
    try:
        module.eval()
        with torch.no_grad():
            for s in range(0, idx.numel(), batch):
                sel = idx[s:s + batch]
                logits = module(loader_normalize(data_u8.index_select(0, sel))).float()
                want = labels.index_select(0, sel)
                preds.append(logits.argmax(1).to(torch.int32))
                correct += (preds[-1] == want).sum()
                loss_sum += F.cross_entropy(logits, want, reduction="none").double().sum()
    finally:
        for m, was in flags:
            m.training = was
    sums = torch.stack([correct, loss_sum]).cpu()
    return _result(int(sums[0]), int(idx.numel()), float(sums[1]), torch.cat(preds))


def eval_shard(n: int, world_size: int, rank: int) -> np.ndarray:
    """This rank's share of ``range(n)``: every world_size-th index from `rank`, no padding (the shares partition
    ``range(n)``; they differ in length by at most one and may be empty)."""
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError("need 0 <= rank < world_size")
    return np.arange(n, dtype=np.int64)[rank::world_size]


def evaluate_distributed(model, data_u8: torch.Tensor, labels: torch.Tensor, indices=None, evaluate=None,
                         sync_bn_stats: bool = True, bn_stats_src=None, **kw) -> EvalResult:
    """Evaluate this rank's shard and all-reduce (correct, count, loss_sum) over ``torch.distributed`` (SUM; one
    process without a process group evaluates everything).  Collective: every rank calls it with the same
    `indices`.  `evaluate` replaces ``evaluate_netresdeep`` (e.g. an engine's bound ``evaluate``, which takes the
    data first); `pred` / `logits` of the result are this rank's shard.

    Between two steps the ranks' BatchNorm running statistics differ (DDP broadcasts rank 0's at the next forward,
    and rank 0's are what a checkpoint holds), so with `sync_bn_stats` every rank evaluates with a copy of rank 0's
    (``bn_stats=``; the modules' own buffers are not touched): the result is that of rank 0's model on all images.
    `bn_stats_src`: this rank's (running_mean, running_var) to take in place of the module's -- averaged statistics
    (``utils/ema.py``), which differ between the ranks just as the live ones do."""
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    ws, rank = (dist.get_world_size(), dist.get_rank()) if on else (1, 0)
    net = unwrap(model)
    cpu_group = on and dist.get_backend() == "gloo"
    if on and ws > 1 and sync_bn_stats:
        bn = net.resblocks[0].batch_norm
        src = bn_stats_src if bn_stats_src is not None else (bn.running_mean, bn.running_var)
        stats = torch.cat([src[0].detach().float().reshape(-1), src[1].detach().float().reshape(-1)])
        stats = stats.cpu() if cpu_group else stats.clone()
        dist.broadcast(stats, 0)
        stats = stats.to(bn.running_mean.device)
        kw["bn_stats"] = (stats[:32].contiguous(), stats[32:].contiguous())
    n_data = int(data_u8.shape[0])
    full = _checked_indices(indices, n_data)
    mine = full[eval_shard(len(full), ws, rank)]
    res = None
    if len(mine):
        res = evaluate(data_u8, labels, mine, **kw) if evaluate is not None else \
            evaluate_netresdeep(model, data_u8, labels, mine, **kw)
    sums = torch.tensor([res.correct, res.count, res.loss_sum] if res else [0.0, 0.0, 0.0], dtype=torch.float64)
    if on and ws > 1:
        if not cpu_group:
            sums = sums.to(next(net.parameters()).device)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        sums = sums.cpu()
    return _result(int(round(float(sums[0]))), int(round(float(sums[1]))), float(sums[2]),
                   res.pred if res else None, res.logits if res else None, res.loss if res else None)
