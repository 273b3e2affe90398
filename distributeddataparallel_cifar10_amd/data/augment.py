"""Training augmentation on the uint8 dataset: random crop (zero padding) followed by a horizontal flip.

torchvision's ``RandomCrop(32, padding=pad)`` + ``RandomHorizontalFlip()`` act on the uint8 image, before
``Normalize``, with fill 0, so the augmentation is exact in the uint8 domain.  It is an extension: the reference has
no augmentation.

This module is the definition; ``csrc/augment.hip`` matches it bit for bit.  The draw is pure integer arithmetic,
stateless and keyed by the sample id (uint32, wrapping)::

    fmix32(h): h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16
    k  = fmix32(id * 0x9E3779B9 + seed)
    k  = fmix32(k ^ (epoch * 0x85EBCA77))
    dx = (uint64(fmix32(k+1)) * (2*pad+1)) >> 32        # 0 .. 2*pad
    dy = (uint64(fmix32(k+2)) * (2*pad+1)) >> 32
    f  = fmix32(k+3) >> 31   (0 when the flip is off)
    out[c,y,x] = P[c, y+dy, (f ? 31-x : x) + dx]        # P: the image zero-padded by `pad` on every side

The crop comes first and the flip acts on the cropped image (torchvision's order).  `id` is the dataset row, `seed`
the run's seed, `epoch` the 1-based epoch number.  The result does not depend on rank, world size, batch size or
the position in the index list: it is identical under DDP, a resumed run redraws what the uninterrupted run drew,
and nothing of it goes into a checkpoint.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

PAD_MAX = 8
IMAGE_SHAPE = (3, 32, 32)


@dataclass(frozen=True)
class AugmentConfig:
    """Random crop with `pad` zero pixels on every side, then (``flip``) a horizontal flip with probability 1/2;
    `seed` keys the draws (``train.py`` passes the run's ``--seed``)."""
    pad: int = 4
    flip: bool = True
    seed: int = 0

    def __post_init__(self):
        _check_pad(self.pad)


def _check_pad(pad) -> int:
    if int(pad) != pad or not 0 <= int(pad) <= PAD_MAX:
        raise ValueError(f"pad must be an integer in [0, {PAD_MAX}]")
    return int(pad)


def fmix32(h: np.ndarray) -> np.ndarray:
    """MurmurHash3's 32-bit finaliser on a uint32 array (wrapping)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _ids_array(ids) -> np.ndarray:
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))


def crop_flip_params(seed: int, epoch: int, ids, pad: int = 4, flip: bool = True) -> Tuple[np.ndarray, np.ndarray,
                                                                                           np.ndarray]:
    """``(dy, dx, f)`` of every id in `ids` (int64 arrays): crop offsets in ``[0, 2*pad]`` and the flip bit."""
    pad = _check_pad(pad)
    with np.errstate(over="ignore"):
        u = (_ids_array(ids) & 0xFFFFFFFF).astype(np.uint32)
        k = fmix32(u * np.uint32(0x9E3779B9) + np.uint32(int(seed) & 0xFFFFFFFF))
        k = fmix32(k ^ np.uint32((int(epoch) * 0x85EBCA77) & 0xFFFFFFFF))
        span = np.uint64(2 * pad + 1)
        dx = (fmix32(k + np.uint32(1)).astype(np.uint64) * span) >> np.uint64(32)
        dy = (fmix32(k + np.uint32(2)).astype(np.uint64) * span) >> np.uint64(32)
        f = fmix32(k + np.uint32(3)) >> np.uint32(31) if flip else np.zeros_like(k)
    return dy.astype(np.int64), dx.astype(np.int64), f.astype(np.int64)


def _check_dataset(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or \
            tuple(t.shape[1:]) != IMAGE_SHAPE or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous uint8 tensor [N, 3, 32, 32]")


def _checked_ids(ids, n_rows: int) -> np.ndarray:
    """`ids` (None: every row) as int64, every entry inside [0, n_rows): ValueError otherwise."""
    if ids is None:
        return np.arange(n_rows, dtype=np.int64)
    idx = _ids_array(ids)
    if idx.size and (idx.min() < 0 or idx.max() >= n_rows):
        raise ValueError(f"augmentation id out of range [0, {n_rows})")
    return idx


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() and b0 < a0 + a.numel()


def augment_reference(src_u8: torch.Tensor, ids, seed: int, epoch: int, pad: int = 4, flip: bool = True,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The definition on the CPU: ``out[id] = T(src_u8[id])`` for every id in `ids` (None: every row); the other rows
    of `out` (default: a copy of `src_u8`) stay as they are.  Returns `out` (a CPU tensor unless one was given)."""
    pad = _check_pad(pad)
    _check_dataset(src_u8, "src")
    n_rows = int(src_u8.shape[0])
    idx = _checked_ids(ids, n_rows)
    if out is None:
        out = src_u8.detach().cpu().clone()
    else:
        _check_dataset(out, "out")
        if out.shape != src_u8.shape or _overlap(src_u8, out):
            raise ValueError("out must have src's shape and must not alias it")
    if idx.size == 0:
        return out
    dy, dx, f = crop_flip_params(seed, epoch, idx, pad, flip)
    src = src_u8.detach().cpu().numpy()
    padded = np.zeros((idx.size, 3, 32 + 2 * pad, 32 + 2 * pad), dtype=np.uint8)
    padded[:, :, pad:pad + 32, pad:pad + 32] = src[idx]
    ar = np.arange(32, dtype=np.int64)
    rows = (dy[:, None] + ar[None, :])[:, None, :, None]                             # [n,1,32,1]: y + dy
    cols = (np.where(f[:, None] != 0, 31 - ar[None, :], ar[None, :]) + dx[:, None])[:, None, None, :]
    res = padded[np.arange(idx.size)[:, None, None, None], np.arange(3)[None, :, None, None], rows, cols]
    out[torch.from_numpy(idx).to(out.device)] = torch.from_numpy(np.ascontiguousarray(res)).to(out.device)
    return out


def _stream_of(stream, device):
    """None -> torch's current stream; a torch stream; or a raw hipStream_t handle (``runtime/evaluate.py``)."""
    if stream is None:
        return torch.cuda.current_stream(device)
    if isinstance(stream, torch.cuda.Stream):
        return stream
    return torch.cuda.ExternalStream(int(stream), device=device)


def augment_u8(src: torch.Tensor, dst: torch.Tensor, ids=None, *, seed: int, epoch: int, pad: int = 4,
               flip: bool = True, stream=None) -> torch.Tensor:
    """``dst[ids[k]] = T(src[ids[k]])`` for the draw of ``(seed, epoch)``; the other rows of `dst` are not touched.

    `src` and `dst` are distinct contiguous uint8 ``[N, 3, 32, 32]`` tensors of one shape on one device; `ids` (a
    sequence, numpy array or tensor; None: every row) may repeat -- duplicates write identical bytes.  On the GPU this
    is one launch of ``k_augment_u8`` (``csrc/augment.hip``) on `stream` (None: torch's current stream; a torch stream;
    or a raw ``hipStream_t`` such as the engine's): a missing kernel is an error.  On the CPU it is
    ``augment_reference``.  Returns `dst`."""
    pad = _check_pad(pad)
    _check_dataset(src, "src")
    _check_dataset(dst, "dst")
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError("src and dst must have the same shape and device")
    if _overlap(src, dst):
        raise ValueError("src and dst must not alias")
    n_rows = int(src.shape[0])
    idx = None if ids is None else _checked_ids(ids, n_rows)
    if n_rows == 0 or (idx is not None and idx.size == 0):
        return dst
    if src.device.type != "cuda":
        return augment_reference(src, idx, seed, epoch, pad, flip, out=dst)
    from ..runtime import native
    lib = native.require_native()
    dev = src.device
    with torch.cuda.device(dev):
        st = _stream_of(stream, dev)
        d_ids = None
        if idx is not None:  # uploaded on torch's current stream; the allocator keeps the block until the pass has run
            d_ids = torch.from_numpy(idx.astype(np.int32)).to(dev)
            d_ids.record_stream(st)
        # whatever torch's current stream did to src, dst and the ids so far is ordered before the pass; work that
        # other streams enqueue afterwards has to wait for `stream` itself
        st.wait_stream(torch.cuda.current_stream(dev))
        rc = lib.dca_augment_u8(src.data_ptr(), dst.data_ptr(), d_ids.data_ptr() if d_ids is not None else None,
                                int(idx.size) if idx is not None else n_rows, n_rows, int(seed) & 0xFFFFFFFF,
                                int(epoch) & 0xFFFFFFFF, pad, 1 if flip else 0, ctypes.c_void_p(st.cuda_stream))
        if rc != 0:
            raise RuntimeError(lib.dca_augment_last_error().decode(errors="replace"))
    return dst
