"""ConvNeXt (Liu et al. 2022, "A ConvNet for the 2020s"): a ``patch`` x ``patch`` stride-``patch`` stem conv + LayerNorm,
four stages of blocks (depthwise 7x7 conv with bias -> LayerNorm over channels -> Linear(C, 4C) -> GELU -> Linear(4C, C)
-> per-channel layer scale -> residual add) with a LayerNorm + 2x2 stride-2 conv between stages, then global average
pool, LayerNorm and a Linear head.  LayerNorm eps 1e-6; no stochastic depth.

On the ops path (``OpsModel``) the depthwise convolutions run on csrc/ops_dwconv7.hip, the LayerNorms and the GELU on
csrc/ops_ln.hip and every Linear, the stem and the downsample convs on the MFMA GEMMs; this module's own forward is
stock torch and runs on the CPU.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as TF


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return super().forward(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class Block(nn.Module):
    def __init__(self, dim: int, layer_scale: float):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        y = self.gamma * self.pwconv2(TF.gelu(self.pwconv1(y)))
        return x + y.permute(0, 3, 1, 2)


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), num_classes: int = 1000, patch: int = 4,
                 layer_scale: float = 1e-6):
        super().__init__()
        if len(depths) != len(dims) or not dims:
            raise ValueError(f"ConvNeXt: one depth per stage width, got depths {depths} and dims {dims}")
        self.patch = patch
        self.stem = nn.Sequential(nn.Conv2d(3, dims[0], patch, stride=patch), LayerNorm2d(dims[0], eps=1e-6))
        self.downsamples = nn.ModuleList(
            nn.Sequential(LayerNorm2d(a, eps=1e-6), nn.Conv2d(a, b, 2, stride=2)) for a, b in zip(dims, dims[1:]))
        self.stages = nn.ModuleList(nn.Sequential(*[Block(d, layer_scale) for _ in range(n)])
                                    for n, d in zip(depths, dims))
        self.norm = nn.LayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Linear(dims[-1], num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stem(x)
        for i, stage in enumerate(self.stages):
            if i:
                x = self.downsamples[i - 1](x)
            x = stage(x)
        return self.head(self.norm(x.mean((2, 3))))


def convnext_tiny(num_classes: int = 1000) -> ConvNeXt:
    """ConvNeXt-T: depths (3, 3, 9, 3), widths 96 / 192 / 384 / 768; grids 56 / 28 / 14 / 7 at a 224 input, 8 / 4 / 2 / 1
    on the CIFAR tensors."""
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes)
