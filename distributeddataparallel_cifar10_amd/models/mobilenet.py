"""MobileNetV1 (Howard et al. 2017, "MobileNets: Efficient Convolutional Neural Networks for Mobile Vision
Applications", table 1): a 3x3/2 stem to 32 channels, 13 depthwise-separable blocks (depthwise 3x3 + BN + ReLU, then
1x1 + BN + ReLU) of widths 64, 128, 128, 256, 256, 512 x 6, 1024, 1024 with stride 2 at the 2nd, 4th, 6th and 12th,
global average pool, fc.  Plain ReLU (the BN kernels of the ops layer fuse ReLU and nothing else).  ``width_mult``
scales every width, rounded to a multiple of 8 (the depthwise kernels' channel chunk).

On the ops path (``OpsModel``) the depthwise convolutions run on csrc/ops_dwconv.hip, everything else on the kernels
the ResNets use.
"""
from __future__ import annotations

import torch
import torch.nn as nn

#        width, stride of the 13 blocks
BLOCKS = [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2)] + [(512, 1)] * 5 + [(1024, 2), (1024, 1)]


def _width(ch: int, mult: float) -> int:
    return max(8, int(ch * mult + 4) // 8 * 8)


class DepthwiseSeparable(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, stride: int):
        super().__init__()
        self.dw = nn.Conv2d(in_ch, in_ch, 3, stride=stride, padding=1, groups=in_ch, bias=False)
        self.bn1 = nn.BatchNorm2d(in_ch)
        self.pw = nn.Conv2d(in_ch, out_ch, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.relu(self.bn1(self.dw(x)))
        return self.relu(self.bn2(self.pw(x)))


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0):
        super().__init__()
        ch = _width(32, width_mult)
        self.stem = nn.Sequential(nn.Conv2d(3, ch, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(ch),
                                  nn.ReLU(inplace=True))
        blocks = []
        for width, stride in BLOCKS:
            out = _width(width, width_mult)
            blocks.append(DepthwiseSeparable(ch, out, stride))
            ch = out
        self.blocks = nn.Sequential(*blocks)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(ch, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.blocks(self.stem(x))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def mobilenet(num_classes: int = 1000) -> MobileNetV1:
    return MobileNetV1(num_classes)
