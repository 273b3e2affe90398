"""ResNet-50 (bottleneck v1.5: stride on the 3x3 conv), written from scratch (torchvision is not installed).

BASELINE.json lists "ResNet-50 on synthetic 3x224x224 DDP 8xMI355X" as an extension configuration of this
framework.  The reference's second application (``ppe_main_ddp.py``) fine-tunes a ResNet-101 under the same DDP
wrapper; its model file is missing from the reference, so the ResNet family here is defined
from the standard architecture: stem 7x7/2 conv + 3x3/2 max-pool, stages of [3, 4, 6, 3] (ResNet-50) or
[3, 4, 23, 3] (ResNet-101) bottlenecks with expansion 4, global average pool, fc.  ``groups`` / ``width_per_group``
give the ResNeXt members (``resnext50_32x4d``); the defaults are the plain ResNet.  ``se_reduction`` r > 0 gives every
bottleneck a squeeze-and-excitation gate (Hu et al.: ``se_resnet50``, ``se_resnext50_32x4d``, r = 16): bn3's output is
scaled per sample and channel by sigmoid(fc2(relu(fc1(its spatial mean))) before the residual add.

Training runs through the generic data-parallel path (``parallel/flat_ddp.py``: flat buffers, bucketed async
all-reduce overlapped with backward, fused flat SGD) with bf16 autocast and channels-last activations.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None,
                 groups: int = 1, width_per_group: int = 64, se_reduction: int = 0):
        super().__init__()
        out_ch = planes * self.expansion
        width = int(planes * width_per_group / 64) * groups  # torchvision's formula (ResNeXt: wider, grouped 3x3)
        self.conv1 = nn.Conv2d(in_ch, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, out_ch, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        if se_reduction > 0:  # (no module and no RNG draw otherwise)
            self.se = nn.Module()
            self.se.fc1 = nn.Linear(out_ch, out_ch // se_reduction)
            self.se.fc2 = nn.Linear(out_ch // se_reduction, out_ch)
        else:
            self.se = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.se is not None:
            s = self.se.fc2(torch.relu(self.se.fc1(out.mean((2, 3)))))
            out = out * torch.sigmoid(s)[:, :, None, None]
        return self.relu(out + idt)


class ResNet(nn.Module):
    def __init__(self, layers: List[int], num_classes: int = 1000, zero_init_residual: bool = True,
                 groups: int = 1, width_per_group: int = 64, se_reduction: int = 0):
        super().__init__()
        self.in_ch = 64
        self.groups, self.width_per_group, self.se_reduction = groups, width_per_group, se_reduction
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._stage(64, layers[0], 1)
        self.layer2 = self._stage(128, layers[1], 2)
        self.layer3 = self._stage(256, layers[2], 2)
        self.layer4 = self._stage(512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)

    def _stage(self, width: int, blocks: int, stride: int) -> nn.Sequential:
        out_ch = width * Bottleneck.expansion
        down = None
        if stride != 1 or self.in_ch != out_ch:
            down = nn.Sequential(nn.Conv2d(self.in_ch, out_ch, 1, stride=stride, bias=False), nn.BatchNorm2d(out_ch))
        gw = dict(groups=self.groups, width_per_group=self.width_per_group, se_reduction=self.se_reduction)
        mods = [Bottleneck(self.in_ch, width, stride, down, **gw)]
        self.in_ch = out_ch
        mods += [Bottleneck(out_ch, width, **gw) for _ in range(1, blocks)]
        return nn.Sequential(*mods)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet50(num_classes: int = 1000) -> ResNet:
    return ResNet([3, 4, 6, 3], num_classes)


def resnet101(num_classes: int = 1000) -> ResNet:
    return ResNet([3, 4, 23, 3], num_classes)


def resnext50_32x4d(num_classes: int = 1000) -> ResNet:
    """ResNeXt-50 32x4d: the ResNet-50 layout with 32-group 3x3 convolutions of width 128 / 256 / 512 / 1024."""
    return ResNet([3, 4, 6, 3], num_classes, groups=32, width_per_group=4)


def se_resnet50(num_classes: int = 1000) -> ResNet:
    """SE-ResNet-50: ResNet-50 with a squeeze-and-excitation gate (reduction 16) in every bottleneck."""
    return ResNet([3, 4, 6, 3], num_classes, se_reduction=16)


def se_resnext50_32x4d(num_classes: int = 1000) -> ResNet:
    """SE-ResNeXt-50 32x4d: ResNeXt-50 32x4d with the same gate."""
    return ResNet([3, 4, 6, 3], num_classes, groups=32, width_per_group=4, se_reduction=16)
