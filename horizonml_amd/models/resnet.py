"""ResNet family, built on the fused MI355X blocks in ``layers.py``.

Capability parity with the torchvision models the reference instantiates
(``resnet18`` at reference ``data_parallel_train.py:198``,
``layer_model_parallel_train.py:30``, ``tensor_parallel_train.py:74``;
``resnet50`` for the hybrid DP×PP config in BASELINE.json), but implemented
from scratch against our fused ConvBNAct blocks so the GPU path runs the
hand-written gfx950 kernels end to end.

Stems: ``imagenet`` = 7x7/2 conv + 3x3/2 maxpool (what the reference uses
even on CIFAR 32x32 inputs); ``cifar`` = 3x3/1 conv, no pool (offered as a
deliberate improvement, not the parity default).
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

from .layers import (ConvBNAct, ConvGNAct, GlobalAvgPool, GroupedConvBNAct,
                     Linear, MaxPool2d3x3s2, SqueezeExcite)


def _conv_ctor(norm: str, gn_groups: int):
    """The dense conv+norm+act module of a block: ``ConvBNAct`` for "bn" (the
    default: same modules, parameter order and state_dict keys as ever), or
    ``ConvGNAct`` with ``gn_groups`` groups for "gn"."""
    if norm == "bn":
        return ConvBNAct
    if norm != "gn":
        raise ValueError(f"unknown norm {norm!r} (bn | gn)")

    def make(in_ch, out_ch, kernel_size, **kw):
        return ConvGNAct(in_ch, out_ch, kernel_size, groups=gn_groups, **kw)
    return make


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_ch: int, ch: int, stride: int = 1,
                 norm: str = "bn", gn_groups: int = 32):
        super().__init__()
        conv = _conv_ctor(norm, gn_groups)
        self.conv1 = conv(in_ch, ch, 3, stride=stride, act=True)
        # conv2 fuses norm + residual add + final ReLU into one epilogue:
        # out = relu(norm(conv(x)) + identity)
        self.conv2 = conv(ch, ch, 3, stride=1, act=True)
        self.downsample = (conv(in_ch, ch, 1, stride=stride, act=False)
                           if (stride != 1 or in_ch != ch) else None)

    def _fusable(self) -> bool:
        return (type(self.conv1) is ConvBNAct and type(self.conv2) is ConvBNAct
                and (self.downsample is None
                     or type(self.downsample) is ConvBNAct))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and self._fusable():
            from ._functional_gpu import res_block
            return res_block(x, (self.conv1, self.conv2), self.downsample)
        identity = self.downsample(x) if self.downsample is not None else x
        out = self.conv1(x)
        return self.conv2(out, residual=identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch: int, ch: int, stride: int = 1,
                 groups: int = 1, base_width: int = 64,
                 se_reduction: int = 0, norm: str = "bn",
                 gn_groups: int = 32):
        super().__init__()
        if norm != "bn" and (groups > 1 or se_reduction > 0):
            raise ValueError("norm='gn' serves dense convs only: not with "
                             "groups > 1 or se_reduction")
        conv = _conv_ctor(norm, gn_groups)
        out_ch = ch * self.expansion
        # ResNeXt: the 3x3 is a grouped conv of `groups` x `base_width`-scaled
        # channels; the defaults give width == ch and a dense 3x3 (ResNet)
        width = int(ch * (base_width / 64.0)) * groups
        self.conv1 = conv(in_ch, width, 1, stride=1, act=True)
        if groups > 1:
            # runs per module on the GPU: _fusable() is False for this block
            self.conv2 = GroupedConvBNAct(width, width, 3, stride=stride,
                                          groups=groups, act=True)
        else:
            self.conv2 = conv(width, width, 3, stride=stride, act=True)
        # SE block: conv3 ends at its BN; the gate, the block residual and the
        # final ReLU are the SE op's.  Runs per module on the GPU.
        self.conv3 = conv(width, out_ch, 1, stride=1, act=se_reduction <= 0)
        self.downsample = (conv(in_ch, out_ch, 1, stride=stride, act=False)
                           if (stride != 1 or in_ch != out_ch) else None)
        # registered last and only when asked for: the default block keeps
        # its modules, parameter order and state_dict keys
        if se_reduction > 0:
            self.se = SqueezeExcite(out_ch, se_reduction)

    def _fusable(self) -> bool:
        return (getattr(self, "se", None) is None
                and type(self.conv1) is ConvBNAct
                and type(self.conv2) is ConvBNAct
                and type(self.conv3) is ConvBNAct
                and (self.downsample is None
                     or type(self.downsample) is ConvBNAct))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and self._fusable():
            from ._functional_gpu import res_block
            return res_block(x, (self.conv1, self.conv2, self.conv3),
                             self.downsample)
        identity = self.downsample(x) if self.downsample is not None else x
        out = self.conv1(x)
        out = self.conv2(out)
        if getattr(self, "se", None) is not None:
            return self.se(self.conv3(out), identity)
        return self.conv3(out, residual=identity)


class Stem(nn.Module):
    def __init__(self, kind: str = "imagenet", out_ch: int = 64,
                 norm: str = "bn", gn_groups: int = 32):
        super().__init__()
        self.kind = kind
        conv = _conv_ctor(norm, gn_groups)
        if kind == "imagenet":
            self.conv = conv(3, out_ch, 7, stride=2, padding=3, act=True)
            self.pool = MaxPool2d3x3s2()
        elif kind == "cifar":
            self.conv = conv(3, out_ch, 3, stride=1, padding=1, act=True)
            self.pool = nn.Identity()
        else:
            raise ValueError(f"unknown stem kind {kind!r}")

    def forward(self, x):
        return self.pool(self.conv(x))


class Tail(nn.Module):
    """avgpool + flatten + fc — the reference's last layer group
    (``layer_model_parallel_train.py:47-52``)."""

    def __init__(self, in_features: int, num_classes: int):
        super().__init__()
        self.pool = GlobalAvgPool()
        self.fc = Linear(in_features, num_classes)

    def forward(self, x):
        return self.fc(self.pool(x))


class ResNet(nn.Module):
    def __init__(self, block, layers: List[int], num_classes: int = 10,
                 stem: str = "imagenet", width: int = 64, groups: int = 1,
                 width_per_group: int = 64, se_reduction: int = 0,
                 norm: str = "bn", gn_groups: int = 32):
        super().__init__()
        if norm not in ("bn", "gn"):
            raise ValueError(f"unknown norm {norm!r} (bn | gn)")
        if norm == "gn" and (groups != 1 or se_reduction):
            raise ValueError("norm='gn' serves dense convs only: not with "
                             "groups > 1 or se_reduction")
        if ((groups != 1 or width_per_group != 64 or se_reduction)
                and block is not Bottleneck):
            raise ValueError("groups / width_per_group / se_reduction need "
                             "Bottleneck blocks")
        self.block_type = block
        self.groups, self.base_width = groups, width_per_group
        self.se_reduction = se_reduction
        self.norm, self.gn_groups = norm, gn_groups
        self.stem = (Stem(stem, width) if norm == "bn"
                     else Stem(stem, width, norm, gn_groups))
        self.in_ch = width
        self.layer1 = self._make_layer(block, width, layers[0], 1)
        self.layer2 = self._make_layer(block, width * 2, layers[1], 2)
        self.layer3 = self._make_layer(block, width * 4, layers[2], 2)
        self.layer4 = self._make_layer(block, width * 8, layers[3], 2)
        self.tail = Tail(width * 8 * block.expansion, num_classes)

    def _make_layer(self, block, ch: int, n: int, stride: int) -> nn.Sequential:
        # only the ResNeXt and SE variants pass the extra arguments on
        kw = ({} if self.groups == 1 and self.base_width == 64
              else dict(groups=self.groups, base_width=self.base_width))
        if self.se_reduction:
            kw["se_reduction"] = self.se_reduction
        if self.norm != "bn":
            kw.update(norm=self.norm, gn_groups=self.gn_groups)
        blocks = [block(self.in_ch, ch, stride, **kw)]
        self.in_ch = ch * block.expansion
        for _ in range(n - 1):
            blocks.append(block(self.in_ch, ch, 1, **kw))
        return nn.Sequential(*blocks)

    def forward(self, x):
        x = self.stem(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        return self.tail(x)

    # ---- partitioning support (SURVEY.md §2.2 SplitResNet parity) -------
    def layer_units(self, granularity: str = "group") -> List[Tuple[str, nn.Module]]:
        """Ordered pipeline units.

        ``group``  → 5 units: stem, layer1..layer3, (layer4+tail) — the
                     reference's layer-group decomposition
                     (``layer_model_parallel_train.py:37-52``).
        ``block``  → stem, every residual block, tail — supports up to
                     2 + Σlayers stages (10 for resnet18 → 8-stage pipelines
                     per BASELINE.json config #3).
        """
        if granularity == "group":
            tail = nn.Sequential(self.layer4, self.tail)
            return [("stem", self.stem), ("layer1", self.layer1),
                    ("layer2", self.layer2), ("layer3", self.layer3),
                    ("tail", tail)]
        elif granularity == "block":
            units: List[Tuple[str, nn.Module]] = [("stem", self.stem)]
            for li, layer in enumerate(
                    (self.layer1, self.layer2, self.layer3, self.layer4), 1):
                for bi, blk in enumerate(layer):
                    units.append((f"layer{li}.{bi}", blk))
            units.append(("tail", self.tail))
            return units
        raise ValueError(f"unknown granularity {granularity!r}")


def resnet18(num_classes: int = 10, stem: str = "imagenet") -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, stem)


def resnet34(num_classes: int = 10, stem: str = "imagenet") -> ResNet:
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes, stem)


def resnet50(num_classes: int = 1000, stem: str = "imagenet") -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem)


def resnext50_32x4d(num_classes: int = 1000, stem: str = "imagenet") -> ResNet:
    """ResNeXt-50 32x4d: the resnet50 layout with a 32-group 3x3 of 4, 8, 16
    and 32 channels per group in layers 1 to 4."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem, groups=32,
                  width_per_group=4)


def se_resnet50(num_classes: int = 1000, stem: str = "imagenet") -> ResNet:
    """SE-ResNet-50 (SENet): resnet50 with a reduction-16 SE gate per block."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem,
                  se_reduction=16)


def se_resnext50_32x4d(num_classes: int = 1000,
                       stem: str = "imagenet") -> ResNet:
    """SE-ResNeXt-50 32x4d: resnext50_32x4d with the same gate."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem, groups=32,
                  width_per_group=4, se_reduction=16)


def resnet18_gn(num_classes: int = 10, stem: str = "imagenet",
                gn_groups: int = 32) -> ResNet:
    """ResNet-18 with GroupNorm in place of every BatchNorm."""
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, stem, norm="gn",
                  gn_groups=gn_groups)


def resnet50_gn(num_classes: int = 1000, stem: str = "imagenet",
                gn_groups: int = 32) -> ResNet:
    """ResNet-50 with GroupNorm in place of every BatchNorm."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, stem, norm="gn",
                  gn_groups=gn_groups)


def build_model(name: str, num_classes: int = 10, stem: str = "imagenet") -> nn.Module:
    name = name.lower()
    if name in ("resnet18", "resnet"):
        return resnet18(num_classes, stem)
    if name == "resnet34":
        return resnet34(num_classes, stem)
    if name == "resnet50":
        return resnet50(num_classes, stem)
    if name in ("resnext50", "resnext50_32x4d"):
        return resnext50_32x4d(num_classes, stem)
    if name == "se_resnet50":
        return se_resnet50(num_classes, stem)
    if name in ("se_resnext50", "se_resnext50_32x4d"):
        return se_resnext50_32x4d(num_classes, stem)
    if name == "resnet18_gn":
        return resnet18_gn(num_classes, stem)
    if name == "resnet50_gn":
        return resnet50_gn(num_classes, stem)
    if name in ("mobilenet", "mobilenet_v2"):
        from .mobilenet import mobilenet_v2
        return mobilenet_v2(num_classes)
    raise ValueError(f"unknown model {name!r}")
