"""Folded-BatchNorm inference.

In eval mode BatchNorm is a constant per-channel affine map, so every
``ConvBNAct`` / ``DepthwiseConvBNAct`` can run as ONE kernel,
``y = act(conv(x)·scale + bias (+ residual))`` (``infer_kernels.hip``), with

    scale = γ / sqrt(running_var + eps)
    bias  = β − running_mean·scale

Usage::

    model.eval()
    fold_for_inference(model)
    with torch.no_grad():
        logits = model(x)

The constants are computed in float64 and kept on each module as
non-persistent buffers (absent from ``state_dict``) in f32 — or in float64
when the module's own parameters are float64, as on the CPU reference path.
The weights are neither copied nor rescaled: the folded kernels read the same
bf16 shadow as the unfolded ones.

The folded route is taken when the module is folded, in eval mode, and grad
is disabled; otherwise the module runs as if it had never been folded.  A
training-mode forward DROPS the fold, so constants that further training made
stale are never used.  The constants are a snapshot: fold again after
``load_state_dict`` or any other change of γ, β or the running statistics.

Grouped, GroupNorm, squeeze-excite and tensor-parallel sharded modules are
left as they are; a model containing them still folds its dense and depthwise
convs.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .layers import ConvBNAct, DepthwiseConvBNAct, drop_fold


def _foldable(m: nn.Module) -> bool:
    return (type(m) in (ConvBNAct, DepthwiseConvBNAct)
            and not getattr(m.weight, "tensor_parallel", False))


def fold_for_inference(model: nn.Module) -> nn.Module:
    """Fold the BatchNorm of every dense and depthwise conv module of `model`
    into per-channel (scale, bias) constants.  Returns `model`."""
    for m in model.modules():
        if not _foldable(m):
            continue
        with torch.no_grad():
            scale = m.bn_weight.double() / torch.sqrt(
                m.running_var.double() + m.eps)
            bias = m.bn_bias.double() - m.running_mean.double() * scale
        dt = (torch.float64 if m.bn_weight.dtype == torch.float64
              else torch.float32)
        drop_fold(m)
        m.register_buffer("fold_scale", scale.to(dt).contiguous(),
                          persistent=False)
        m.register_buffer("fold_bias", bias.to(dt).contiguous(),
                          persistent=False)
        m._folded = True
    return model


def unfold_inference(model: nn.Module) -> nn.Module:
    """Remove every fold of `model`: it runs its BatchNorm again."""
    for m in model.modules():
        drop_fold(m)
    return model
