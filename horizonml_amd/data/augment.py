"""On-device ``RandomCrop(size, padding=pad)`` + ``RandomHorizontalFlip``
for raw uint8 batches, fused into the normalize pass.

The GPU path is ONE pass over the batch (``k_augment_normalize_u8``, plus a
one-thread counter bump): the crop offset and the flip are folded into the
gather address of the u8 NCHW -> bf16 NHWC normalize, and the per-sample parameters come from a counter-based hash of
``(key, step, sample index)`` whose step counter lives on the device and is
advanced by the op itself — a replayed hipGraph therefore draws fresh
parameters every step with no host involvement.

``augment_params`` is the exact CPU mirror of the kernel's hash (unsigned
32-bit arithmetic written as masked int64), ``augment_reference`` the exact
mirror of its gather; together with ``normalize_uint8`` they define what the
kernel must produce, bit for bit.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .cifar import _MEAN, _STD, normalize_uint8

_M32 = 0xFFFFFFFF
_GOLD = 0x9E3779B1   # sample-index spread
_WORD = 0x85EBCA77   # per-word offset (r0, r1, r2 = 1x, 2x, 3x)


def _mul32(a, c: int):
    """(a * c) mod 2**32 for 0 <= a < 2**32 without leaving int64's range
    (works on python ints and int64 tensors alike)."""
    lo = a * (c & 0xFFFF)
    hi = (a * (c >> 16)) & 0xFFFF
    return (lo + (hi << 16)) & _M32


def _fmix32(h):
    """murmur3 32-bit finaliser."""
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    h = h ^ (h >> 16)
    return h


def augment_params(key: int, step: int, n_samples: int, pad: int,
                   flip: bool = True
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-sample ``(dy, dx, fl)`` (int64 CPU tensors of length
    ``n_samples``) exactly as the kernel derives them for ``state = [key,
    step]``: ``0 <= dy, dx <= 2*pad``, ``fl`` in {0, 1} (all 0 when
    ``flip`` is off).  Only the low 32 bits of ``step`` enter the hash; the
    key is split into two 32-bit halves."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    klo, khi, slo = key & _M32, key >> 32, int(step) & _M32
    seed = _fmix32(_fmix32(_fmix32(klo) ^ khi) ^ slo)
    n = torch.arange(n_samples, dtype=torch.int64)
    t = _fmix32(_mul32(n, _GOLD) ^ seed)
    rng = 2 * int(pad) + 1
    r0 = _fmix32((t + _WORD) & _M32)
    r1 = _fmix32((t + 2 * _WORD) & _M32)
    r2 = _fmix32((t + 3 * _WORD) & _M32)
    dy = (r0 * rng) >> 32
    dx = (r1 * rng) >> 32
    fl = (r2 >> 31) if flip else torch.zeros_like(r2)
    return dy, dx, fl


def augment_reference(x_u8: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor,
                      fl: torch.Tensor, pad: int) -> torch.Tensor:
    """Zero-pad the raw uint8 NCHW batch by ``pad``, crop sample ``n`` at
    offset ``(dy[n], dx[n])`` back to ``H x W``, then mirror it horizontally
    where ``fl[n]`` is set (flip AFTER crop, torchvision's order).  Works on
    any device; returns uint8."""
    N, _, H, W = x_u8.shape
    dev = x_u8.device
    dy = dy.to(dev).view(N, 1, 1)
    dx = dx.to(dev).view(N, 1, 1)
    fl = fl.to(dev).view(N, 1, 1)
    ho = torch.arange(H, device=dev).view(1, H, 1)
    wo = torch.arange(W, device=dev).view(1, 1, W)
    hi = ho + dy - pad
    wi = torch.where(fl != 0, W - 1 - wo, wo) + dx - pad
    ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)          # [N, H, W]
    idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1))       # [N, H, W]
    C = x_u8.shape[1]
    g = x_u8.reshape(N, C, H * W).gather(
        2, idx.view(N, 1, H * W).expand(N, C, H * W)).view(N, C, H, W)
    return torch.where(ok.view(N, 1, H, W), g, torch.zeros_like(g))


def pack_params(dy: torch.Tensor, dx: torch.Tensor,
                fl: torch.Tensor) -> torch.Tensor:
    """``dy | dx << 8 | fl << 16`` as int32 — the kernel's explicit-mode
    parameter word."""
    return (dy | (dx << 8) | (fl << 16)).to(torch.int32)


class DeviceAugment:
    """Random crop + flip + normalize for raw uint8 batches.

    GPU: the fused kernel plus a one-thread launch that advances ``step``;
    ``state`` (int64 ``[key, step]``) lives on the device, so the call can
    be captured in a hipGraph.  CPU: ``augment_reference`` with
    ``augment_params`` and the f32 normalize, advancing a host step — the
    same stream of crops and flips as the GPU path."""

    def __init__(self, key: int, pad: int = 4, flip: bool = True,
                 device: Optional[torch.device] = None):
        if not 0 <= int(pad) <= 127:
            raise ValueError(f"pad must be in [0, 127], got {pad}")
        self.key = int(key) & 0xFFFFFFFFFFFFFFFF
        self.pad = int(pad)
        self.flip = bool(flip)
        self.device = torch.device(device if device is not None else "cpu")
        self._host_step = 0
        self.state = None
        if self.device.type == "cuda":
            from .. import ops as _ops
            self._ext = _ops.extension()  # a missing kernel is an error
            skey = self.key - (1 << 64) if self.key >= (1 << 63) else self.key
            self.state = torch.tensor([skey, 0], dtype=torch.int64,
                                      device=self.device)

    def set_step(self, s: int) -> None:
        if self.state is not None:
            self.state[1:].copy_(torch.tensor([int(s)]))
        else:
            self._host_step = int(s)

    def step(self) -> int:
        """Current step (syncs on GPU — not for the hot loop)."""
        if self.state is not None:
            return int(self.state[1].item())
        return self._host_step

    def __call__(self, x_u8: torch.Tensor) -> torch.Tensor:
        if x_u8.dim() != 4 or x_u8.dtype != torch.uint8:
            raise ValueError("DeviceAugment expects a uint8 NCHW batch")
        if self.state is not None:
            return self._ext.augment_normalize_u8(
                x_u8.contiguous(), self.state, _MEAN, _STD, self.pad,
                self.flip, None)
        dy, dx, fl = augment_params(self.key, self._host_step,
                                    x_u8.shape[0], self.pad, self.flip)
        self._host_step += 1
        return normalize_uint8(augment_reference(x_u8, dy, dx, fl, self.pad))
