"""Dropout on the device: the Keras `Dropout` layer as a differentiable op, and the mask itself.

The mask is generated inside the kernels (Philox4x32-10, csrc/vtd_philox.h) and is a pure
function of (seed, step, site, logical index): this library has no implicit randomness, every
result is reproducible from its arguments.  TensorFlow's random stream is not reproduced; the
distribution and the graph are the reference's, the bits of the mask are this library's.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L


def spec(what, rate, seed, step=0, site=0):
    """The vtd_dropout of (rate, seed, step, site), or None for a rate of None / 0 (no dropout:
    the caller runs today's path).  A positive rate needs a seed."""
    if rate is None:
        return None
    rate = float(rate)
    if math.isnan(rate) or not 0.0 <= rate < 1.0:
        raise ValueError(f"{what}: dropout rate must be in [0, 1), got {rate}")
    if rate == 0.0:
        return None
    if seed is None:
        raise ValueError(f"{what}: dropout > 0 needs a seed (no implicit randomness: the mask is a "
                         "function of seed, step and site)")
    seed, step, site = int(seed), int(step), int(site)
    if not (0 <= seed < 1 << 64 and 0 <= step < 1 << 64 and 0 <= site < 1 << 32):
        raise ValueError(f"{what}: seed and step must fit 64 unsigned bits, site 32")
    return L.VtdDropout(seed=seed, step=step, site=site, rate=rate)


def inv_keep(rate) -> float:
    """The kept scale the kernels use: fp32 of 1 / (1 - thr / 65536), thr = round(rate 65536)."""
    thr = min(int(float(rate) * 65536.0 + 0.5), 65535)
    return float(torch.tensor(1.0 / (1.0 - thr / 65536.0), dtype=torch.float32))


def _apply(x2d, d):
    y = torch.empty_like(x2d)
    with torch.cuda.device(x2d.device):
        L.check(L.lib.vtd_dropout_apply(ctypes.byref(d), x2d.data_ptr(), x2d.shape[1],
                                        x2d.shape[0], x2d.shape[1], y.data_ptr(), y.shape[1],
                                        L.stream_ptr()), "vtd_dropout_apply")
    return y


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, d):
        ctx.d = d
        return _apply(x.detach().reshape(-1, x.shape[-1]).contiguous(), d).reshape(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g2 = g.to(torch.float32).reshape(-1, g.shape[-1]).contiguous()
        return _apply(g2, ctx.d).reshape(g.shape), None


def dropout(x, rate, seed, step=0, site=0):
    """Keras Dropout(rate) in training on a float32 device tensor [..., N]: kept values times
    inv_keep, dropped ones +0; element (row, column) of x viewed as [rows][N] takes mask bit
    (row, column) of (seed, step, site).  Differentiable; rate None / 0 returns x."""
    d = spec("dropout", rate, seed, step, site)
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 1 \
            or x.numel() < 1:
        raise ValueError("dropout: x must be a non-empty float32 device tensor")
    return x if d is None else _Dropout.apply(x, d)


def dropout_mask(shape, rate, seed, step=0, site=0, device="cuda"):
    """The mask the kernels generate, as a bool device tensor (True = kept): shape (rows, N) for
    an elementwise site, (B, heads, N, N) for an attention site."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 4) or min(shape) < 1 or (len(shape) == 4 and shape[2] != shape[3]):
        raise ValueError(f"dropout_mask: shape must be (rows, N) or (B, heads, N, N), got {shape}")
    d = spec("dropout_mask", rate, seed, step, site)
    if d is None:
        return torch.ones(shape, dtype=torch.bool, device=device)
    out = torch.empty(shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        if len(shape) == 2:
            L.check(L.lib.vtd_dropout_mask(ctypes.byref(d), shape[0], shape[1], out.data_ptr(),
                                           shape[1], L.stream_ptr()), "vtd_dropout_mask")
        else:
            L.check(L.lib.vtd_dropout_mask_attention(ctypes.byref(d), shape[0], shape[1], shape[2],
                                                     out.data_ptr(), L.stream_ptr()),
                    "vtd_dropout_mask_attention")
    return out.bool()
