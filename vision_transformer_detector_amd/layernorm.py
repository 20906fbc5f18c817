"""Keras LayerNormalization(axis=-1) as a differentiable op on device tensors.

layer_norm(x, gamma, beta, eps) = (x - mean) / sqrt(var + eps) * gamma + beta over the last
axis, fp32: forward by vtd_layernorm_stats + vtd_layernorm, backward by one
vtd_layernorm_backward call (dx, dgamma, dbeta; include/vtd.h).  There is no fallback: a tensor
the kernels do not cover raises.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L


def backward_workspace_bytes(rows: int, D: int) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_layernorm_backward_workspace_bytes(rows, D, ctypes.byref(n)),
            "vtd_layernorm_backward_workspace_bytes")
    return int(n.value)


def forward(x2d, gamma, beta, eps):
    """(y, stat) of x2d [rows][D] fp32 contiguous: y fp32 [rows][D], stat fp32 [rows][2] =
    (mean, rstd) per row."""
    rows, D = x2d.shape
    stat = torch.empty((rows, 2), device=x2d.device, dtype=torch.float32)
    y = torch.empty_like(x2d)
    with torch.cuda.device(x2d.device):
        s = L.stream_ptr()
        L.check(L.lib.vtd_layernorm_stats(x2d.data_ptr(), L.F32, rows, D, D, float(eps),
                                          stat.data_ptr(), s), "vtd_layernorm_stats")
        L.check(L.lib.vtd_layernorm(x2d.data_ptr(), L.F32, rows, D, D, gamma.data_ptr(),
                                    beta.data_ptr(), float(eps), y.data_ptr(), D, L.F32, s),
                "vtd_layernorm")
    return y, stat


def backward(x2d, stat, gamma, dy2d, add=None, params=True):
    """vtd_layernorm_backward on contiguous [rows][D] fp32 tensors: (dx, dgamma, dbeta); the last
    two None when params is False.  add (nullable, [rows][D]) is added to dx."""
    rows, D = x2d.shape
    dx = torch.empty_like(x2d)
    dg = db = ws = None
    ws_bytes = 0
    if params:
        dg = torch.empty(D, device=x2d.device, dtype=torch.float32)
        db = torch.empty(D, device=x2d.device, dtype=torch.float32)
        ws_bytes = backward_workspace_bytes(rows, D)
        ws = torch.empty(ws_bytes, device=x2d.device, dtype=torch.uint8)
    with torch.cuda.device(x2d.device):
        L.check(L.lib.vtd_layernorm_backward(
            x2d.data_ptr(), D, stat.data_ptr(), gamma.data_ptr(), dy2d.data_ptr(), D, L.ptr(add),
            D, rows, D, dx.data_ptr(), D, L.ptr(dg), L.ptr(db), L.ptr(ws), ws_bytes,
            L.stream_ptr()), "vtd_layernorm_backward")
    return dx, dg, db


class _LayerNorm(torch.autograd.Function):
    """Forward keeps x and the row statistics; backward is one C call."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        D = x.shape[-1]
        x2d = x.detach().reshape(-1, D)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        y, stat = forward(x2d, g, b, eps)
        ctx.save_for_backward(x2d, stat, g)
        return y.reshape(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2d, stat, g = ctx.saved_tensors
        dy2d = gy.to(torch.float32).reshape(x2d.shape).contiguous()
        params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dg, db = backward(x2d, stat, g, dy2d, params=params)
        return (dx.reshape(gy.shape), dg if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None)


def layer_norm(x, gamma, beta, eps=1e-3):
    """Keras LayerNormalization(axis=-1, epsilon=eps) of x, differentiable w.r.t. x, gamma and
    beta.

    x: float32 device tensor [..., D]; gamma, beta: float32 device tensors [D] on x's device.
    Returns y in x's shape; backward() fills x.grad, gamma.grad and beta.grad through one
    vtd_layernorm_backward call, bit-identical from run to run, with no synchronisation."""
    for name, t in (("x", x), ("gamma", gamma), ("beta", beta)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"layer_norm: {name} must be a device tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"layer_norm: {name} must be float32, got {t.dtype}")
    if x.dim() < 1 or x.shape[-1] < 1 or x.numel() < 1:
        raise ValueError(f"layer_norm: x {tuple(x.shape)} must be (..., D) and not empty")
    D = x.shape[-1]
    if tuple(gamma.shape) != (D,) or tuple(beta.shape) != (D,):
        raise ValueError(f"layer_norm: gamma {tuple(gamma.shape)} and beta {tuple(beta.shape)} "
                         f"must be ({D},)")
    if gamma.device != x.device or beta.device != x.device:
        raise ValueError("layer_norm: x, gamma and beta must be on one device")
    if not float(eps) > 0.0:
        raise ValueError(f"layer_norm: eps must be positive, got {eps}")
    return _LayerNorm.apply(x.contiguous(), gamma, beta, float(eps))
