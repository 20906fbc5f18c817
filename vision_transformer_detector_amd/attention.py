"""The MultiHeadAttention core as a differentiable op on device tensors.

attention_core(qkv, num_heads, key_dim) = softmax(scale Q K^T) V per (image, head), forward by
vtd_attention_train (the streaming attention kernels, which also keep the row log-sum-exp),
backward by vtd_attention_backward (dQ, dK, dV with P recomputed from qkv and the LSE).  Both
run in the library's operand modes "bf16x3" (fp32 tensors, every product as three bf16 MFMA
products) and "bf16".  With `dropout` the attention probabilities pass the MultiHeadAttention
dropout inside the same kernels (vtd_attention_train_dropout / vtd_attention_backward_dropout):
the mask is generated in-kernel from (seed, step, site) and never stored.  There is no
fallback: a mode the kernels do not cover raises.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

MODES = {"bf16x3": (L.BF16X3, torch.float32), "bf16": (L.BF16, torch.bfloat16),
         "bfloat16": (L.BF16, torch.bfloat16)}


def padded_key_dim(key_dim: int) -> int:
    """The library's per-head column count dkp for a Keras key_dim."""
    if not 1 <= key_dim <= 128:
        raise ValueError(f"attention_core: key_dim must be in [1, 128], got {key_dim}")
    return 32 if key_dim <= 32 else (64 if key_dim <= 64 else 128)


def train_forward(qkv2d, B, N, heads, dkp, scale, code, drop=None):
    """vtd_attention_train on qkv2d [B*N][3 heads dkp] (contiguous): (O in operand form --
    bf16 [B*N][inner], or the split [hi | lo] bf16 [B*N][2 inner] -- and lse fp32 [B][heads][N]).
    drop: a VtdDropout (vtd_attention_train_dropout) or None."""
    inner = heads * dkp
    ldo = 2 * inner if code == L.BF16X3 else inner
    o = torch.empty((B * N, ldo), device=qkv2d.device, dtype=torch.bfloat16)
    lse = torch.empty((B, heads, N), device=qkv2d.device, dtype=torch.float32)
    with torch.cuda.device(qkv2d.device):
        if drop is None:
            L.check(L.lib.vtd_attention_train(qkv2d.data_ptr(), B, N, heads, dkp, qkv2d.shape[1],
                                              float(scale), o.data_ptr(), ldo, lse.data_ptr(), code,
                                              L.stream_ptr()), "vtd_attention_train")
        else:
            L.check(L.lib.vtd_attention_train_dropout(
                qkv2d.data_ptr(), B, N, heads, dkp, qkv2d.shape[1], float(scale), o.data_ptr(), ldo,
                lse.data_ptr(), code, L.stream_ptr(), ctypes.byref(drop)),
                "vtd_attention_train_dropout")
    return o, lse


def backward_workspace_bytes(B, N, heads, dkp, code) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_attention_backward_workspace_bytes(B, N, heads, dkp, code, ctypes.byref(n)),
            "vtd_attention_backward_workspace_bytes")
    return int(n.value)


def backward(qkv2d, o, do2d, lse, B, N, heads, dkp, scale, code, drop=None):
    """vtd_attention_backward: dqkv in operand form, bf16 [B*N][3 inner] or the split
    [hi | lo] bf16 [B*N][6 inner].  do2d [B*N][inner] in qkv2d's dtype, pad columns zero."""
    inner = heads * dkp
    ldd = 6 * inner if code == L.BF16X3 else 3 * inner
    dqkv = torch.empty((B * N, ldd), device=qkv2d.device, dtype=torch.bfloat16)
    ws_bytes = backward_workspace_bytes(B, N, heads, dkp, code)
    ws = torch.empty(ws_bytes, device=qkv2d.device, dtype=torch.uint8)
    args = (qkv2d.data_ptr(), o.data_ptr(), do2d.data_ptr(), lse.data_ptr(), B, N, heads, dkp,
            qkv2d.shape[1], o.shape[1], do2d.shape[1], float(scale), dqkv.data_ptr(), ldd, code,
            ws.data_ptr(), ws_bytes, L.stream_ptr())
    with torch.cuda.device(qkv2d.device):
        if drop is None:
            L.check(L.lib.vtd_attention_backward(*args), "vtd_attention_backward")
        else:
            L.check(L.lib.vtd_attention_backward_dropout(*args, ctypes.byref(drop)),
                    "vtd_attention_backward_dropout")
    return dqkv


def _plain(op, code):
    """Operand form -> a plain tensor: bf16 as it is, the split form as fp32 hi + lo."""
    if code != L.BF16X3:
        return op
    P = op.shape[1] // 2
    return op[:, :P].float() + op[:, P:].float()


class _AttentionCore(torch.autograd.Function):
    """Forward keeps qkv, O in operand form and the LSE; backward is one C call."""

    @staticmethod
    def forward(ctx, qkv, heads, key_dim, dkp, scale, code, drop=None):
        B, N, _ = qkv.shape
        qkv2d = qkv.detach().reshape(B * N, 3 * heads * dkp)
        o, lse = train_forward(qkv2d, B, N, heads, dkp, scale, code, drop)
        ctx.save_for_backward(qkv2d, o, lse)
        ctx.dims = (B, N, heads, key_dim, dkp, scale, code)
        ctx.drop = drop
        return _plain(o, code).reshape(B, N, heads * dkp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        qkv2d, o, lse = ctx.saved_tensors
        B, N, heads, key_dim, dkp, scale, code = ctx.dims
        g = g.to(qkv2d.dtype)
        if key_dim < dkp:
            # the kernel reads dO's pad columns; O's are constants (zero), so is their gradient
            g = g.reshape(B, N, heads, dkp).clone()
            g[..., key_dim:] = 0
        do2d = g.reshape(B * N, heads * dkp).contiguous()
        dqkv = backward(qkv2d, o, do2d, lse, B, N, heads, dkp, scale, code, ctx.drop)
        return (_plain(dqkv, code).reshape(B, N, 3 * heads * dkp), None, None, None, None, None,
                None)


def attention_core(qkv, num_heads, key_dim, dtype="bf16x3", scale=None, dropout=None, seed=None,
                   step=0, site=0):
    """softmax(scale Q K^T) V of a Keras MultiHeadAttention, differentiable w.r.t. qkv.

    qkv: device tensor [B, N, 3 * num_heads * dkp] in the library's layout -- Q, K, V of head h
    at columns h * dkp, inner + h * dkp, 2 * inner + h * dkp (inner = num_heads * dkp, dkp =
    key_dim padded to 32 / 64 / 128, pad columns zero) -- float32 for dtype "bf16x3", bfloat16
    for "bf16".  scale defaults to 1 / sqrt(key_dim).  Returns O [B, N, num_heads * dkp] in
    qkv's dtype; backward() fills qkv.grad through vtd_attention_backward, bit-identical from
    run to run, with no synchronisation.

    dropout: the MultiHeadAttention dropout rate on the attention probabilities (training
    semantics: kept probabilities times 1 / (1 - rate), dropped ones zero, after the softmax).
    None or 0 is the op without dropout, bit for bit.  A positive rate needs `seed`: the mask
    bit of (image, head, query, key) is a function of (seed, step, site) alone, so the same
    arguments give the same bits, and the backward regenerates the forward's mask."""
    if dtype not in MODES:
        raise ValueError(f"attention_core: dtype must be one of {sorted(MODES)}, got {dtype!r}")
    code, tdt = MODES[dtype]
    dkp = padded_key_dim(int(key_dim))
    heads = int(num_heads)
    if not torch.is_tensor(qkv) or not qkv.is_cuda:
        raise ValueError("attention_core: qkv must be a device tensor")
    if qkv.dtype != tdt:
        raise ValueError(f"attention_core: dtype {dtype!r} takes {tdt} qkv, got {qkv.dtype}")
    if qkv.dim() != 3 or heads < 1 or qkv.shape[2] != 3 * heads * dkp or qkv.shape[0] < 1 \
            or qkv.shape[1] < 1:
        raise ValueError(f"attention_core: qkv {tuple(qkv.shape)} must be (B, N, 3 * num_heads * "
                         f"{dkp})")
    from .dropout import spec
    drop = spec("attention_core", dropout, seed, step, site)
    scale = 1.0 / math.sqrt(key_dim) if scale is None else float(scale)
    if drop is None:
        return _AttentionCore.apply(qkv.contiguous(), heads, int(key_dim), dkp, scale, code)
    return _AttentionCore.apply(qkv.contiguous(), heads, int(key_dim), dkp, scale, code, drop)
