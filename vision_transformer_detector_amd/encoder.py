"""One encoder block of the detector as a differentiable op on device tensors.

encoder_block(x, weights, ...) is the reference's block (vtd.py:350-412):
x1 = x + MultiHeadAttention(LayerNorm(x)), y = x1 + MLP(LayerNorm(x1)), from the block's Keras
weights in their Keras shapes; with `dropout` the MultiHeadAttention dropout on the attention
probabilities and a Dropout after every MLP activation, masks generated inside the kernels from
(seed, step, site_base).  Forward and backward are one vtd_encoder_block_backward call
each (include/vtd.h): the forward keeps only x and the weights, the backward recomputes the
training forward and fills every gradient.  There is no fallback: what the kernels do not cover
raises.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

_FIXED = ("ln1_gamma", "ln1_beta", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln2_gamma",
          "ln2_beta")
_LABELS = ("ln1 gamma", "ln1 beta", "query kernel", "query bias", "key kernel", "key bias",
           "value kernel", "value bias", "attention_output kernel", "attention_output bias",
           "ln2 gamma", "ln2 beta")


def _dtype_code(dtype) -> int:
    from .detector import _resolve_dtype
    code = _resolve_dtype(dtype)
    if code not in (L.BF16X3, L.BF16):
        raise ValueError(f"encoder_block: dtype {dtype!r} has no backward: use 'bf16x3' or "
                         "'bfloat16'")
    return code


def block_dims(batch, tokens, d, num_heads, key_dim, mlp_quantities, use_mish=True,
               dtype="bf16x3") -> L.VtdBlockDims:
    return L.VtdBlockDims(batch=int(batch), tokens=int(tokens), d=int(d),
                          num_heads=int(num_heads), key_dim=int(key_dim),
                          mlp_quantities=int(mlp_quantities), use_mish=1 if use_mish else 0,
                          dtype=_dtype_code(dtype))


def workspace_bytes(dims: L.VtdBlockDims) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_encoder_block_backward_workspace_bytes(ctypes.byref(dims), ctypes.byref(n)),
            "vtd_encoder_block_backward_workspace_bytes")
    return int(n.value)


def weight_shapes(d, num_heads, key_dim, mlp_quantities):
    """The Keras shapes of one block's weights in creation order (`keras_weight_names`)."""
    shapes = [(d,), (d,)]
    for _ in range(3):
        shapes += [(d, num_heads, key_dim), (num_heads, key_dim)]
    shapes += [(num_heads, key_dim, d), (d,), (d,), (d,)]
    k = d
    for j in range(mlp_quantities):
        n = d << (mlp_quantities - 1 - j)
        shapes += [(k, n), (n,)]
        k = n
    return shapes


def _fill(struct, tensors, q):
    for name, t in zip(_FIXED, tensors[:12]):
        setattr(struct, name, t.data_ptr())
    for j in range(q):
        struct.w_mlp[j] = tensors[12 + 2 * j].data_ptr()
        struct.b_mlp[j] = tensors[13 + 2 * j].data_ptr()
    return struct


def run(x, weights, dims: L.VtdBlockDims, dy=None, want_dx=True, want_y=True, ws=None, out=None,
        drop=None):
    """vtd_encoder_block_backward on contiguous fp32 device tensors: x (B, N, d), `weights` the
    block's 12 + 2 q tensors in creation order, dy (B, N, d) or None (the training forward
    alone).  Returns (y or None, grads or None, dx or None): `grads` a list of tensors in the
    weights' order and shapes.  ws: a uint8 workspace of at least workspace_bytes(dims).  out
    (y, grads, dx): the caller's own output tensors in place of new ones.  drop: a
    VtdBlockDropout (vtd_encoder_block_backward_dropout) or None."""
    q = dims.mlp_quantities
    if ws is None:
        ws = torch.empty(workspace_bytes(dims), device=x.device, dtype=torch.uint8)
    oy, ograds, odx = out if out is not None else (None, None, None)
    y = (oy if oy is not None else torch.empty_like(x)) if want_y else None
    params = _fill(L.VtdBlockParams(), weights, q)
    grads = dx = gstruct = None
    if dy is not None:
        grads = ograds if ograds is not None else [torch.empty_like(t) for t in weights]
        gstruct = _fill(L.VtdBlockGrads(), grads, q)
        if want_dx:
            dx = odx if odx is not None else torch.empty_like(x)
            gstruct.dx = dx.data_ptr()
    args = (ctypes.byref(dims), ctypes.byref(params), x.data_ptr(), L.ptr(dy), L.ptr(y),
            ctypes.byref(gstruct) if gstruct is not None else None, ws.data_ptr(), ws.numel(),
            L.stream_ptr())
    with torch.cuda.device(x.device):
        if drop is None:
            L.check(L.lib.vtd_encoder_block_backward(*args), "vtd_encoder_block_backward")
        else:
            L.check(L.lib.vtd_encoder_block_backward_dropout(*args, ctypes.byref(drop)),
                    "vtd_encoder_block_backward_dropout")
    return y, grads, dx


class _EncoderBlock(torch.autograd.Function):
    """Forward: the C entry with dy = NULL, keeping x and the weights only.  Backward: one C call
    that recomputes the training forward and fills the gradients."""

    @staticmethod
    def forward(ctx, x, dims, *weights):
        dims, drop = dims if isinstance(dims, tuple) else (dims, None)
        xd = x.detach()
        wd = [t.detach().contiguous() for t in weights]
        y, _, _ = run(xd, wd, dims, drop=drop)
        ctx.dims = dims
        ctx.drop = drop
        ctx.save_for_backward(xd, *wd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xd, *wd = ctx.saved_tensors
        dy = gy.to(torch.float32).reshape(xd.shape).contiguous()
        need = ctx.needs_input_grad
        _, grads, dx = run(xd, wd, ctx.dims, dy=dy, want_dx=need[0], want_y=False, drop=ctx.drop)
        return (dx, None) + tuple(g if n else None for g, n in zip(grads, need[2:]))


def encoder_block(x, weights, *, num_heads, key_dim, use_mish=True, dtype="bf16x3", dropout=None,
                  seed=None, step=0, site_base=0):
    """One encoder block (vtd.py:350-412), differentiable w.r.t. x and every weight.

    x: float32 device tensor (B, N, d).  weights: a sequence (or an OrderedDict, whose values are
    taken) of float32 device tensors in the Keras creation order of one block, in Keras shapes:
    ln1 gamma, beta (d,); query, key, value kernel (d, num_heads, key_dim) and bias (num_heads,
    key_dim) each; attention_output kernel (num_heads, key_dim, d), bias (d,); ln2 gamma, beta;
    then encoder_mlp_quantities kernel / bias pairs of widths d 2^(q-1) ... d
    (`Model.encoder_block_weights` returns them so).  use_mish: Mish, else tanh-GELU.  dtype:
    'bf16x3' or 'bfloat16', the operand mode of the Dense products and the attention core; the
    residual stream and every gradient are float32.  Returns y (B, N, d); backward() makes one
    vtd_encoder_block_backward call, bit-identical from run to run, with no synchronisation;
    inputs that do not require grad get None.

    dropout: the reference's `dropout` rate inside the block, training semantics: on the
    attention probabilities (site `site_base`) and after the activation of MLP layer j (site
    `site_base + 1 + j`; the last layer's too, before the residual add).  None or 0 is the block
    without dropout, bit for bit.  A positive rate needs `seed`: every mask bit is a function of
    (seed, step, site, index) alone, and the backward regenerates the forward's masks.  Blocks
    chained through autograd must take distinct site_base values: i * (1 + mlp_quantities) for
    block i; advance `step` once per training step."""
    if isinstance(weights, dict):
        weights = list(weights.values())
    else:
        weights = list(weights)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("encoder_block: x must be a device tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"encoder_block: x must be float32, got {x.dtype}")
    if x.dim() != 3 or x.numel() < 1:
        raise ValueError(f"encoder_block: x {tuple(x.shape)} must be (B, N, d) and not empty")
    if len(weights) < 14 or len(weights) % 2:
        raise ValueError(f"encoder_block: weights must hold 12 + 2 q tensors (q >= 1 MLP layers), "
                         f"got {len(weights)}")
    q = (len(weights) - 12) // 2
    if q > L.MAX_MLP:
        raise ValueError(f"encoder_block: {q} MLP layers, at most {L.MAX_MLP}")
    if int(num_heads) < 1 or int(key_dim) < 1:
        raise ValueError("encoder_block: num_heads and key_dim must be positive")
    B, N, d = x.shape
    labels = list(_LABELS)
    for j in range(q):
        labels += [f"MLP {j + 1} kernel", f"MLP {j + 1} bias"]
    shapes = weight_shapes(d, int(num_heads), int(key_dim), q)
    for i, (label, t, shape) in enumerate(zip(labels, weights, shapes)):
        what = f"weights[{i}] ({label})"
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"encoder_block: {what} must be a device tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"encoder_block: {what} must be float32, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"encoder_block: {what} must be on x's device")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"encoder_block: {what} has shape {tuple(t.shape)}, expected {shape}")
    dims = block_dims(B, N, d, num_heads, key_dim, q, use_mish, dtype)
    from .dropout import spec
    d1 = spec("encoder_block", dropout, seed, step, site_base)
    if d1 is None:
        return _EncoderBlock.apply(x.contiguous(), dims, *weights)
    if int(site_base) + q >= 1 << 32:
        raise ValueError("encoder_block: site_base + mlp_quantities must fit 32 bits")
    drop = L.VtdBlockDropout(seed=d1.seed, step=d1.step, site_base=d1.site, rate=d1.rate)
    return _EncoderBlock.apply(x.contiguous(), (dims, drop), *weights)
