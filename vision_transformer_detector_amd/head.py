"""The detection head of the detector as a differentiable op on device tensors.

The head (mlp_head, vtd.py:454-493): Dense(17) on encoded (B, N, d), Reshape((17, -1)), n_head
blocks of Dense + Mish (or tanh-GELU) each followed by a Dropout, Dense(6).  Forward and backward
are one vtd_head_backward call each (include/vtd.h; vtd_head_backward_dropout with dropout): the
forward keeps only `encoded` and the weights, the backward recomputes the training forward --
regenerating the forward's masks from the same (seed, step, site_base) -- and fills every
gradient.  `Model.detection_head` is the public entry; there is no fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L


def workspace_bytes(cfg: L.VtdConfig) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_head_backward_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)),
            "vtd_head_backward_workspace_bytes")
    return int(n.value)


def _fill(struct, tensors):
    """tensors: the head's kernel / bias pairs in Keras creation order (`head_weight_names`)."""
    n_head = len(tensors) // 2 - 2
    struct.w_det, struct.b_det = tensors[0].data_ptr(), tensors[1].data_ptr()
    for j in range(n_head):
        struct.w_head[j] = tensors[2 + 2 * j].data_ptr()
        struct.b_head[j] = tensors[3 + 2 * j].data_ptr()
    struct.w_final, struct.b_final = tensors[-2].data_ptr(), tensors[-1].data_ptr()
    return struct


def run(cfg, encoded, weights, dlogits=None, logits=None, grads=None, d_encoded=None, ws=None,
        drop=None):
    """vtd_head_backward on contiguous fp32 device tensors: encoded (B, N, d), `weights` the head's
    2 (n_head + 2) tensors in creation order.  dlogits None: the training forward alone into
    `logits` (B, 17, 6).  Else the forward + backward: the weight gradients into `grads` (tensors
    in the weights' order) and d loss / d encoded into `d_encoded` (None: not computed).  ws: a
    uint8 workspace of at least workspace_bytes(cfg).  drop: a VtdBlockDropout
    (vtd_head_backward_dropout: site_base + j is head layer j's site) or None."""
    if ws is None:
        ws = torch.empty(workspace_bytes(cfg), device=encoded.device, dtype=torch.uint8)
    params = _fill(L.VtdHeadParams(), weights)
    gstruct = None
    if dlogits is not None:
        gstruct = _fill(L.VtdHeadGrads(), grads)
        gstruct.d_encoded = L.ptr(d_encoded)
    with torch.cuda.device(encoded.device):
        args = (ctypes.byref(cfg), ctypes.byref(params), encoded.data_ptr(), L.ptr(dlogits),
                L.ptr(logits), ctypes.byref(gstruct) if gstruct is not None else None,
                ws.data_ptr(), ws.numel(), L.stream_ptr())
        if drop is None:
            L.check(L.lib.vtd_head_backward(*args), "vtd_head_backward")
        else:
            L.check(L.lib.vtd_head_backward_dropout(*args, ctypes.byref(drop)),
                    "vtd_head_backward_dropout")


class DetectionHead(torch.autograd.Function):
    """DetectionHead.apply(encoded, (cfg, drop), *weights) -> logits (B, 17, 6), arguments already
    checked (Model.detection_head): cfg the model's vtd_config at encoded's batch, drop a
    VtdBlockDropout or None.  Forward: the C entry with dlogits = NULL, keeping encoded and the
    weights only.  Backward: one C call that recomputes the training forward and fills the
    gradients."""

    @staticmethod
    def forward(ctx, encoded, call, *weights):
        cfg, drop = call
        ed = encoded.detach()
        wd = [t.detach().contiguous() for t in weights]
        logits = torch.empty((ed.shape[0], L.MAX_DETECT, 6), dtype=torch.float32, device=ed.device)
        run(cfg, ed, wd, logits=logits, drop=drop)
        ctx.call = call
        ctx.save_for_backward(ed, *wd)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ed, *wd = ctx.saved_tensors
        cfg, drop = ctx.call
        dlogits = g.to(torch.float32).reshape(ed.shape[0], L.MAX_DETECT, 6).contiguous()
        need = ctx.needs_input_grad
        grads = [torch.empty_like(t) for t in wd]
        dx = torch.empty_like(ed) if need[0] else None
        run(cfg, ed, wd, dlogits=dlogits, grads=grads, d_encoded=dx, drop=drop)
        return (dx, None) + tuple(t if n else None for t, n in zip(grads, need[2:]))

