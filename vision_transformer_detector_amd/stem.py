"""The patch embedding of the detector as a differentiable op on device tensors.

patch_embedding(images, weights, ...) is the reference's transformer_preprocessor
(vtd.py:271-307): tf.image.extract_patches (SAME), the linear projection and the position
embedding add, from the three Keras weights in their Keras shapes.  Forward and backward are one
vtd_stem_backward call each (include/vtd.h): the forward keeps only the images and the weights,
the backward extracts the patches again and fills the three weight gradients.  The gradient of
the images is opt-in (`image_gradient=True`): one more call, vtd_stem_image_grad (`image_grad`).
There is no fallback: what the kernels do not cover raises.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

_LABELS = ("position embedding", "linear_projection kernel", "linear_projection bias")


def _dtype_code(dtype) -> int:
    from .detector import _resolve_dtype
    code = _resolve_dtype(dtype)
    if code not in (L.BF16X3, L.BF16):
        raise ValueError(f"patch_embedding: dtype {dtype!r} has no backward: use 'bf16x3' or "
                         "'bfloat16'")
    return code


def stem_dims(batch, H, W, C, patch_size, d, dtype="bf16x3") -> L.VtdStemDims:
    return L.VtdStemDims(batch=int(batch), H=int(H), W=int(W), C=int(C), patch=int(patch_size),
                         d=int(d), dtype=_dtype_code(dtype))


def workspace_bytes(dims: L.VtdStemDims) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_stem_backward_workspace_bytes(ctypes.byref(dims), ctypes.byref(n)),
            "vtd_stem_backward_workspace_bytes")
    return int(n.value)


def tokens_of(H, W, patch_size) -> int:
    p = int(patch_size)
    return (-(-int(H) // p)) * (-(-int(W) // p))


def weight_shapes(H, W, C, patch_size, d):
    """The Keras shapes of the stem's weights in creation order (`keras_weight_names`)."""
    p = int(patch_size)
    return [(tokens_of(H, W, p), 1), (p * p * int(C), int(d)), (int(d),)]


def _fill(tensors):
    s = L.VtdStemParams()
    s.pos, s.w, s.b = (t.data_ptr() for t in tensors)
    return s


def run(images, weights, dims: L.VtdStemDims, dx0=None, want_x0=True, ws=None, out=None):
    """vtd_stem_backward on contiguous fp32 device tensors: images (B, H, W, C), `weights` the
    three tensors in creation order, dx0 (B, N, d) or None (the training forward alone).
    Returns (x0 or None, grads or None): `grads` a list of tensors in the weights' order and
    shapes.  ws: a uint8 workspace of at least workspace_bytes(dims).  out (x0, grads): the
    caller's own output tensors in place of new ones."""
    if ws is None:
        ws = torch.empty(workspace_bytes(dims), device=images.device, dtype=torch.uint8)
    ox0, ograds = out if out is not None else (None, None)
    x0 = None
    if want_x0:
        x0 = ox0 if ox0 is not None else torch.empty(
            (dims.batch, weights[0].shape[0], dims.d), device=images.device, dtype=torch.float32)
    params = _fill(weights)
    grads = gstruct = None
    if dx0 is not None:
        grads = ograds if ograds is not None else [torch.empty_like(t) for t in weights]
        gstruct = _fill(grads)
    with torch.cuda.device(images.device):
        L.check(L.lib.vtd_stem_backward(
            ctypes.byref(dims), ctypes.byref(params), images.data_ptr(), L.ptr(dx0), L.ptr(x0),
            ctypes.byref(gstruct) if gstruct is not None else None, ws.data_ptr(), ws.numel(),
            L.stream_ptr()), "vtd_stem_backward")
    return x0, grads


def image_grad_workspace_bytes(dims: L.VtdStemDims) -> int:
    n = L.c_size_t(0)
    L.check(L.lib.vtd_stem_image_grad_workspace_bytes(ctypes.byref(dims), ctypes.byref(n)),
            "vtd_stem_image_grad_workspace_bytes")
    return int(n.value)


def image_grad(dx0, w, dims: L.VtdStemDims, ws=None, out=None):
    """vtd_stem_image_grad on contiguous fp32 device tensors: dx0 (B, N, d) = d loss / d x0 and
    w, the linear_projection kernel (patch_dim, d).  Returns d loss / d images, fp32 (B, H, W, C).
    ws: a uint8 workspace of at least image_grad_workspace_bytes(dims).  out: the caller's own
    output tensor in place of a new one."""
    if ws is None:
        ws = torch.empty(image_grad_workspace_bytes(dims), device=dx0.device, dtype=torch.uint8)
    dimages = out if out is not None else torch.empty(
        (dims.batch, dims.H, dims.W, dims.C), device=dx0.device, dtype=torch.float32)
    with torch.cuda.device(dx0.device):
        L.check(L.lib.vtd_stem_image_grad(
            ctypes.byref(dims), w.data_ptr(), dx0.data_ptr(), dimages.data_ptr(), ws.data_ptr(),
            ws.numel(), L.stream_ptr()), "vtd_stem_image_grad")
    return dimages


class _PatchEmbedding(torch.autograd.Function):
    """Forward: the C entry with dx0 = NULL, keeping the images and the weights only.  Backward:
    one C call that extracts the patches again and fills the weight gradients; with
    `image_gradient` and images that require grad, one vtd_stem_image_grad call as well."""

    @staticmethod
    def forward(ctx, images, dims, image_gradient, *weights):
        xd = images.detach()
        wd = [t.detach().contiguous() for t in weights]
        x0, _ = run(xd, wd, dims)
        ctx.dims = dims
        ctx.image_gradient = image_gradient
        ctx.save_for_backward(xd, *wd)
        return x0

    @staticmethod
    @once_differentiable
    def backward(ctx, gx0):
        xd, *wd = ctx.saved_tensors
        dx0 = gx0.to(torch.float32).reshape(xd.shape[0], -1, ctx.dims.d).contiguous()
        need = ctx.needs_input_grad
        _, grads = run(xd, wd, ctx.dims, dx0=dx0, want_x0=False)
        dimages = image_grad(dx0, wd[1], ctx.dims) if ctx.image_gradient and need[0] else None
        return (dimages, None, None) + tuple(g if n else None for g, n in zip(grads, need[3:]))


def patch_embedding(images, weights, *, patch_size, dtype="bf16x3", image_gradient=False):
    """The patch embedding (vtd.py:271-307), differentiable w.r.t. its three weights and, on
    request, its images.

    images: float32 device tensor (B, H, W, C).  weights: a sequence (or an OrderedDict, whose
    values are taken) of float32 device tensors in Keras creation order and shapes: the position
    embedding (tokens, 1) with tokens = ceil(H / patch_size) ceil(W / patch_size), the
    linear_projection kernel (patch_size^2 C, d) and bias (d,) (`Model.stem_weights` returns them
    so).  dtype: 'bf16x3' or 'bfloat16', the operand mode of the two products; x0 and every
    gradient are float32.  Returns x0 (B, tokens, d), the input of the first `encoder_block`;
    backward() makes one vtd_stem_backward call, bit-identical from run to run, with no
    synchronisation; weights that do not require grad get None.  image_gradient: False (the
    default) leaves `images.grad` None whatever the images require; True, with images that
    require grad, makes backward() also fill `images.grad` = d loss / d images, fp32 (B, H, W, C),
    with one vtd_stem_image_grad call (dx0 W^T in the mode's operands, then the adjoint of the
    patch extraction: the gradient that falls on the SAME zero pad is dropped), bit-identical from
    run to run.  The weight gradients and x0 have the same bits either way."""
    if isinstance(weights, dict):
        weights = list(weights.values())
    else:
        weights = list(weights)
    code = _dtype_code(dtype)
    if len(weights) != 3:
        raise ValueError("patch_embedding: weights must hold 3 tensors (position embedding, "
                         f"linear_projection kernel and bias), got {len(weights)}")
    if int(patch_size) < 1:
        raise ValueError("patch_embedding: patch_size must be positive")
    if not torch.is_tensor(images) or not images.is_cuda:
        raise ValueError("patch_embedding: images must be a device tensor")
    if images.dtype != torch.float32:
        raise ValueError(f"patch_embedding: images must be float32, got {images.dtype}")
    if images.dim() != 4 or images.numel() < 1:
        raise ValueError(f"patch_embedding: images {tuple(images.shape)} must be (B, H, W, C) "
                         "and not empty")
    B, H, W, C = images.shape
    if not torch.is_tensor(weights[1]) or weights[1].dim() != 2:
        raise ValueError("patch_embedding: weights[1] (linear_projection kernel) must be a "
                         "(patch_dim, d) tensor")
    d = int(weights[1].shape[1])
    shapes = weight_shapes(H, W, C, patch_size, d)
    for i, (label, t, shape) in enumerate(zip(_LABELS, weights, shapes)):
        what = f"weights[{i}] ({label})"
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"patch_embedding: {what} must be a device tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"patch_embedding: {what} must be float32, got {t.dtype}")
        if t.device != images.device:
            raise ValueError(f"patch_embedding: {what} must be on the images' device")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"patch_embedding: {what} has shape {tuple(t.shape)}, expected "
                             f"{shape}")
    dims = L.VtdStemDims(batch=B, H=H, W=W, C=C, patch=int(patch_size), d=d, dtype=code)
    return _PatchEmbedding.apply(images.contiguous(), dims, bool(image_gradient), *weights)
