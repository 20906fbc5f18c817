"""Validation loss on the device, mirroring the reference's API.

`my_custom_loss` (vision_transformer_detector.py:1122-1265), `ciou_calculator` and
`diagonal_calculator` (vtd.py:878-1015) with the reference's names, arguments and defaults;
the work runs in libvtd.so (vtd_loss / vtd_ciou / vtd_diagonal, include/vtd.h): one launch
per batch, fp32 per-slot arithmetic in the reference's order, fp64 fixed-order sums.
`my_custom_loss`, `loss_components` (its total), `ciou_calculator` and
`transform_predictions` are differentiable w.r.t. the prediction: when the float32
prediction tensor requires grad (and grad mode is on) they run as torch.autograd.Functions
over the analytic gradient kernels (vtd_loss_grad / vtd_ciou_grad / vtd_decode_grad, first
derivatives only); otherwise they take the value-only path unchanged.  Labels are constants.
`loss_and_grad` returns the values and d loss / d prediction without autograd; from there
`Model.head_gradients` carries the gradient back through the detection head (vtd_head_backward:
the head's weight gradients and d loss / d encoded_images).  Backward through the encoder,
optimizers and `fit` are out of scope.  `get_label_arrays` (host only)
builds the reference's label rows (vision_transformer_utilities.py:268-382, 452-507).
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .metrics import _device_f32


def _pair(label_bbox, prediction_bbox, what):
    dev = prediction_bbox.device if torch.is_tensor(prediction_bbox) and \
        prediction_bbox.is_cuda else torch.device("cuda")
    lb, pb = _device_f32(label_bbox, dev), _device_f32(prediction_bbox, dev)
    if lb.shape != pb.shape or lb.dim() == 0 or lb.shape[-1] < 4:
        raise ValueError(f"{what}: shapes {tuple(lb.shape)} / {tuple(pb.shape)} must "
                         "match and end in >= 4 box channels")
    return dev, lb, pb, torch.empty(lb.shape[:-1], device=dev, dtype=torch.float32)


def ciou_calculator(label_bbox, prediction_bbox, get_diou=None):
    """vtd.py:946-1015: the CIoU loss 1 - IoU + r_diou + alpha * v of the boxes at matching
    positions, or the DIoU (IoU - r_diou) with `get_diou`.  Inputs as `iou_calculator`: the
    same shape (..., k), k >= 4, the last 4 channels (x, y, height, width).  Returns a (...)
    float32 tensor on the device, differentiable w.r.t. `prediction_bbox` (vtd_ciou_grad;
    the channels before the last four get a zero gradient)."""
    dev, lb, pb, out = _pair(label_bbox, prediction_bbox, "ciou_calculator")
    if _wants_grad(lb, pb, "ciou_calculator"):
        return _Ciou.apply(pb, lb, bool(get_diou))
    with torch.cuda.device(dev):
        L.check(L.lib.vtd_ciou(lb.data_ptr(), pb.data_ptr(), out.numel(), lb.shape[-1],
                               1 if get_diou else 0, out.data_ptr(), L.stream_ptr()), "vtd_ciou")
    return out


def diagonal_calculator(label_bbox, prediction_bbox):
    """vtd.py:878-943: the diagonal length of the smallest box enclosing each pair.  Inputs
    and result as `ciou_calculator`."""
    dev, lb, pb, out = _pair(label_bbox, prediction_bbox, "diagonal_calculator")
    with torch.cuda.device(dev):
        L.check(L.lib.vtd_diagonal(lb.data_ptr(), pb.data_ptr(), out.numel(), lb.shape[-1],
                                   out.data_ptr(), L.stream_ptr()), "vtd_diagonal")
    return out


def loss_params(focal_binary_loss=True, coefficient=4, exponent=2, weight_classification=0.0074,
                weight_ciou=10, use_transform_predictions=True) -> L.VtdLossParams:
    """my_custom_loss's keyword arguments as the C struct (vtd_loss_params)."""
    coefficient = float(coefficient)
    if not math.isfinite(coefficient) or coefficient < 0:
        raise ValueError(f"my_custom_loss: coefficient must be finite and >= 0, got {coefficient}")
    return L.VtdLossParams(focal_binary_loss=1 if focal_binary_loss else 0,
                           coefficient=coefficient, exponent=float(exponent),
                           weight_classification=float(weight_classification),
                           weight_ciou=float(weight_ciou),
                           from_logits=1 if use_transform_predictions else 0)


def _launch(yt, yp, params, running=None):
    """vtd_loss on the current stream of yt's device.  Returns the fp32 [5] device tensor."""
    out = torch.empty(5, device=yt.device, dtype=torch.float32)
    with torch.cuda.device(yt.device):
        L.check(L.lib.vtd_loss(yt.data_ptr(), yp.data_ptr(), yt.shape[0], yt.shape[1],
                               ctypes.byref(params), out.data_ptr(), L.ptr(running),
                               L.stream_ptr()), "vtd_loss")
    return out


def _wants_grad(label, pred, what):
    """The dispatch rule of every differentiable entry point: the gradient path when the
    float32 prediction tensor requires grad and grad mode is on, else the value-only one."""
    if not torch.is_grad_enabled():
        return False
    if label.requires_grad:
        raise ValueError(f"{what}: labels are constants; the label tensor requires grad")
    return pred.requires_grad


def _launch_grad(yt, yp, params, upstream=None):
    """vtd_loss_grad on the current stream of yt's device: (out5, d total / d yp)."""
    out = torch.empty(5, device=yt.device, dtype=torch.float32)
    grad = torch.empty_like(yp)
    with torch.cuda.device(yt.device):
        L.check(L.lib.vtd_loss_grad(yt.data_ptr(), yp.data_ptr(), yt.shape[0], yt.shape[1],
                                    ctypes.byref(params), L.ptr(upstream), out.data_ptr(),
                                    grad.data_ptr(), L.stream_ptr()), "vtd_loss_grad")
    return out, grad


class _Loss(torch.autograd.Function):
    """(total, the four reported values) with d total / d y_pred computed in the forward's
    own launch; backward is one multiply and never synchronises."""

    @staticmethod
    def forward(ctx, yp, yt, params):
        out, grad = _launch_grad(yt, yp.detach(), params)
        ctx.save_for_backward(grad)
        total, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, _g_parts):
        grad, = ctx.saved_tensors
        return grad * g_total, None, None


class _Ciou(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pb, lb, get_diou):
        pb = pb.detach()
        out = torch.empty(lb.shape[:-1], device=lb.device, dtype=torch.float32)
        with torch.cuda.device(lb.device):
            L.check(L.lib.vtd_ciou(lb.data_ptr(), pb.data_ptr(), out.numel(), lb.shape[-1],
                                   1 if get_diou else 0, out.data_ptr(), L.stream_ptr()), "vtd_ciou")
        ctx.save_for_backward(lb, pb)
        ctx.get_diou = get_diou
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lb, pb = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(pb)
        with torch.cuda.device(lb.device):
            L.check(L.lib.vtd_ciou_grad(lb.data_ptr(), pb.data_ptr(), g.numel(), lb.shape[-1],
                                        1 if ctx.get_diou else 0, g.data_ptr(), grad.data_ptr(),
                                        L.stream_ptr()), "vtd_ciou_grad")
        return grad, None, None


def _batch(y_true, y_pred, what):
    dev = y_pred.device if torch.is_tensor(y_pred) and y_pred.is_cuda else torch.device("cuda")
    yt, yp = _device_f32(y_true, dev), _device_f32(y_pred, dev)
    if yt.dim() != 3 or yt.shape[-1] != 6 or yt.shape != yp.shape or yt.shape[1] < 1:
        raise ValueError(f"{what}: y_true {tuple(yt.shape)} and y_pred {tuple(yp.shape)} must "
                         "both be (batch, boxes >= 1, 6)")
    return yt, yp


def loss_components(y_true, y_pred, focal_binary_loss=True, coefficient=4, exponent=2,
                    weight_classification=0.0074, weight_ciou=10,
                    use_transform_predictions=True):
    """my_custom_loss with its parts: a float32 [5] device tensor (total, objectness mean,
    classification mean, CIoU mean, number of positive slots).  No synchronisation.  Element
    0 is differentiable w.r.t. y_pred; the other four are reported values."""
    yt, yp = _batch(y_true, y_pred, "loss_components")
    if _wants_grad(yt, yp, "loss_components"):
        total, parts = _Loss.apply(yp, yt, loss_params(
            focal_binary_loss, coefficient, exponent, weight_classification, weight_ciou,
            use_transform_predictions))
        return torch.cat([total.reshape(1), parts])
    return _launch(yt, yp, loss_params(focal_binary_loss, coefficient, exponent,
                                       weight_classification, weight_ciou,
                                       use_transform_predictions))


def my_custom_loss(y_true, y_pred, focal_binary_loss=True,
                   coefficient=4, exponent=2,
                   weight_classification=0.0074, weight_ciou=10,
                   use_transform_predictions=True):
    """vtd.py:1122-1265.  y_true: (B, boxes, 6) labels (objectness, class, x, y, height,
    width; empty rows [0, -8, -8, -8, -8, -8]); y_pred: (B, boxes, 6) model logits, or decoded
    predictions with use_transform_predictions=False.  Returns the batch's loss as a 0-d
    float32 device tensor without synchronising: focal (or plain) binary cross-entropy of the
    objectness over every slot + weight_classification * mean (coefficient * |class
    error|)^exponent + weight_ciou * mean CIoU loss, the two means over the positive slots
    (0 when there are none).  Differentiable w.r.t. y_pred (first derivatives): when it
    requires grad the same launch also computes d loss / d y_pred (vtd_loss_grad) and
    backward multiplies it by the incoming gradient; exponent must then be >= 1."""
    yt, yp = _batch(y_true, y_pred, "my_custom_loss")
    if _wants_grad(yt, yp, "my_custom_loss"):
        return _Loss.apply(yp, yt, loss_params(
            focal_binary_loss, coefficient, exponent, weight_classification, weight_ciou,
            use_transform_predictions))[0]
    return _launch(yt, yp, loss_params(focal_binary_loss, coefficient, exponent,
                                       weight_classification, weight_ciou,
                                       use_transform_predictions))[0]


def loss_and_grad(y_true, y_pred, upstream=None, **kwargs):
    """(out5, grad) without autograd: loss_components' float32 [5] tensor -- the same bits --
    and d total / d y_pred, float32 of y_pred's shape (w.r.t. the logits, or the decoded
    predictions with use_transform_predictions=False), from one launch with no
    synchronisation.  `upstream`: an optional one-element float32 device tensor that
    multiplies the gradient on the device.  **kwargs: my_custom_loss's keywords, or
    params=<vtd_loss_params>."""
    yt, yp = _batch(y_true, y_pred, "loss_and_grad")
    params = kwargs.pop("params", None)
    if params is None:
        params = loss_params(**kwargs)
    elif kwargs:
        raise TypeError("loss_and_grad: params excludes the other keywords")
    if upstream is not None:
        upstream = _device_f32(upstream, yt.device)
        if upstream.numel() != 1:
            raise ValueError("loss_and_grad: upstream must hold one element")
    with torch.no_grad():
        return _launch_grad(yt, yp, params, upstream)


def fused_loss_params(loss):
    """The vtd_loss parameters of `loss` when it is my_custom_loss or a functools.partial of
    it with keyword arguments only (the notebook's compile pattern, ipynb:408-435), else
    None: Model.evaluate then calls `loss(y_true, logits)` per batch."""
    if loss is my_custom_loss:
        return loss_params()
    if isinstance(loss, functools.partial) and loss.func is my_custom_loss and not loss.args:
        return loss_params(**loss.keywords)     # an unknown keyword raises TypeError, as a call would
    return None


def get_label_arrays(annotations, image_original_size, category_ids,
                     model_image_size=(608, 608), max_boxes=17):
    """The reference's (max_boxes, 6) float32 label of one image
    (vision_transformer_utilities.py:268-382, 452-507), host only.

    annotations: [id_in_coco, centre x, centre y, height, width, area] per object, in
    original-image pixels (the reference's annotations_dict entries); image_original_size:
    (height, width); category_ids: the ordered COCO ids to detect, the index is the model's
    class (the reference's CATEGORIES_TO_DETECT table, which is its data and not shipped
    here) -- other ids are dropped.  Boxes are divided by resize_scale = max(width / W,
    height / H) and the letterbox blank is added to y when the width scale >= the height
    scale, else to x, in float64, so the rows line up with what get_image_tensors does to
    the pixels.  The first max_boxes objects are kept; empty rows are
    [0, -8, -8, -8, -8, -8]."""
    height, width = (float(v) for v in image_original_size)
    model_h, model_w = (float(v) for v in model_image_size)
    if height <= 0 or width <= 0:
        raise ValueError(f"get_label_arrays: image_original_size {image_original_size} must be positive")
    index = {int(c): i for i, c in reversed(list(enumerate(category_ids)))}
    width_scale, height_scale = width / model_w, height / model_h
    blank_in_height = blank_in_width = 0.0
    if width_scale > height_scale:
        resize_scale = width_scale
        blank_in_height = (model_h - height / resize_scale) / 2
    elif width_scale == height_scale:
        resize_scale = width_scale
    else:
        resize_scale = height_scale
        blank_in_width = (model_w - width / resize_scale) / 2
    labels = np.full((int(max_boxes), 6), -8.0, np.float64)
    labels[:, 0] = 0.0
    n = 0
    for one in annotations or ():
        if n == max_boxes:
            break
        cls = index.get(int(one[0]))
        if cls is None:
            continue
        x, y, h, w = (float(v) / resize_scale for v in one[1:5])
        if width_scale >= height_scale:
            y += blank_in_height
        else:
            x += blank_in_width
        labels[n] = (1.0, cls, x, y, h, w)
        n += 1
    return labels.astype(np.float32)
