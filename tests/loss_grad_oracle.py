"""torch restatement of tests/loss_oracle.py, for the gradient tests: the same lines with
torch.sort / torch.where / torch.clamp, parameterised by dtype, so that torch.autograd
differentiates the reference's own graph.  torch.float64 is the yardstick; torch.float32 is
the error a correct float32 implementation is allowed.

One line differs from the numpy restatement, on purpose: r_diou is written
(dx^2 + dy^2) / (c + eps)^2 instead of square(sqrt(dx^2 + dy^2) / (c + eps)).  The value is
the same; the derivative of the sqrt form is 0/0 = NaN at coincident centres (the reference's
own "box" fixture), the derivative of this form is 0 there and equal everywhere else.
torch.sort runs with stable=True so that tied edges route their gradient the same way at
either dtype (min: the first of the tied entries, max: the last).  The decode's sigmoid
carries TensorFlow's registered gradient s (1 - s) (_Sigmoid)."""
import numpy as np
import torch

from tests import loss_oracle as O

KINK_MARGIN = 1e-3
SCALE = (1.0, O.CLASSES - 1.0, O.MODEL_IMAGE_SIZE[1], O.MODEL_IMAGE_SIZE[0],
         O.MODEL_IMAGE_SIZE[0], O.MODEL_IMAGE_SIZE[1])


def _edges(lb, pb):
    horizontal = torch.stack([lb[..., -3] - lb[..., -2] / 2, lb[..., -3] + lb[..., -2] / 2,
                              pb[..., -3] - pb[..., -2] / 2, pb[..., -3] + pb[..., -2] / 2], -1)
    vertical = torch.stack([lb[..., -4] - lb[..., -1] / 2, lb[..., -4] + lb[..., -1] / 2,
                            pb[..., -4] - pb[..., -1] / 2, pb[..., -4] + pb[..., -1] / 2], -1)
    return horizontal, vertical


def iou_calculator(lb, pb):
    hor, ver = _edges(lb, pb)
    cond = ((ver[..., 0] < ver[..., 3]) & (ver[..., 1] > ver[..., 2]) &
            (hor[..., 0] < hor[..., 3]) & (hor[..., 1] > hor[..., 2]))[..., None]
    zero = torch.zeros((), dtype=lb.dtype)
    hor = torch.sort(torch.where(cond, hor, zero), stable=True, dim=-1).values
    ver = torch.sort(torch.where(cond, ver, zero), stable=True, dim=-1).values
    inter = (hor[..., -2] - hor[..., -3]) * (ver[..., -2] - ver[..., -3])
    union = pb[..., -1] * pb[..., -2] + lb[..., -1] * lb[..., -2] - inter
    return inter / (union + O.EPSILON)


def diagonal_calculator(lb, pb):
    hor, ver = _edges(lb, pb)
    hor = torch.sort(hor, stable=True, dim=-1).values
    ver = torch.sort(ver, stable=True, dim=-1).values
    h, w = hor[..., -1] - hor[..., 0], ver[..., -1] - ver[..., 0]
    return torch.sqrt(h * h + w * w)


def ciou_calculator(label_bbox, prediction_bbox, get_diou=None):
    """Tensors of one dtype, shape (..., k >= 4)."""
    lb, pb = label_bbox, prediction_bbox
    eps = O.EPSILON
    iou = iou_calculator(lb, pb)
    dx, dy = lb[..., -4] - pb[..., -4], lb[..., -3] - pb[..., -3]
    r_diou = (dx * dx + dy * dy) / torch.square(diagonal_calculator(lb, pb) + eps)
    atan_label = torch.atan(lb[..., -1] / (lb[..., -2] + eps))
    atan_prediction = torch.atan(pb[..., -1] / (pb[..., -2] + eps))
    squared_pi = torch.tensor(float(O.SQUARED_PI), dtype=lb.dtype)
    v = torch.square(atan_label - atan_prediction) * 4 / squared_pi
    alpha = v / ((1 - iou) + v + eps)
    r_ciou = r_diou + alpha * v
    if get_diou:
        return iou - r_diou
    return 1 - iou + r_ciou


class _Sigmoid(torch.autograd.Function):
    """keras.activations.sigmoid (vtd.py:619): the value as loss_oracle writes it, the
    gradient as TensorFlow registers it for Sigmoid [upstream]: dy * s * (1 - s) of the
    OUTPUT.  Autodiff of 1 / (1 + exp(-x)) itself gives exp(-x) s^2 instead, which is the
    same number except where s has rounded to 1: there the reference's gradient is exactly 0."""

    @staticmethod
    def forward(ctx, x):
        s = 1 / (1 + torch.exp(-x))
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return g * (s * (1 - s))


def transform_predictions(x):
    s = _Sigmoid.apply(x)
    s = torch.cat([s[..., :2], torch.clamp(s[..., 2:], 0, 1)], -1)
    return s * torch.tensor(SCALE, dtype=x.dtype)


def positives(y_true):
    return torch.from_numpy(O.isclose(np.asarray(y_true, np.float32)[..., 0], 1.0, np.float32))


def my_custom_loss(y_true, y_pred, focal_binary_loss=True, coefficient=4, exponent=2,
                   weight_classification=0.0074, weight_ciou=10,
                   use_transform_predictions=True):
    """y_true: array; y_pred: a torch tensor whose dtype is the dtype of every operation.
    Returns (objectness mean, classification mean, CIoU mean, total) as 0-d tensors."""
    dtype = y_pred.dtype
    positive = positives(y_true)
    y_true = torch.tensor(np.asarray(y_true, np.float32)).to(dtype)
    if use_transform_predictions:
        y_pred = transform_predictions(y_pred)
    keps = O.KERAS_EPSILON
    y, p = y_true[..., 0], y_pred[..., 0]
    p_c = torch.clamp(p, keps, 1 - keps)
    bce = y * torch.log(p_c + keps)
    bce = bce + (1 - y) * torch.log(1 - p_c + keps)
    bce = -bce
    if focal_binary_loss:
        p_t = y * p + (1 - y) * (1 - p)
        bce = torch.pow(1 - p_t, 2) * bce
    objectness = bce.mean()
    if bool(positive.any()):
        error = torch.abs(y_pred[..., 1][positive] - y_true[..., 1][positive])
        classification = torch.pow(coefficient * error, exponent).mean()
        ciou = ciou_calculator(y_true[..., -4:][positive], y_pred[..., -4:][positive]).mean()
    else:
        classification = ciou = torch.zeros((), dtype=dtype)
    total = objectness + classification * weight_classification + ciou * weight_ciou
    return objectness, classification, ciou, total


def loss_and_grad(y_true, y_pred, dtype=torch.float64, **kw):
    """(the four values as floats, d total / d y_pred as a float64 numpy array)."""
    x = torch.tensor(np.asarray(y_pred), dtype=dtype, requires_grad=True)
    values = my_custom_loss(y_true, x, **kw)
    values[3].backward()
    return tuple(float(v.detach()) for v in values), x.grad.numpy().astype(np.float64)


def ciou_grad(label, pred, upstream=None, get_diou=None, dtype=torch.float64):
    """d sum(upstream * ciou_calculator) / d pred, float64 numpy, pred's shape."""
    lb = torch.tensor(np.asarray(label), dtype=dtype)
    pb = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    out = ciou_calculator(lb, pb, get_diou)
    up = torch.ones_like(out) if upstream is None else torch.tensor(np.asarray(upstream), dtype=dtype)
    (out * up).sum().backward()
    return pb.grad.numpy().astype(np.float64)


def edge_margin(label, pred):
    """The least of the eight label-edge / prediction-edge distances (near-near, far-far,
    near-far, far-near on both axes) of float64 (..., k >= 4) boxes: how far a pair is from
    two edges changing order, where the sorts and the intersect condition have their kinks."""
    y, d = np.asarray(label, np.float64), np.asarray(pred, np.float64)
    margin = np.full(y.shape[:-1], np.inf)
    for centre, size in ((-4, -1), (-3, -2)):
        for a in (y[..., centre] - y[..., size] / 2, y[..., centre] + y[..., size] / 2):
            for b in (d[..., centre] - d[..., size] / 2, d[..., centre] + d[..., size] / 2):
                margin = np.minimum(margin, np.abs(a - b))
    return margin


def near_kink(y_true, y_pred, use_transform_predictions=True):
    """(mask, margin) over the slots, True where a POSITIVE slot lies within KINK_MARGIN of a
    point where the loss is not differentiable and either one-sided derivative is right: two
    edges of the label and the prediction on one axis changing order, or the class error
    changing sign.  d = the float64 decoded prediction; the margin is the least of
    edge_margin and 10 |d_class - y_class|."""
    y = np.asarray(y_true, np.float64)
    d = np.asarray(y_pred, np.float64)
    if use_transform_predictions:
        d = O.transform_predictions(d, np.float64)
    positive = O.isclose(np.asarray(y_true, np.float32)[..., 0], 1.0, np.float32)
    margin = np.minimum(10.0 * np.abs(d[..., 1] - y[..., 1]), edge_margin(y, d))
    margin = np.where(positive, margin, np.inf)
    return margin < KINK_MARGIN, margin


def channel_bound(g64, g32, keep):
    """Per channel (the last axis) over the kept elements: (8 x the float32 gradient's
    largest error + 4 float32 ulp of the largest |float64 gradient|, that float32 error)."""
    keep = np.broadcast_to(keep, g64.shape)
    k = g64.shape[-1]
    err32 = np.where(keep, np.abs(g32 - g64), 0.0).reshape(-1, k).max(0)
    top = np.where(keep, np.abs(g64), 0.0).reshape(-1, k).max(0)
    return np.array([8.0 * e + 4.0 * O.fp32_ulp(t) for e, t in zip(err32, top)]), err32


def gradient_rule(y_true, y_pred, keep=None, **kw):
    """The rule a device gradient is held to.  Returns (float64 gradient, keep, bound [6],
    float32 error [6]).  keep (B, boxes, 1 or 6) marks what is held to the bound: by default
    the slots that are not near a kink.  Per channel, over the kept elements, bound = 8 x the
    float32 restatement's largest error + 4 float32 ulp of the channel's largest |float64
    gradient|."""
    _, g64 = loss_and_grad(y_true, y_pred, torch.float64, **kw)
    _, g32 = loss_and_grad(y_true, y_pred, torch.float32, **kw)
    if keep is None:
        keep = ~near_kink(y_true, y_pred, kw.get("use_transform_predictions", True))[0][..., None]
    keep = np.broadcast_to(keep, g64.shape)
    bound, err32 = channel_bound(g64, g32, keep)
    return g64, keep, bound, err32
