"""numpy restatement of the reference's validation loss, for the tests:
iou_calculator, diagonal_calculator, ciou_calculator (vision_transformer_detector.py:761-1015)
and my_custom_loss (vtd.py:1122-1265), line by line, every array operation in `dtype`
(np.float64: the yardstick; np.float32: the reference's own arithmetic, whose distance from
the float64 result is the error a correct float32 implementation is allowed).

TensorFlow is not importable in this repository's environment, so two facts about what the
reference calls are restated from TF / Keras 2.9 and marked [upstream]:
 - keras.losses.BinaryCrossentropy / BinaryFocalCrossentropy(from_logits=False,
   label_smoothing=0, gamma=2, reduction=NONE) on (..., 1) inputs [upstream]:
     p_c = clip(p, 1e-7, 1 - 1e-7)
     bce = -(y log(p_c + 1e-7) + (1 - y) log(1 - p_c + 1e-7))
     focal: bce * (1 - p_t)^2 with p_t = y p + (1 - y)(1 - p) of the unclipped p;
   the mean over the size-1 last axis changes nothing.
 - tf.square(np.pi) converts the Python float to a float32 tensor first [upstream], so the
   reference's squared_pi is float32(pi) * float32(pi) rounded to float32 (9.869605), one
   ulp above float32(pi^2).  That float32 constant is part of the reference's definition
   and is used as is at either dtype.
Boxes are the LAST four channels (x, y, height, width) throughout, the centre included, so
that (..., 6) detection rows work as they do in iou_calculator.
"""
import numpy as np

EPSILON = 1e-8                      # Constants.EPSILON vtd.py:23
KERAS_EPSILON = 1e-7                # keras.backend.epsilon() [upstream]
SQUARED_PI = np.float32(np.pi) * np.float32(np.pi)       # vtd.py:992-994
CLASSES, MODEL_IMAGE_SIZE = 80, (608, 608)


def _edges(label_bbox, prediction_bbox, dtype):
    lb, pb = np.asarray(label_bbox, dtype), np.asarray(prediction_bbox, dtype)
    two = dtype(2)
    horizontal = np.stack([lb[..., -3] - lb[..., -2] / two, lb[..., -3] + lb[..., -2] / two,
                           pb[..., -3] - pb[..., -2] / two, pb[..., -3] + pb[..., -2] / two], -1)
    vertical = np.stack([lb[..., -4] - lb[..., -1] / two, lb[..., -4] + lb[..., -1] / two,
                         pb[..., -4] - pb[..., -1] / two, pb[..., -4] + pb[..., -1] / two], -1)
    return lb, pb, horizontal, vertical


def iou_calculator(label_bbox, prediction_bbox, dtype=np.float64):
    """vtd.py:761-875."""
    lb, pb, hor, ver = _edges(label_bbox, prediction_bbox, dtype)
    cond = ((ver[..., 0] < ver[..., 3]) & (ver[..., 1] > ver[..., 2]) &
            (hor[..., 0] < hor[..., 3]) & (hor[..., 1] > hor[..., 2]))[..., None]
    hor = np.sort(np.where(cond, hor, dtype(0)), -1)
    ver = np.sort(np.where(cond, ver, dtype(0)), -1)
    inter = (hor[..., -2] - hor[..., -3]) * (ver[..., -2] - ver[..., -3])
    union = pb[..., -1] * pb[..., -2] + lb[..., -1] * lb[..., -2] - inter
    return (inter / (union + dtype(EPSILON))).astype(dtype)


def diagonal_calculator(label_bbox, prediction_bbox, dtype=np.float64):
    """vtd.py:878-943."""
    _, _, hor, ver = _edges(label_bbox, prediction_bbox, dtype)
    hor, ver = np.sort(hor, -1), np.sort(ver, -1)
    h, w = hor[..., -1] - hor[..., 0], ver[..., -1] - ver[..., 0]
    return np.sqrt(h * h + w * w).astype(dtype)


def ciou_calculator(label_bbox, prediction_bbox, get_diou=None, dtype=np.float64):
    """vtd.py:946-1015."""
    lb, pb = np.asarray(label_bbox, dtype), np.asarray(prediction_bbox, dtype)
    eps = dtype(EPSILON)
    iou = iou_calculator(lb, pb, dtype)
    dx, dy = lb[..., -4] - pb[..., -4], lb[..., -3] - pb[..., -3]
    rho = np.sqrt(dx * dx + dy * dy)
    r_diou = np.square(rho / (diagonal_calculator(lb, pb, dtype) + eps))
    atan_label = np.arctan(lb[..., -1] / (lb[..., -2] + eps))
    atan_prediction = np.arctan(pb[..., -1] / (pb[..., -2] + eps))
    v = np.square(atan_label - atan_prediction) * dtype(4) / dtype(SQUARED_PI)
    alpha = v / ((dtype(1) - iou) + v + eps)
    r_ciou = r_diou + alpha * v
    if get_diou:
        return (iou - r_diou).astype(dtype)
    return (dtype(1) - iou + r_ciou).astype(dtype)


def transform_predictions(logits, dtype=np.float64):
    """vtd.py:586-647."""
    x = np.asarray(logits, dtype)
    with np.errstate(over="ignore"):             # exp(-x) = inf gives the sigmoid's exact 0
        s = dtype(1) / (dtype(1) + np.exp(-x))
    s[..., 2:] = np.clip(s[..., 2:], dtype(0), dtype(1))
    scale = np.array([1, CLASSES - 1, MODEL_IMAGE_SIZE[1], MODEL_IMAGE_SIZE[0],
                      MODEL_IMAGE_SIZE[0], MODEL_IMAGE_SIZE[1]], dtype)
    return (s * scale).astype(dtype)


def isclose(a, b, dtype):
    """tf.experimental.numpy.isclose: rtol 1e-5, atol 1e-8."""
    a, b = np.asarray(a, dtype), dtype(b)
    return np.abs(a - b) <= dtype(1e-8) + dtype(1e-5) * np.abs(b)


def my_custom_loss(y_true, y_pred, focal_binary_loss=True, coefficient=4, exponent=2,
                   weight_classification=0.0074, weight_ciou=10,
                   use_transform_predictions=True, dtype=np.float64):
    """vtd.py:1122-1265.  Returns (objectness mean, classification mean, CIoU mean, total)
    as `dtype` scalars.  Positive slots are decided on the float32 labels (what the reference
    holds) so both dtypes select the same slots."""
    positive = isclose(np.asarray(y_true, np.float32)[..., 0], 1.0, np.float32)
    y_true = np.asarray(y_true, dtype)
    y_pred = np.asarray(y_pred, dtype)
    if use_transform_predictions:
        y_pred = transform_predictions(y_pred, dtype)
    one, keps = dtype(1), dtype(KERAS_EPSILON)
    y, p = y_true[..., 0], y_pred[..., 0]
    p_c = np.clip(p, keps, one - keps)
    bce = y * np.log(p_c + keps)
    bce = bce + (one - y) * np.log(one - p_c + keps)
    bce = -bce
    if focal_binary_loss:
        p_t = y * p + (one - y) * (one - p)
        bce = np.power(one - p_t, dtype(2)) * bce
    objectness = np.mean(bce, dtype=dtype)
    if positive.any():
        error = np.abs(y_pred[..., 1][positive] - y_true[..., 1][positive])
        classification = np.mean((dtype(coefficient) * error) ** dtype(exponent), dtype=dtype)
        ciou = np.mean(ciou_calculator(y_true[..., -4:][positive], y_pred[..., -4:][positive],
                                       dtype=dtype), dtype=dtype)
    else:
        classification = ciou = dtype(0)
    total = objectness + classification * dtype(weight_classification) + ciou * dtype(weight_ciou)
    return dtype(objectness), dtype(classification), dtype(ciou), dtype(total)


# ---------------------------------------------------------------- inputs for the tests
def kat_case(change=None):
    """The reference's own fixtures (testcases_vision_transformer_detector.py:760-926): two
    images of 10 slots, one label [1, 79, 9, 9, 10, 10], every other row empty, the prediction
    a copy of the label with one change.  change: None | 'objectness' | 'class' | 'box'."""
    y_true = np.full((2, 10, 6), -8.0, np.float32)
    y_true[..., 0] = 0
    y_true[0, 0] = (1, 79, 9, 9, 10, 10)
    y_pred = y_true.copy()
    if change == "objectness":
        y_pred[0, 0, 0] = 0.98
    elif change == "class":
        y_pred[0, 0, 1] = 79.2
    elif change == "box":
        y_pred[0, 0, -4:] = (9, 9, 9.8, 9.8)
    elif change is not None:
        raise KeyError(change)
    return y_true, y_pred


def logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


def random_loss_batch(rng, batch, boxes, jitter=20.0, fill=None):
    """Seeded labels and LOGITS (the idea of map_cases.random_batch, for the loss): each
    image has a random number of objects in its first slots -- image 0 none, image 1 (when
    there is one) every slot, or `fill` objects in every image -- and the logits decode to
    the label's box moved by N(0, jitter) pixels, a class off by up to 1.5 and a confident
    objectness for positive slots, to anything for the rest."""
    y = np.full((batch, boxes, 6), -8.0, np.float32)
    y[..., 0] = 0.0
    dec = np.empty((batch, boxes, 6), np.float64)
    dec[..., 0] = rng.uniform(0.001, 0.6, (batch, boxes))
    dec[..., 1] = rng.uniform(0.0, 79.0, (batch, boxes))
    dec[..., 2:4] = rng.uniform(1.0, 607.0, (batch, boxes, 2))
    dec[..., 4:6] = rng.uniform(2.0, 300.0, (batch, boxes, 2))
    for b in range(batch):
        n = fill if fill is not None else (0 if b == 0 else boxes if b == 1
                                           else int(rng.integers(0, boxes + 1)))
        for i in range(n):
            h, w = rng.uniform(8, 300, 2)
            y[b, i] = (1.0, float(rng.integers(0, 80)), rng.uniform(60, 548),
                       rng.uniform(60, 548), h, w)
            dec[b, i, 0] = rng.uniform(0.3, 0.999)
            dec[b, i, 1] = np.clip(y[b, i, 1] + rng.uniform(-1.5, 1.5), 0.05, 78.95)
            dec[b, i, 2:] = y[b, i, 2:] + rng.normal(0, jitter, 4)
    dec[..., 2:] = np.clip(dec[..., 2:], 0.5, 607.5)
    scale = np.array([1, 79, 608, 608, 608, 608], np.float64)
    return y, logit(dec / scale).astype(np.float32)


def fp32_ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def allowed_error(y_true, y_pred, **kw):
    """The rule every device result is held to: at most 8x the float32 restatement's own
    error against float64 on this input, plus 4 float32 ulp of the value -- per component
    and for the total.  Returns (float64 values, bounds, float32 errors), 4-tuples in
    my_custom_loss's order."""
    ref = my_custom_loss(y_true, y_pred, dtype=np.float64, **kw)
    f32 = my_custom_loss(y_true, y_pred, dtype=np.float32, **kw)
    err = tuple(abs(float(a) - float(b)) for a, b in zip(f32, ref))
    bound = tuple(8.0 * e + 4.0 * fp32_ulp(r) for e, r in zip(err, ref))
    return ref, bound, err
