"""Known answers for the numpy restatement of the reference's loss (tests/loss_oracle.py),
no GPU: the reference's own four my_custom_loss fixtures
(testcases_vision_transformer_detector.py:760-926) with hand-derived values, both
cross-entropy branches, a batch without positives, and ciou_calculator / get_diou /
diagonal_calculator on boxes whose terms can be worked out on paper."""
import math

import numpy as np
import pytest

from tests import loss_oracle as O

KW = dict(use_transform_predictions=False)


def test_identical_prediction_is_zero():
    """tests.py:768-789: the reference asserts isclose(total, 0), i.e. |total| <= 1e-8."""
    obj, cls, ciou, total = O.my_custom_loss(*O.kat_case(None), **KW)
    assert abs(total) <= 1e-8
    assert cls == 0 and abs(obj) <= 1e-8 and abs(ciou) <= 1e-8
    assert O.my_custom_loss(*O.kat_case(None), dtype=np.float32, **KW)[3] == 0


def test_objectness_case():
    """Objectness 0.98 on the one positive slot: p_t = 0.98, focal factor 0.02^2, every other
    slot contributes 0; the mean is over the 20 slots."""
    obj, cls, ciou, total = O.my_custom_loss(*O.kat_case("objectness"), **KW)
    expected = 0.02 ** 2 * -math.log(0.98 + 1e-7) / 20
    assert expected == pytest.approx(4.0405e-7, rel=1e-4)
    assert obj == pytest.approx(4.0405e-7, rel=1e-4)
    assert cls == 0
    # In float64 the identical boxes leave IoU = 100 / (100 + 1e-8), a box term of 1e-9
    # (the residue the identical-prediction case bounds by 1e-8), which is 0.25 % of this
    # case's value: the known answer is what the changed objectness adds to that case.  In
    # float32 -- the reference's own arithmetic -- the residue rounds away and the total is
    # the known answer itself.
    residue = O.my_custom_loss(*O.kat_case(None), **KW)[3]
    assert residue == pytest.approx(1e-9, rel=1e-3)
    assert total - residue == pytest.approx(4.0405e-7, rel=1e-4)
    total32 = O.my_custom_loss(*O.kat_case("objectness"), dtype=np.float32, **KW)[3]
    assert float(total32) == pytest.approx(4.0405e-7, rel=1e-4)


def test_class_case():
    """Class 79.2 against 79: (4 * 0.2)^2 * 0.0074 (float32 79.2 is inexact: rel 1e-4)."""
    obj, cls, ciou, total = O.my_custom_loss(*O.kat_case("class"), **KW)
    assert total == pytest.approx(4.736e-3, rel=1e-4)
    assert cls == pytest.approx(0.64, rel=1e-4)


def test_box_case():
    """Box (9, 9, 9.8, 9.8) inside (9, 9, 10, 10): IoU 0.9604, equal centres and aspect
    ratios, so 10 * (1 - 0.9604).  1 - iou cancels, hence an absolute bound; the float32
    evaluation gives 0.3960037."""
    obj, cls, ciou, total = O.my_custom_loss(*O.kat_case("box"), **KW)
    assert abs(total - 0.396) <= 1e-5
    assert abs(ciou - 0.0396) <= 1e-6
    total32 = O.my_custom_loss(*O.kat_case("box"), dtype=np.float32, **KW)[3]
    assert total32.dtype == np.float32 and abs(float(total32) - 0.396) <= 1e-5


def test_plain_cross_entropy_branch():
    """focal_binary_loss=False: the same slot's objectness term without the (1 - p_t)^2 factor."""
    plain = O.my_custom_loss(*O.kat_case("objectness"), focal_binary_loss=False, **KW)[0]
    assert plain == pytest.approx(-math.log(0.98 + 1e-7) / 20, rel=1e-6)
    focal = O.my_custom_loss(*O.kat_case("objectness"), **KW)[0]
    assert focal == pytest.approx(plain * 0.02 ** 2, rel=1e-6)


def test_objectness_on_an_empty_slot_and_clipping():
    """A confident false positive: y = 0, p = 0.9 -> 0.9^2 * -log(0.1 + 1e-7); p = 1 is
    clipped to 1 - 1e-7 inside the log only: 1^2 * -log(2e-7)."""
    y, p = O.kat_case(None)
    p[1, 3, 0] = 0.9
    p[1, 4, 0] = 1.0
    obj = O.my_custom_loss(y, p, **KW)[0]
    expected = (0.81 * -math.log(0.1 + 1e-7) + -math.log(2e-7)) / 20
    assert obj == pytest.approx(expected, rel=1e-6)


def test_no_positive_slot():
    """vtd.py:1249-1251: without a positive slot both means are 0, total = objectness mean;
    the -8 padding reaches no log / atan / division (no warning, nothing non-finite)."""
    y = np.full((3, 10, 6), -8.0, np.float32)
    y[..., 0] = 0
    p = y.copy()
    p[..., 0] = 0.3
    for dtype in (np.float64, np.float32):
        with np.errstate(all="raise"):
            obj, cls, ciou, total = O.my_custom_loss(y, p, dtype=dtype, **KW)
        assert cls == 0 and ciou == 0 and total == obj
        assert float(obj) == pytest.approx(0.09 * -math.log(0.7 + 1e-7), rel=1e-6)


def test_from_logits_decodes_first():
    """use_transform_predictions=True equals decoding the logits by hand."""
    rng = np.random.default_rng(0)
    y, logits = O.random_loss_batch(rng, 4, 10)
    a = O.my_custom_loss(y, logits)
    b = O.my_custom_loss(y, O.transform_predictions(logits), use_transform_predictions=False)
    assert a == b
    dec = O.transform_predictions(np.array([[0.0, 0.0, 50.0, -50.0, 0.0, 0.0]]))
    np.testing.assert_allclose(dec, [[0.5, 39.5, 608.0, 0.0, 304.0, 304.0]], atol=1e-12)


def test_parameters_scale_the_terms():
    """The notebook's parameters (ipynb:408-435): coefficient 9 scales the class mean by
    (9 / 4)^2, the weights enter the total linearly; exponent 4 is a real power."""
    rng = np.random.default_rng(1)
    y, logits = O.random_loss_batch(rng, 5, 17)
    obj, cls, ciou, total = O.my_custom_loss(y, logits)
    obj9, cls9, ciou9, total9 = O.my_custom_loss(y, logits, coefficient=9, weight_ciou=4.5)
    assert obj9 == obj and ciou9 == ciou
    assert cls9 == pytest.approx(cls * (9 / 4) ** 2, rel=1e-12)
    assert total9 == pytest.approx(obj + cls9 * 0.0074 + ciou * 4.5, rel=1e-12)
    y, p = O.kat_case("class")
    assert O.my_custom_loss(y, p, exponent=4, **KW)[1] == pytest.approx(0.8 ** 4, rel=1e-4)


def test_ciou_and_diou_by_hand():
    """Equal sizes, centres 3 right and 4 down: IoU 42 / 158, rho^2 = 25, enclosing box
    13 x 14, no aspect term."""
    lab = np.array([9.0, 9.0, 10.0, 10.0])
    pred = np.array([12.0, 13.0, 10.0, 10.0])
    iou, r_diou = 42 / 158, 25 / (13 ** 2 + 14 ** 2)
    assert O.iou_calculator(lab, pred) == pytest.approx(iou, rel=1e-9)
    assert O.diagonal_calculator(lab, pred) == pytest.approx(math.sqrt(365), rel=1e-12)
    assert O.ciou_calculator(lab, pred, get_diou=True) == pytest.approx(iou - r_diou, rel=1e-8)
    assert O.ciou_calculator(lab, pred) == pytest.approx(1 - iou + r_diou, rel=1e-8)
    # disjoint boxes: IoU 0, DIoU negative
    far = np.array([100.0, 9.0, 10.0, 10.0])
    assert O.iou_calculator(lab, far) == 0
    assert O.ciou_calculator(lab, far, get_diou=True) == pytest.approx(
        -(91 ** 2) / (101 ** 2 + 10 ** 2), rel=1e-8)


def test_ciou_aspect_term_by_hand():
    """Same centre, label 10 x 10 and prediction height 5, width 10: IoU 0.5, rho 0,
    v = (pi / 4 - atan 2)^2 * 4 / pi^2, alpha = v / (0.5 + v)."""
    lab = np.array([[0.0, 1.0, 9.0, 9.0, 10.0, 10.0]])            # 6-channel rows work too
    pred = np.array([[1.0, 2.0, 9.0, 9.0, 5.0, 10.0]])
    v = (math.pi / 4 - math.atan(2)) ** 2 * 4 / math.pi ** 2
    expected = 0.5 + v / (0.5 + v) * v
    assert O.ciou_calculator(lab, pred)[0] == pytest.approx(expected, rel=1e-6)
    assert O.ciou_calculator(lab, pred, get_diou=True)[0] == pytest.approx(0.5, rel=1e-8)


def test_float32_restatement_stays_float32_and_close():
    rng = np.random.default_rng(2)
    y, logits = O.random_loss_batch(rng, 8, 17)
    ref, bound, err = O.allowed_error(y, logits)
    f32 = O.my_custom_loss(y, logits, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in f32)
    assert all(e <= 1e-5 * abs(float(r)) for e, r in zip(err, ref))
    assert all(b >= 4 * O.fp32_ulp(r) for b, r in zip(bound, ref))
    assert O.ciou_calculator(y[..., 2:], O.transform_predictions(logits)[..., 2:],
                             dtype=np.float32).dtype == np.float32
