"""Pins the CPU metric restatement (oracle/vtd_map.py) to the reference's own known-answer
tests (testcases_vision_transformer_detector.py:11-734)."""
import numpy as np
import pytest

from oracle import vtd_map as M
from tests.map_cases import CASES, case_3, case_4, case_5_2


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_map_known_answers(name):
    y, p, expected = CASES[name]()
    m = M.MeanAveragePrecision()
    m.update_state(y, p)
    # the reference asserts float32 equality (assertEqual on a float32 tensor)
    assert m.result() == np.float32(expected), (name, m.result(), expected)


def test_oracle_reset_state():
    """tests.py:713-734: after reset every state is zero and result() is 0."""
    m = M.MeanAveragePrecision()
    y, p, _ = CASES["11_two_categories_two_images"]()
    m.update_state(y, p)
    assert m.result() > 0
    m.reset_state()
    assert not m.latest_positive_bboxes.any()
    assert not m.labels_quantity_per_image.any()
    assert not m.showed_up_classes.any()
    assert m.result() == 0


def test_oracle_iou_values_of_the_kats():
    """The IoUs the reference tests print: 0.64 (test 3), 0.49 (test 4), 0.9801 (test 5.2)."""
    y, p, _ = case_3()
    assert abs(M.iou_calculator(y, p).max() - 0.64) < 1e-6
    y, p, _ = case_4()
    assert abs(M.iou_calculator(y, p).max() - 0.49) < 1e-6
    y, p, _ = case_5_2()
    iou = M.iou_calculator(np.broadcast_to(y[0, 1], p[0].shape), p[0])
    assert abs(iou[2] - 0.9801) < 1e-6 and iou[1] == np.float32(1.0)


def test_oracle_thresholds_float32():
    t = M.MeanAveragePrecision.thresholds()
    assert len(t) == 10 and t[0] == np.float32(0.5) and t[-1] == np.float32(0.95)
    assert all(a < b for a, b in zip(t, t[1:]))


def test_oracle_latest_related_images_window():
    """Only the LATEST_RELATED_IMAGES (3) most recent related images of a category are
    kept (vtd.py:1538-1544, 1856-1862): four updates, newest first in slot 0."""
    m = M.MeanAveragePrecision()
    for k in range(4):
        y, p, _ = CASES["1_one_image_one_category"]()
        y[0, 1, 4:] = 10 + k          # distinct sizes per image
        m.update_state(y, y)
    assert m.labels_quantity_per_image[79].tolist() == [1, 1, 1]
    assert np.allclose(m.latest_positive_bboxes[79, :, -1], 1.0, atol=1e-6)
    assert not m.latest_positive_bboxes[79, :, :-1].any()


def test_oracle_scenario_c_pads_at_end_and_scenario_d_at_front():
    m = M.MeanAveragePrecision()
    y = np.full((1, 10, 6), -8.0, np.float32)
    y[..., 0] = 0
    p = np.zeros((1, 10, 6), np.float32)
    p[0, 3] = (0.9, 5.2, 100, 100, 10, 10)      # category 5 predicted, not labelled
    m.update_state(y, p)
    e = m.latest_positive_bboxes[5, 0]
    assert e[0, 0] == M._confidence(np.float32(5.2)) and not e[1:].any()
    assert m.showed_up_classes[5] and m.labels_quantity_per_image[5, 0] == 0
    y, p, _ = CASES["1_one_image_one_category"]()
    m.update_state(y, p)
    e = m.latest_positive_bboxes[79, 0]
    assert e[-1].tolist() == [1.0, 1.0] and not e[:-1].any()


# ------------------------------------------------------------------ designed cases, by hand
# Four cases of tests/map_designs.py (one image of 17 rows, class 79 alone) derived from the
# reference's text, not from the restatement: the image's slot of latest_positive_bboxes, its
# label count, and the AP at IoU 0.5 and 0.95.  A class 79 + j / 256 has confidence
# (0.5 - j / 256) / 0.5 = 1 - j / 128 (vtd.py:1367-1376); a prediction hp high inside a label
# 32 high of the same width has IoU hp / 32.  oracle/vtd_map.py must meet them here, the device
# in tests/test_gpu_metrics.py.
F = np.float32


def _conf(j):
    return 1 - j / 128


def _ap(recall_precisions, labels):
    """vtd.py:1964-2000: the trapezoids under the recall-precision list, in float32."""
    acc = F(0)
    for top, bottom in zip(recall_precisions, recall_precisions[1:]):
        acc = F(acc + F(F(top) + F(bottom)))
    return F(F(acc * F(F(1) / F(labels))) / F(2))


DESIGNED_KAT = {
    # Scenario c (vtd.py:1560-1621).  Row i has j = (11 i + 3) mod 17: 17 distinct confidences.
    # 17 >= 14, so :1601-1612 sorts them descending and keeps [:14]: j = 0..13; IoUs are zeros
    # (:1615).  No label: count 0 (:1531-1536), and result() gives AP 0 without labels (:2005).
    "kat_c_over": dict(
        slot=[(_conf(j), 0.0) for j in range(14)], labels=0, ap50=F(0), ap95=F(0)),
    # Scenario d, 16 labels (vtd.py:1625-1758).  Label i is 8 + (5 i + 3) mod 16 wide and 32
    # high; :1646-1653 orders by ascending area, i = 9, 6, 3, 0, 13, 10, 7, 4, 1, 14, 11, 8, 5,
    # 2, 15, 12.  Each matches its own prediction (IoU (17 + i) / 32 > 0.5, confidence
    # 1 - i / 128), appended at the end (:1730-1738).  At the 14th hit :1756-1758 breaks:
    # labels 15 and 12 are never tried, and :1785-1788 (14 < 14 is false) drops the three
    # predictions left.  The count is all 16 (:1531).
    # AP at 0.5: 14 true positives, precision 1 each (:1928-1953), 1 / 16 per trapezoid.
    # At 0.95 only 31/32 (i = 14) counts; by descending confidence it is last, after 13 false
    # positives that each overwrite element 0 with 0 (:1951-1953), then 1 / 14 is appended.
    "kat_d_full": dict(
        slot=[(_conf(i), (17 + i) / 32) for i in (9, 6, 3, 0, 13, 10, 7, 4, 1, 14, 11, 8, 5, 2)],
        labels=16, ap50=_ap([1] * 15, 16), ap95=_ap([0, F(1) / F(14)], 16)),
    # Scenario d, 5 hits and 12 left-overs.  Label j is 12 - j wide: ascending area is j = 4,
    # 3, 2, 1, 0, with IoUs 17/32, 20/32, 24/32, 31/32, 1 and confidences 1 - (20 + j) / 128.
    # The 12 unmatched predictions stay >= 0 (vtd.py:1767-1771) with j = 0..11 in some order;
    # 5 + 12 > 14, so :1809-1827 sorts them descending and keeps 14 - 5 = 9: j = 0..8, IoU 0,
    # appended after the hits (:1843-1852).
    # result() sorts by confidence: the 9 left-overs (false positives) come first, then the
    # hits j = 0..4.  At 0.5 all five are true: precisions 1/10, 2/11, 3/12, 4/13, 5/14.  At
    # 0.95 j = 0 and 1 are: 1/10, 2/11, then three false positives overwrite 2/11 down to 2/14.
    "kat_d_cut": dict(
        slot=[(_conf(24), 17 / 32), (_conf(23), 20 / 32), (_conf(22), 24 / 32),
              (_conf(21), 31 / 32), (_conf(20), 1.0)] + [(_conf(m), 0.0) for m in range(9)],
        labels=5,
        ap50=_ap([0, F(1) / F(10), F(2) / F(11), F(3) / F(12), F(4) / F(13), F(5) / F(14)], 5),
        ap95=_ap([0, F(1) / F(10), F(2) / F(14)], 5)),
    # Equal areas.  C (16 x 16) is smallest and matches its own prediction (IoU 1, j = 2).
    # A (row 0) and B (row 1) are both 32 x 32 = 1024: tf.argsort (:1646) keeps row order on the
    # tie, A first.  A = y [64, 96]; P1 = [65, 97]: 31 x 32 = 992 over 2048 - 992 = 1056; P2 =
    # [72, 104]: 768 / 1280.  A takes P1 (j = 1), which is removed (:1750-1752).  B = [68, 100]
    # is left with P2 (j = 0): 28 x 32 = 896 over 1152 > 0.5.  Three entries: 11 zero pairs stay
    # in front (:1657, :1736-1738).  At 0.95 only C counts, after P2 and P1: [0, 1/3].
    "kat_equal_areas": dict(
        slot=[(0.0, 0.0)] * 11 + [(_conf(2), 1.0), (_conf(1), F(992) / F(1056)),
                                  (_conf(0), F(896) / F(1152))],
        labels=3, ap50=_ap([1, 1, 1, 1], 3), ap95=_ap([0, F(1) / F(3)], 3)),
}


def check_designed_kat(name, slot, labels, per_iou):
    """`slot`: (14, 2) entries of class 79's newest image; `per_iou`: the 10 APs."""
    want = DESIGNED_KAT[name]
    np.testing.assert_array_equal(np.asarray(slot, F), np.array(want["slot"], F))
    assert labels == want["labels"]
    assert F(per_iou[0]) == want["ap50"] and F(per_iou[9]) == want["ap95"], (name, per_iou)


@pytest.mark.parametrize("name", sorted(DESIGNED_KAT))
def test_oracle_meets_hand_derived_designed_cases(name):
    from tests.map_designs import CASES as DESIGNED
    (y, p), = DESIGNED[name]()[0]
    assert y.shape == (1, 17, 6)
    m = M.MeanAveragePrecision()
    m.update_state(y, p)
    assert m.showed_up_classes.nonzero()[0].tolist() == [79]
    check_designed_kat(name, m.latest_positive_bboxes[79, 0], m.labels_quantity_per_image[79, 0],
                       m.per_iou())
    assert not m.latest_positive_bboxes[79, 1:].any()
