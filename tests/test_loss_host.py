"""Host-side tests of the loss feature, no GPU: get_label_arrays against the reference's
letterbox arithmetic (vision_transformer_utilities.py:268-382, 452-507), and the C-ABI of
vtd_loss / vtd_ciou through ctypes -- ABI version, struct layout, and every argument check,
all of which must answer before any device call."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vtd.h")
EMPTY = [0, -8, -8, -8, -8, -8]
IDS = [1, 2, 3, 5, 90]            # a caller's ordered COCO ids: index = model class


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def vtd():
    import vision_transformer_detector_amd as m
    return m


# ---------------------------------------------------------------- get_label_arrays
def test_labels_wide_image_shifts_y(vtd):
    """480 x 640 (h x w): resize_scale 640 / 608, blank (608 - 456) / 2 = 76 added to y."""
    lab = vtd.get_label_arrays([[3, 320, 240, 100, 200, 20000]], (480, 640), IDS)
    assert lab.shape == (17, 6) and lab.dtype == np.float32
    np.testing.assert_array_equal(lab[0], np.array([1, 2, 304, 304, 95, 190], np.float32))
    np.testing.assert_array_equal(lab[1:], np.tile(np.array(EMPTY, np.float32), (16, 1)))


def test_labels_tall_image_shifts_x(vtd):
    """640 x 480: the height scale wins and the blank goes to x."""
    lab = vtd.get_label_arrays([[90, 240, 320, 200, 100, 20000]], (640, 480), IDS)
    np.testing.assert_array_equal(lab[0], np.array([1, 4, 304, 304, 190, 95], np.float32))


def test_labels_square_image_adds_no_blank(vtd):
    lab = vtd.get_label_arrays([[1, 100, 50, 30, 40, 1200]], (1216, 1216), IDS)
    np.testing.assert_array_equal(lab[0], np.array([1, 0, 50, 25, 15, 20], np.float32))
    same = vtd.get_label_arrays([[1, 100, 50, 30, 40, 1200]], (608, 608), IDS)
    np.testing.assert_array_equal(same[0], np.array([1, 0, 100, 50, 30, 40], np.float32))


def test_labels_float64_then_float32(vtd):
    """The arithmetic runs in float64 and is cast once (vtd_utilities.py:358-374, 495)."""
    lab = vtd.get_label_arrays([[2, 101.5, 77.25, 33.3, 44.4, 1]], (427, 640), IDS)
    s = 640 / 608
    blank = (608 - 427 / s) / 2
    want = np.array([1, 1, 101.5 / s, 77.25 / s + blank, 33.3 / s, 44.4 / s]).astype(np.float32)
    np.testing.assert_array_equal(lab[0], want)


def test_labels_truncate_drop_and_empty(vtd):
    many = [[5, 10 + i, 20 + i, 4, 6, 24] for i in range(20)]
    lab = vtd.get_label_arrays(many, (608, 608), IDS)
    assert lab.shape == (17, 6) and (lab[:, 0] == 1).all() and (lab[:, 1] == 3).all()
    np.testing.assert_array_equal(lab[:, 2], np.arange(10, 27, dtype=np.float32))
    # an id outside the caller's list is dropped, the next object takes its row
    lab = vtd.get_label_arrays([[7, 1, 1, 1, 1, 1], [2, 30, 40, 10, 20, 200]], (608, 608), IDS)
    np.testing.assert_array_equal(lab[0], np.array([1, 1, 30, 40, 10, 20], np.float32))
    np.testing.assert_array_equal(lab[1], np.array(EMPTY, np.float32))
    for none in ([], None):
        lab = vtd.get_label_arrays(none, (480, 640), IDS)
        np.testing.assert_array_equal(lab, np.tile(np.array(EMPTY, np.float32), (17, 1)))
    assert vtd.get_label_arrays(many, (608, 608), IDS, max_boxes=3).shape == (3, 6)


# ---------------------------------------------------------------- C-ABI without a device
def test_abi_version_is_17(L):
    assert L.lib.vtd_abi_version() == 17 and L.ABI_VERSION == 17
    assert "#define VTD_ABI_VERSION 17" in open(HEADER).read()


def test_loss_params_struct_matches_header(L):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "vtd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(vtd_loss_params),
         offsetof(vtd_loss_params, focal_binary_loss), offsetof(vtd_loss_params, coefficient),
         offsetof(vtd_loss_params, exponent), offsetof(vtd_loss_params, weight_classification),
         offsetof(vtd_loss_params, weight_ciou), offsetof(vtd_loss_params, from_logits));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    P = L.VtdLossParams
    assert [int(v) for v in out] == [
        ctypes.sizeof(P), P.focal_binary_loss.offset, P.coefficient.offset, P.exponent.offset,
        P.weight_classification.offset, P.weight_ciou.offset, P.from_logits.offset]


def _params(L, **kw):
    base = dict(focal_binary_loss=1, coefficient=4.0, exponent=2.0, weight_classification=0.0074,
                weight_ciou=10.0, from_logits=1)
    base.update(kw)
    return L.VtdLossParams(**base)


def test_loss_argument_checks_need_no_device(L):
    """Non-null dummy pointers (1): every call is refused on the host before any use."""
    ok = _params(L)
    bad = [
        ("null y_true", (None, 1, 2, 10, ctypes.byref(ok), 1, None, None), b"null"),
        ("null y_pred", (1, None, 2, 10, ctypes.byref(ok), 1, None, None), b"null"),
        ("null out", (1, 1, 2, 10, ctypes.byref(ok), None, None, None), b"null"),
        ("null params", (1, 1, 2, 10, None, 1, None, None), b"null"),
        ("B < 0", (1, 1, -1, 10, ctypes.byref(ok), 1, None, None), b"B"),
        ("boxes 0", (1, 1, 2, 0, ctypes.byref(ok), 1, None, None), b"boxes"),
        ("boxes < 0", (1, 1, 2, -3, ctypes.byref(ok), 1, None, None), b"boxes"),
    ]
    for coefficient in (-1.0, float("inf"), float("-inf"), float("nan")):
        bad.append((f"coefficient {coefficient}",
                    (1, 1, 2, 10, ctypes.byref(_params(L, coefficient=coefficient)), 1, None, None),
                    b"coefficient"))
    for what, args, word in bad:
        assert L.lib.vtd_loss(*args) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(L.lib.vtd_loss(*args), "vtd_loss")


def test_ciou_argument_checks_need_no_device(L):
    assert L.lib.vtd_ciou(1, 1, -1, 4, 0, 1, None) == -1
    assert L.lib.vtd_ciou(1, 1, 8, 3, 0, 1, None) == -1
    assert b"stride" in L.lib.vtd_last_error()
    for args in ((None, 1, 8, 4, 0, 1, None), (1, None, 8, 6, 1, 1, None),
                 (1, 1, 8, 4, 0, None, None)):
        assert L.lib.vtd_ciou(*args) == -1
        assert b"null" in L.lib.vtd_last_error()
    assert L.lib.vtd_diagonal(None, 1, 8, 4, 1, None) == -1
    assert L.lib.vtd_diagonal(1, 1, 8, 2, 1, None) == -1
    # nothing to do: no launch, no error
    assert L.lib.vtd_ciou(None, None, 0, 4, 0, None, None) == 0


def test_python_api_checks_before_the_device(vtd):
    """Keyword handling of compile's loss and the coefficient check are host code."""
    from vision_transformer_detector_amd import loss as VL
    p = VL.fused_loss_params(functools.partial(vtd.my_custom_loss, coefficient=9, exponent=2,
                                               weight_ciou=4.5))
    assert (p.coefficient, p.exponent, p.weight_ciou, p.from_logits, p.focal_binary_loss) == \
        (9.0, 2.0, 4.5, 1, 1)
    assert p.weight_classification == np.float32(0.0074)
    d = VL.fused_loss_params(vtd.my_custom_loss)
    assert (d.coefficient, d.weight_ciou) == (4.0, 10.0)
    q = VL.fused_loss_params(functools.partial(vtd.my_custom_loss, focal_binary_loss=False,
                                               use_transform_predictions=False))
    assert (q.focal_binary_loss, q.from_logits) == (0, 0)
    assert VL.fused_loss_params(lambda y, p: 0.0) is None
    with pytest.raises(ValueError, match="coefficient"):
        VL.loss_params(coefficient=-2)
    with pytest.raises(TypeError):
        VL.fused_loss_params(functools.partial(vtd.my_custom_loss, gamma=3))
