"""The yardstick of the loss gradients, no GPU: the torch restatement
(tests/loss_grad_oracle.py) against the numpy one (tests/loss_oracle.py) -- forward values,
central finite differences, the reference's "box" fixture -- the near-kink mask's counts on
the batches the GPU tests use, and the three gradient entry points' argument checks through
ctypes, all of which must answer before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_grad_oracle as G
from tests import loss_oracle as O

SHAPES = [(1, 1), (3, 10), (8, 17), (37, 17), (256, 17)]


def batch(shape, jitter=20.0, seed=0):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    return O.random_loss_batch(rng, *shape, jitter=jitter)


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_agrees_with_numpy_restatement(shape):
    y, logits = batch(shape)
    want = O.my_custom_loss(y, logits)
    got = G.my_custom_loss(y, torch.tensor(logits, dtype=torch.float64))
    for w, g in zip(want, got):
        assert abs(float(g) - float(w)) <= 1e-14 * abs(float(w))


def test_autograd_matches_finite_differences_of_the_numpy_oracle():
    """Central differences, step 1e-5, float64, every coordinate of the (3, 10) batch: within
    1e-7 of the channel's largest |gradient| (measured 1.8e-9)."""
    y, logits = batch((3, 10))
    _, grad = G.loss_and_grad(y, logits)
    x = logits.astype(np.float64)
    fd = np.empty_like(x)
    h = 1e-5
    for idx in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[idx] += h
        lo[idx] -= h
        fd[idx] = (O.my_custom_loss(y, hi)[3] - O.my_custom_loss(y, lo)[3]) / (2 * h)
    top = np.abs(grad).reshape(-1, 6).max(0)
    worst = (np.abs(fd - grad).reshape(-1, 6).max(0) / top).max()
    print(f"finite differences: worst error / channel maximum {worst:.3g}")
    assert (np.abs(fd - grad) <= 1e-7 * top).all()


def test_box_fixture_gradient():
    """Coincident centres: autodiff of the reference's sqrt gives NaN in x and y; the
    restatement's (dx^2 + dy^2) / (c + eps)^2 gives 0 (the documented deviation), and
    d (10 (1 - h w / 100)) / dh = -0.98."""
    y, p = O.kat_case("box")
    _, grad = G.loss_and_grad(y, p, use_transform_predictions=False)
    assert np.isfinite(grad).all()
    np.testing.assert_allclose(grad[0, 0], [0, 0, 0, 0, -0.98, -0.98], atol=1e-6, rtol=0)
    assert not grad[0, 1:, 1:].any() and not grad[1, :, 1:].any()


def test_near_kink_counts():
    """No slot of the seeded batches is near a kink (smallest margin 1.6e-3, at (256, 17));
    the near-coincident batch has 18 of 320: at most 10 %."""
    least = np.inf
    for shape in SHAPES:
        y, logits = batch(shape)
        kinked, margin = G.near_kink(y, logits)
        assert not kinked.any(), shape
        least = min(least, margin.min())
    y, logits = batch((37, 17), jitter=0.05, seed=1)
    kinked, _ = G.near_kink(y, logits)
    positive = O.isclose(y[..., 0], 1.0, np.float32)
    print(f"smallest margin {least:.3g}; near-coincident {kinked.sum()} of {positive.sum()}")
    assert not (kinked & ~positive).any()
    assert 0 < kinked.sum() <= 0.1 * positive.sum()
    # the fixtures sit on kinks: identical edges, a zero class error
    assert G.near_kink(*O.kat_case("box"), use_transform_predictions=False)[0][0, 0]


# ---------------------------------------------------------------- C-ABI without a device
def _params(L, **kw):
    base = dict(focal_binary_loss=1, coefficient=4.0, exponent=2.0, weight_classification=0.0074,
                weight_ciou=10.0, from_logits=1)
    base.update(kw)
    return L.VtdLossParams(**base)


def test_symbols_and_abi_version(L):
    for name in ("vtd_loss_grad", "vtd_ciou_grad", "vtd_decode_grad"):
        assert callable(getattr(L.lib, name)) and name in L.SIGNATURES
    assert L.lib.vtd_abi_version() == 17 and L.ABI_VERSION == 17


def test_loss_grad_argument_checks_need_no_device(L):
    """Non-null dummy pointers (1): every call is refused on the host before any use.
    Arguments: y_true, y_pred, B, boxes, params, upstream, out5, grad, stream."""
    ok = ctypes.byref(_params(L))
    bad = [
        ("null y_true", (None, 1, 2, 10, ok, None, 1, 1, None), b"null"),
        ("null y_pred", (1, None, 2, 10, ok, None, 1, 1, None), b"null"),
        ("null out5", (1, 1, 2, 10, ok, None, None, 1, None), b"null"),
        ("null grad", (1, 1, 2, 10, ok, None, 1, None, None), b"null"),
        ("null params", (1, 1, 2, 10, None, None, 1, 1, None), b"null"),
        ("B < 0", (1, 1, -1, 10, ok, None, 1, 1, None), b"B"),
        ("boxes 0", (1, 1, 2, 0, ok, None, 1, 1, None), b"boxes"),
        ("boxes < 0", (1, 1, 2, -3, ok, None, 1, 1, None), b"boxes"),
    ]
    for coefficient in (-1.0, float("inf"), float("nan")):
        bad.append((f"coefficient {coefficient}",
                    (1, 1, 2, 10, ctypes.byref(_params(L, coefficient=coefficient)), None, 1, 1,
                     None), b"coefficient"))
    for exponent in (0.5, 0.0, -2.0, float("inf"), float("nan")):
        bad.append((f"exponent {exponent}",
                    (1, 1, 2, 10, ctypes.byref(_params(L, exponent=exponent)), None, 1, 1, None),
                    b"exponent"))
    for what, args, word in bad:
        assert L.lib.vtd_loss_grad(*args) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(L.lib.vtd_loss_grad(*args), "vtd_loss_grad")
    # the forward entry point still takes an exponent below 1: nothing existing changes
    assert L.lib.vtd_loss(None, 1, 2, 10, ctypes.byref(_params(L, exponent=0.5)), 1, None,
                          None) == -1
    assert b"null" in L.lib.vtd_last_error()


def test_ciou_and_decode_grad_argument_checks_need_no_device(L):
    """vtd_ciou_grad(label, pred, n, stride, get_diou, upstream, grad, stream);
    vtd_decode_grad(logits, upstream, n, grad, stream)."""
    assert L.lib.vtd_ciou_grad(1, 1, -1, 4, 0, None, 1, None) == -1
    assert L.lib.vtd_ciou_grad(1, 1, 8, 3, 0, None, 1, None) == -1
    assert b"stride" in L.lib.vtd_last_error()
    for args in ((None, 1, 8, 4, 0, None, 1, None), (1, None, 8, 6, 1, 1, 1, None),
                 (1, 1, 8, 4, 0, None, None, None)):
        assert L.lib.vtd_ciou_grad(*args) == -1
        assert b"null" in L.lib.vtd_last_error()
    for args in ((None, 1, 8, 1, None), (1, None, 8, 1, None), (1, 1, 8, None, None)):
        assert L.lib.vtd_decode_grad(*args) == -1
        assert b"null" in L.lib.vtd_last_error()
    assert L.lib.vtd_decode_grad(1, 1, -1, 1, None) == -1
    # nothing to do: no launch, no error
    assert L.lib.vtd_ciou_grad(None, None, 0, 4, 0, None, None, None) == 0
    assert L.lib.vtd_decode_grad(None, None, 0, None, None) == 0
