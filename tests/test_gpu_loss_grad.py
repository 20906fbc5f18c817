"""Loss gradients on the device (vtd_loss_grad / vtd_ciou_grad / vtd_decode_grad, the
torch.autograd path of loss.py, Model.loss_and_grad) against float64 autograd of the torch
restatement of the reference (tests/loss_grad_oracle.py).

The rule follows the forward's (test_gpu_loss.py): per channel, over the slots that are not
within 1e-3 of a kink (loss_grad_oracle.near_kink: either one-sided derivative is right
there), |device - float64| <= 8 x the float32 restatement's own largest error on that
channel + 4 float32 ulp of the channel's largest |float64 gradient|.  Every element is
finite, the excluded slots included, and non-positive slots are exactly 0 in channels 1..5.
Each check prints its device / float32 error ratio per channel."""
import functools

import numpy as np
import pytest
import torch

from tests import loss_grad_oracle as G
from tests import loss_oracle as O

pytestmark = pytest.mark.gpu

NOTEBOOK = dict(coefficient=9, weight_ciou=4.5)                      # ipynb:408-435
SHAPES = [(1, 1), (3, 10), (8, 17), (37, 17), (256, 17)]
DECODED = dict(use_transform_predictions=False)


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@functools.lru_cache(maxsize=None)
def batch(shape, jitter=20.0, seed=0):
    """The seeded (labels, logits) pairs of test_gpu_loss.py, shared and left unchanged."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    y, logits = O.random_loss_batch(rng, *shape, jitter=jitter)
    y.setflags(write=False)
    logits.setflags(write=False)
    return y, logits


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()


def device_grad(vtd, y, p, **kw):
    """loss_and_grad's gradient as numpy; its out5 must be vtd_loss's, bit for bit."""
    yt, pt = dev(y), dev(p)
    out5, grad = vtd.loss_and_grad(yt, pt, **kw)
    assert grad.shape == pt.shape and grad.dtype == torch.float32 and grad.is_cuda
    assert out5.cpu().numpy().tobytes() == vtd.loss_components(yt, pt, **kw).cpu().numpy().tobytes()
    return grad.cpu().numpy()


def check_rule(what, got, y, p, keep=None, **kw):
    g64, keep, bound, err32 = G.gradient_rule(y, p, keep=keep, **kw)
    assert np.isfinite(got).all(), what
    positive = O.isclose(np.asarray(y, np.float32)[..., 0], 1.0, np.float32)
    assert not got[~positive][:, 1:].any(), what
    err = np.where(keep, np.abs(got - g64), 0.0).reshape(-1, 6).max(0)
    ratio = [f"{e / f:.3g}" if f else ("0" if not e else "inf") for e, f in zip(err, err32)]
    print(f"{what}: device err {err} float32 err {err32} ratio {ratio} bound {bound} "
          f"excluded slots {(~keep[..., 0]).sum()}")
    assert (err <= bound).all(), (what, err, bound)


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("params", [{}, NOTEBOOK], ids=["defaults", "notebook"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gradient_matches_float64_autograd(vtd, cuda, shape, params):
    """(37, 17): a part-filled wave and idle ones; (256, 17): 4.25 trips of the workgroup in
    both phases.  Every shape but (1, 1) holds an image without positives."""
    y, logits = batch(shape)
    check_rule(f"{shape} {params}", device_grad(vtd, y, logits, **params), y, logits, **params)


@pytest.mark.parametrize("focal,exponent", [(False, 2), (True, 4), (True, 2.5)])
def test_gradient_other_branches(vtd, cuda, focal, exponent):
    """Plain cross-entropy, and exponents whose derivative takes powf."""
    y, logits = batch((8, 17))
    kw = dict(focal_binary_loss=focal, exponent=exponent)
    check_rule(f"focal={focal} exponent={exponent}", device_grad(vtd, y, logits, **kw), y, logits,
               **kw)


def test_gradient_decoded_mode(vtd, cuda):
    """use_transform_predictions=False: the gradient w.r.t. the decoded predictions."""
    y, logits = batch((8, 17))
    dec = O.transform_predictions(logits, np.float32)
    check_rule("decoded", device_grad(vtd, y, dec, **DECODED), y, dec, **DECODED)


def test_known_answers(vtd, cuda):
    """The reference's fixtures, decoded mode, against the float64 values.  Each sits on
    kinks (identical edges; a zero class error in "box" and "objectness"), where any
    one-sided derivative is right: those channels of the positive slot must be finite, the
    others meet the rule.  "box" has coincident centres: (0, 0, 0, 0, -0.98, -0.98), the x
    and y zeros being the documented deviation from autodiff of the reference's sqrt."""
    smooth = {"box": [0, 2, 3, 4, 5], "class": [0, 1], "objectness": [0]}
    for case, channels in smooth.items():
        y, p = O.kat_case(case)
        keep = np.ones(y.shape, bool)
        keep[0, 0] = False
        keep[0, 0, channels] = True
        got = device_grad(vtd, y, p, **DECODED)
        check_rule(case, got, y, p, keep=keep, **DECODED)
        if case == "box":
            np.testing.assert_allclose(got[0, 0], [0, 0, 0, 0, -0.98, -0.98], atol=1e-6, rtol=0)
            assert got[0, 0, 2] == 0 and got[0, 0, 3] == 0
        if case == "class":
            assert got[0, 0, 1] == pytest.approx(2 * 16 * (np.float32(79.2) - 79) * 0.0074, rel=1e-5)


def test_two_runs_and_upstream(vtd, cuda):
    """The gradient is bit-identical from run to run; a device scalar `upstream` multiplies
    it (a power of two: exactly) and leaves out5 alone; B = 0 zeroes out5 only."""
    y, logits = batch((256, 17))
    yt, lg = dev(y), dev(logits)
    out_a, a = vtd.loss_and_grad(yt, lg, **NOTEBOOK)
    out_b, b = vtd.loss_and_grad(yt, lg, **NOTEBOOK)
    assert torch.equal(a, b) and torch.equal(out_a, out_b)
    out_c, c = vtd.loss_and_grad(yt, lg, upstream=torch.tensor([0.5], device=cuda), **NOTEBOOK)
    assert torch.equal(c, a * 0.5) and torch.equal(out_c, out_a)
    out5, grad = vtd.loss_and_grad(np.zeros((0, 17, 6)), np.zeros((0, 17, 6)))
    assert out5.cpu().tolist() == [0.0] * 5 and grad.shape == (0, 17, 6)
    with pytest.raises(ValueError, match="exponent"):
        vtd.loss_and_grad(yt, lg, exponent=0.5)
    with pytest.raises(ValueError):
        vtd.loss_and_grad(yt, lg[:, :10])


# ---------------------------------------------------------------- torch.autograd
def test_autograd_backward_and_scaling(vtd, cuda):
    y, logits = batch((8, 17))
    yt = dev(y)
    _, want = vtd.loss_and_grad(yt, dev(logits))
    x = dev(logits).requires_grad_()
    loss = vtd.my_custom_loss(yt, x)
    assert loss.requires_grad and loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    assert torch.equal(x.grad, want)
    x.grad = None
    (3 * vtd.my_custom_loss(yt, x)).backward()                 # upstream scaling
    assert torch.equal(x.grad, want * 3)
    # loss_components: element 0 carries the gradient, the rest are reported values
    x.grad = None
    parts = vtd.loss_components(yt, x)
    assert parts.shape == (5,) and parts.requires_grad
    assert torch.equal(parts.detach(), vtd.loss_components(yt, dev(logits)))
    parts[0].backward()
    assert torch.equal(x.grad, want)
    x.grad = None
    vtd.loss_components(yt, x)[1:].sum().backward()
    assert not x.grad.any()
    # a bf16 prediction chains through its own .float()
    xb = dev(logits).to(torch.bfloat16).requires_grad_()
    vtd.my_custom_loss(yt, xb).backward()
    _, wb = vtd.loss_and_grad(yt, xb.detach().float())
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, wb.to(torch.bfloat16))
    with pytest.raises(ValueError, match="label"):
        vtd.my_custom_loss(dev(y).requires_grad_(), x)
    with pytest.raises(ValueError, match="exponent"):
        vtd.my_custom_loss(yt, x, exponent=0.5)


def test_no_grad_takes_the_value_path(vtd, cuda):
    """Under torch.no_grad(), or with an input that does not require grad, the result is the
    value-only path's, bit for bit, and has no grad_fn."""
    y, logits = batch((37, 17))
    yt, lg = dev(y), dev(logits)
    plain = vtd.my_custom_loss(yt, lg)
    assert plain.grad_fn is None and not plain.requires_grad
    x = dev(logits).requires_grad_()
    with torch.no_grad():
        quiet = vtd.my_custom_loss(yt, x)
        dec = vtd.transform_predictions(x)
        ci = vtd.ciou_calculator(yt, x)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)
    assert dec.grad_fn is None and torch.equal(dec, vtd.transform_predictions(lg))
    assert ci.grad_fn is None and torch.equal(ci, vtd.ciou_calculator(yt, lg))
    assert torch.equal(vtd.my_custom_loss(yt, x).detach(), plain)


def test_decode_then_loss_gives_the_fused_gradient(vtd, cuda):
    """my_custom_loss(y, transform_predictions(x), use_transform_predictions=False): two
    autograd nodes (vtd_loss_grad on the decoded values, vtd_decode_grad) against the rule of
    the from-logits gradient."""
    y, logits = batch((37, 17))
    x = dev(logits).requires_grad_()
    dec = vtd.transform_predictions(x)
    assert dec.requires_grad and torch.equal(dec.detach(), vtd.transform_predictions(dev(logits)))
    vtd.my_custom_loss(dev(y), dec, **DECODED).backward()
    check_rule("decode then loss", x.grad.cpu().numpy(), y, logits)


@pytest.mark.parametrize("shape", [(7, 4), (3, 5, 6)], ids=["7x4", "3x5x6"])
def test_ciou_calculator_gradient(vtd, cuda, shape):
    """CIoU and DIoU with a random per-element upstream; (3, 5, 6): the boxes are the last 4
    of 6 channels and the leading two get exactly 0.  The seeded pairs are checked to lie
    away from the edge kinks, so every element is held to the bound."""
    rng = np.random.default_rng(len(shape))
    lab = np.empty(shape, np.float32)
    lab[..., -4:-2] = rng.uniform(50, 550, shape[:-1] + (2,))
    lab[..., -2:] = rng.uniform(5, 300, shape[:-1] + (2,))
    lab[..., :-4] = rng.normal(0, 100, shape[:-1] + (shape[-1] - 4,))
    pred = (lab + rng.normal(0, 15, shape)).astype(np.float32)
    pred[..., -2:] = np.abs(pred[..., -2:])
    up = rng.normal(0, 1, shape[:-1]).astype(np.float32)
    assert G.edge_margin(lab, pred).min() > G.KINK_MARGIN
    for get_diou in (None, True):
        x = dev(pred).requires_grad_()
        out = vtd.ciou_calculator(dev(lab), x, get_diou=get_diou)
        assert out.requires_grad and torch.equal(
            out.detach(), vtd.ciou_calculator(dev(lab), dev(pred), get_diou=get_diou))
        (out * dev(up)).sum().backward()
        got = x.grad.cpu().numpy()
        assert got.shape == shape and np.isfinite(got).all()
        assert not got[..., :-4].any()
        g64 = G.ciou_grad(lab, pred, up, get_diou)
        g32 = G.ciou_grad(lab, pred, up, get_diou, torch.float32)
        bound, err32 = G.channel_bound(g64, g32, True)
        err = np.abs(got - g64).reshape(-1, shape[-1]).max(0)
        print(f"ciou {shape} get_diou={get_diou}: device err {err} float32 err {err32} bound {bound}")
        assert (err <= bound).all(), (err, bound)


# ---------------------------------------------------------------- extreme inputs
def test_saturated_logits(vtd, cuda):
    """Logits of +-50: the float32 sigmoid is exactly 1 (slope exactly 0) or 2e-22."""
    y, _ = batch((8, 17))
    rng = np.random.default_rng(5)
    sat = np.where(rng.random(y.shape) < 0.5, 50.0, -50.0).astype(np.float32)
    check_rule("saturated", device_grad(vtd, y, sat), y, sat)


def test_near_coincident_boxes(vtd, cuda):
    """Prediction = label + N(0, 0.05) pixels: 1 - iou is nearly all cancellation and some
    edges nearly tie; at most 10 % of the positive slots are near a kink and excluded."""
    y, logits = batch((37, 17), jitter=0.05, seed=1)
    kinked, _ = G.near_kink(y, logits)
    positive = O.isclose(y[..., 0], 1.0, np.float32)
    assert kinked.sum() <= 0.1 * positive.sum()
    check_rule("near-coincident", device_grad(vtd, y, logits), y, logits)


# ---------------------------------------------------------------- use
def test_descent(vtd, cuda):
    """Five SGD steps on a leaf logits tensor.  The step size is one at which the float64
    restatement's own trajectory decreases at every step (asserted first, on the CPU); the
    device loss must then decrease at every step too."""
    y, logits = batch((3, 10))
    rate = 0.02
    x64, ref = logits.astype(np.float64), []
    for _ in range(6):
        values, g = G.loss_and_grad(y, x64)
        ref.append(values[3])
        x64 = x64 - rate * g
    assert all(b < a for a, b in zip(ref, ref[1:])), ref
    yt, x = dev(y), dev(logits).requires_grad_()
    seen = []
    for _ in range(6):
        loss = vtd.my_custom_loss(yt, x)
        seen.append(loss)
        x.grad = None
        loss.backward()
        with torch.no_grad():
            x -= rate * x.grad
    seen = [float(v) for v in torch.stack(seen).detach().cpu()]
    print(f"descent: float64 {ref} device {seen}")
    assert all(b < a for a, b in zip(seen, seen[1:])), seen


TINY = dict(input_shape=(32, 32, 3), patch_size=8, embedding_dim=16, encoder_num_heads=2,
            encoder_key_dim=8, encoder_mlp_quantities=2, encoder_repeat_times=1,
            mlp_head_last_units=8, mlp_head_dense_layers_quantity=2)


def test_model_loss_and_grad(vtd, cuda):
    model = vtd.create_vision_transformer_detector(**TINY, dtype="float32", seed=2)
    rng = np.random.default_rng(9)
    images = rng.uniform(-1, 1, (5, 32, 32, 3)).astype(np.float32)
    y, _ = O.random_loss_batch(np.random.default_rng(11), 5, 17)
    with pytest.raises(ValueError, match="compile"):
        model.loss_and_grad(images, y)
    model.compile(loss=lambda a, b: vtd.my_custom_loss(a, b))
    with pytest.raises(ValueError, match="compile"):
        model.loss_and_grad(images, y)
    model.compile(loss=functools.partial(vtd.my_custom_loss, **NOTEBOOK))
    out5, grad = model.loss_and_grad(images, y)
    want5, want = vtd.loss_and_grad(y, model(images), **NOTEBOOK)
    assert grad.shape == (5, 17, 6) and grad.is_cuda
    assert torch.equal(out5, want5) and torch.equal(grad, want)
    assert grad.abs().sum().item() > 0
