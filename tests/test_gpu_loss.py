"""Validation loss on the device (vtd_loss / vtd_ciou / vtd_diagonal, loss.py, Model.compile
/ evaluate) against the float64 restatement of the reference (tests/loss_oracle.py).

The tolerance is not a constant: the fp32 `1 - iou` cancellation makes the achievable error
depend on the input.  For each input the same restatement is evaluated in float32 on the CPU,
its error against float64 is measured per component and for the total, and the device may be
at most 8x that error plus 4 float32 ulp of the value (loss_oracle.allowed_error): the
device's logf / atanf / expf differ from numpy's by a few ulp, and its fp64 sums are better
than numpy's float32 ones, not worse.  Each check prints its device / float32 error ratio."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import loss_oracle as O

pytestmark = pytest.mark.gpu

NOTEBOOK = dict(coefficient=9, exponent=2, weight_ciou=4.5)          # ipynb:408-435
SHAPES = [(1, 1), (3, 10), (8, 17), (37, 17), (256, 17)]
NAMES = ("objectness", "classification", "ciou", "total")


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@functools.lru_cache(maxsize=None)
def batch(shape, jitter=20.0, seed=0):
    """One seeded (labels, logits) pair per shape, shared by the tests and left unchanged."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    y, logits = O.random_loss_batch(rng, *shape, jitter=jitter)
    y.setflags(write=False)
    logits.setflags(write=False)
    return y, logits


def check_rule(what, got5, y, p, **kw):
    """got5: the device's [total, objectness, classification, ciou, positives]."""
    ref, bound, err = O.allowed_error(y, p, **kw)
    got = (got5[1], got5[2], got5[3], got5[0])
    assert np.isfinite(got5).all(), (what, got5)
    positive = O.isclose(np.asarray(y, np.float32)[..., 0], 1.0, np.float32)
    assert got5[4] == positive.sum(), what
    for name, g, r, b, e in zip(NAMES, got, ref, bound, err):
        d = abs(float(g) - float(r))
        print(f"{what} {name}: device {float(g):.9g} float64 {float(r):.9g} device err {d:.3g} "
              f"float32 err {e:.3g} ratio {d / e if e else float('nan'):.3g} bound {b:.3g}")
    for name, g, r, b in zip(NAMES, got, ref, bound):
        assert abs(float(g) - float(r)) <= b, (what, name, float(g), float(r), b)


def components(vtd, y, p, **kw):
    return vtd.loss_components(torch.tensor(np.asarray(y)).cuda(),
                               torch.tensor(np.asarray(p)).cuda(), **kw).cpu().numpy()


# ---------------------------------------------------------------- known answers
def test_known_answers_on_the_device(vtd, cuda):
    """The reference's four fixtures (tests.py:760-926), the CPU test's bounds; the device's
    float32 leaves no residue in the identical-prediction case: exactly 0."""
    kw = dict(use_transform_predictions=False)
    y, p = O.kat_case(None)
    zero = vtd.my_custom_loss(y, p, **kw)
    assert zero.shape == () and zero.dtype == torch.float32 and zero.is_cuda
    assert zero.item() == 0.0
    np.testing.assert_array_equal(components(vtd, y, p, **kw), [0, 0, 0, 0, 1])
    got = vtd.my_custom_loss(*O.kat_case("objectness"), **kw).item()
    assert got == pytest.approx(4.0405e-7, rel=1e-4)
    got = vtd.my_custom_loss(*O.kat_case("class"), **kw).item()
    assert got == pytest.approx(4.736e-3, rel=1e-4)
    got = vtd.my_custom_loss(*O.kat_case("box"), **kw).item()
    assert abs(got - 0.396) <= 1e-5
    # the plain cross-entropy branch on the objectness fixture
    got = vtd.my_custom_loss(*O.kat_case("objectness"), focal_binary_loss=False, **kw).item()
    assert got == pytest.approx(-np.log(0.98 + 1e-7) / 20, rel=1e-4)


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("params", [{}, NOTEBOOK], ids=["defaults", "notebook"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_matches_float64_oracle(vtd, cuda, shape, params):
    """Seeded labels and logits; every shape but (1, 1) holds an image without positives
    and one with every slot positive.  (37, 17) = 629 slots: no multiple of 64, a part-filled
    wave and idle ones; (256, 17), the bench batch, is 4.25 trips of the workgroup."""
    y, logits = batch(shape)
    check_rule(f"{shape} {params}", components(vtd, y, logits, **params), y, logits, **params)


@pytest.mark.parametrize("focal,exponent", [(False, 2), (True, 4), (True, 2.5)])
def test_loss_other_branches_match_oracle(vtd, cuda, focal, exponent):
    """Plain cross-entropy, and exponents that take powf instead of x * x."""
    y, logits = batch((8, 17))
    kw = dict(focal_binary_loss=focal, exponent=exponent)
    check_rule(f"focal={focal} exponent={exponent}", components(vtd, y, logits, **kw), y, logits,
               **kw)


def test_near_coincident_boxes(vtd, cuda):
    """Prediction = label + N(0, 0.05) pixels: 1 - iou is nearly all cancellation."""
    y, logits = batch((37, 17), jitter=0.05, seed=1)
    check_rule("near-coincident", components(vtd, y, logits), y, logits)
    dec = O.transform_predictions(logits, np.float32)
    kw = dict(use_transform_predictions=False)
    check_rule("near-coincident decoded", components(vtd, y, dec, **kw), y, dec, **kw)


def test_degenerate_inputs(vtd, cuda):
    """Logits of +-50 (the sigmoid saturates to 0 and 1 in float32) and zero-size predicted
    boxes (h = w = 0): everything finite, the same rule."""
    y, logits = batch((8, 17))
    rng = np.random.default_rng(5)
    sat = np.where(rng.random(logits.shape) < 0.5, 50.0, -50.0).astype(np.float32)
    check_rule("saturated", components(vtd, y, sat), y, sat)
    mixed = np.where(rng.random(logits.shape) < 0.3, sat, logits).astype(np.float32)
    check_rule("partly saturated", components(vtd, y, mixed), y, mixed)
    dec = O.transform_predictions(logits, np.float32)
    dec[..., 4:] = 0.0
    kw = dict(use_transform_predictions=False)
    check_rule("zero-size boxes", components(vtd, y, dec, **kw), y, dec, **kw)
    gone = logits.copy()
    gone[..., 4:] = -200.0                       # expf overflows: the sigmoid is exactly 0
    check_rule("zero-size boxes from logits", components(vtd, y, gone), y, gone)


def test_no_positive_in_the_whole_batch(vtd, cuda):
    y, logits = batch((8, 17))
    y = y.copy()
    y[...] = -8.0
    y[..., 0] = 0.0
    got = components(vtd, y, logits)
    assert got[2] == 0 and got[3] == 0 and got[4] == 0
    assert got[0].tobytes() == got[1].tobytes()           # total is the objectness mean, bit for bit
    check_rule("no positives", got, y, logits)


def test_fused_decode_is_bit_identical(vtd, cuda):
    """from_logits=1 decodes with vtd_decode's own device function."""
    y, logits = batch((37, 17))
    fused = components(vtd, y, logits)
    dec = vtd.transform_predictions(torch.tensor(logits).cuda())
    two_step = vtd.loss_components(torch.tensor(y).cuda(), dec,
                                   use_transform_predictions=False).cpu().numpy()
    assert fused.tobytes() == two_step.tobytes()


def test_two_calls_give_identical_bits(vtd, cuda):
    y, logits = batch((256, 17))
    yt, lg = torch.tensor(y).cuda(), torch.tensor(logits).cuda()
    a = vtd.loss_components(yt, lg, **NOTEBOOK).cpu().numpy()
    b = vtd.loss_components(yt, lg, **NOTEBOOK).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def test_running_accumulator_and_empty_batch(vtd, cuda):
    """running_dev after batches of 2, 2 and 1 holds sum(total_b * B_b) and 5; B = 0 writes
    zeros and leaves it alone."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import loss as VL
    y, logits = batch((8, 17))
    yt, lg = torch.tensor(y[:5]).cuda(), torch.tensor(logits[:5]).cuda()
    params = VL.loss_params(**NOTEBOOK)
    running = torch.zeros(2, dtype=torch.float64, device=cuda)
    totals = []
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        out = VL._launch(yt[lo:hi], lg[lo:hi], params, running)
        totals.append((out[0].item(), hi - lo))
    want = 0.0
    for t, n in totals:
        want += float(np.float32(t)) * n
    assert running.cpu().tolist() == [want, 5.0]
    out = torch.full((5,), 7.0, device=cuda)
    L.check(L.lib.vtd_loss(None, None, 0, 17, ctypes.byref(params), out.data_ptr(),
                           running.data_ptr(), L.stream_ptr()))
    assert out.cpu().tolist() == [0.0] * 5 and running.cpu().tolist() == [want, 5.0]
    assert vtd.my_custom_loss(np.zeros((0, 17, 6)), np.zeros((0, 17, 6))).item() == 0.0
    with pytest.raises(ValueError):
        vtd.my_custom_loss(np.zeros((2, 10, 6)), np.zeros((2, 11, 6)))
    with pytest.raises(ValueError, match="coefficient"):
        vtd.my_custom_loss(y, logits, coefficient=float("nan"))


# ---------------------------------------------------------------- ciou / diagonal
@pytest.mark.parametrize("shape", [(5, 4), (2, 3, 7, 6)], ids=["5x4", "2x3x7x6"])
def test_ciou_and_diagonal_match_oracle(vtd, cuda, shape):
    """(2, 3, 7, 6): the boxes are the last 4 of 6 channels.  Both get_diou values, each
    element under the 8x rule; numpy and tensor inputs give the same device result."""
    rng = np.random.default_rng(len(shape))
    lab = np.empty(shape, np.float32)
    lab[..., -4:-2] = rng.uniform(50, 550, shape[:-1] + (2,))
    lab[..., -2:] = rng.uniform(5, 300, shape[:-1] + (2,))
    lab[..., :-4] = rng.normal(0, 100, shape[:-1] + (shape[-1] - 4,))     # ignored channels
    pred = (lab + rng.normal(0, 15, shape)).astype(np.float32)
    pred[..., -2:] = np.abs(pred[..., -2:])
    lab.flat[-4:] = pred.flat[-4:]                                        # one identical pair
    for get_diou in (None, True):
        got = vtd.ciou_calculator(lab, pred, get_diou=get_diou)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == shape[:-1]
        same = vtd.ciou_calculator(torch.tensor(lab).cuda(), torch.tensor(pred).cuda(),
                                   get_diou=get_diou)
        assert torch.equal(got, same)
        got = got.cpu().numpy().astype(np.float64)
        ref = O.ciou_calculator(lab, pred, get_diou=get_diou)
        f32 = O.ciou_calculator(lab, pred, get_diou=get_diou, dtype=np.float32).astype(np.float64)
        bound = 8 * np.abs(f32 - ref) + 4 * np.spacing(np.abs(ref).astype(np.float32))
        print(f"ciou {shape} get_diou={get_diou}: worst device err {np.abs(got - ref).max():.3g} "
              f"worst float32 err {np.abs(f32 - ref).max():.3g}")
        assert (np.abs(got - ref) <= bound).all(), (got, ref, bound)
        if get_diou:        # no atan in the DIoU: every operation is correctly rounded on both
            np.testing.assert_array_equal(got, f32)     # sides, in the same order
        else:               # the identical pair: equal atans cancel exactly on both sides
            assert got.flat[-1] == f32.flat[-1]
    got = vtd.diagonal_calculator(lab, pred).cpu().numpy()
    np.testing.assert_array_equal(got, O.diagonal_calculator(lab, pred, dtype=np.float32))
    for fn in (vtd.ciou_calculator, vtd.diagonal_calculator):
        with pytest.raises(ValueError):
            fn(np.zeros((5, 4)), np.zeros((4, 4)))
        with pytest.raises(ValueError):
            fn(np.zeros((5, 3)), np.zeros((5, 3)))


# ---------------------------------------------------------------- Model.evaluate
TINY = dict(input_shape=(32, 32, 3), patch_size=8, embedding_dim=16, encoder_num_heads=2,
            encoder_key_dim=8, encoder_mlp_quantities=2, encoder_repeat_times=1,
            mlp_head_last_units=8, mlp_head_dense_layers_quantity=2)
SPLITS = ((0, 2), (2, 4), (4, 5))


def test_model_evaluate(vtd, cuda):
    model = vtd.create_vision_transformer_detector(**TINY, dtype="float32", seed=2)
    rng = np.random.default_rng(9)
    images = rng.uniform(-1, 1, (5, 32, 32, 3)).astype(np.float32)
    with pytest.raises(RuntimeError, match="compile"):
        model.evaluate(images, np.zeros((5, 17, 6), np.float32))
    # labels: the model's own confident detections (so the AP has matches to count), the
    # boxes moved a little, in the first slots of each image; the rest empty
    logits = model(images).cpu().numpy()
    dec = O.transform_predictions(logits, np.float32)
    labels = np.full((5, 17, 6), -8.0, np.float32)
    labels[..., 0] = 0.0
    for b in range(5):
        keep = [i for i in range(17) if dec[b, i, 0] > 0.5 and
                abs(dec[b, i, 1] - np.rint(dec[b, i, 1])) < 0.2][:6]
        for k, i in enumerate(keep):
            labels[b, k] = (1.0, np.rint(dec[b, i, 1]), *(dec[b, i, 2:] + rng.normal(0, 4, 4)))

    loss = functools.partial(vtd.my_custom_loss, **NOTEBOOK)
    model.compile(optimizer="adam", loss=loss, metrics=[vtd.MeanAveragePrecision()])
    got = model.evaluate(images, labels, batch_size=2)
    assert isinstance(got, list) and len(got) == 2 and all(type(v) is float for v in got)

    # by hand over the same three batches
    hand = vtd.MeanAveragePrecision()
    ref = bound = 0.0
    for lo, hi in SPLITS:
        lg = model(images[lo:hi])
        hand.update_state(labels[lo:hi], lg)
        r, _, e = O.allowed_error(labels[lo:hi], lg.cpu().numpy(), **NOTEBOOK)
        ref += float(r[3]) * (hi - lo) / 5
        bound += 8 * e[3] * (hi - lo) / 5
    bound += 4 * O.fp32_ulp(ref)
    print(f"evaluate: loss {got[0]:.9g} float64 {ref:.9g} err {abs(got[0] - ref):.3g} "
          f"bound {bound:.3g}; AP {got[1]:.6g}")
    assert abs(got[0] - ref) <= bound
    assert got[1] == hand.result().item()

    batches = [(torch.tensor(images[lo:hi]).cuda(), labels[lo:hi]) for lo, hi in SPLITS]
    assert model.evaluate(iter(batches)) == got
    assert model.evaluate(images, labels, batch_size=2) == got            # metrics are reset
    d = model.evaluate(torch.tensor(images), torch.tensor(labels), batch_size=2,
                       return_dict=True)
    assert list(d) == ["loss", "AP"] and [d["loss"], d["AP"]] == got

    # one device-to-host read: with device inputs, torch reports exactly one synchronising
    # operation (the final copy) over the whole evaluate
    on_device = [(torch.tensor(images[lo:hi]).cuda(), torch.tensor(labels[lo:hi]).cuda())
                 for lo, hi in SPLITS]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            assert model.evaluate(on_device) == got
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, syncs

    def generic(y_true, y_pred):
        return vtd.my_custom_loss(y_true, y_pred, **NOTEBOOK)

    model.compile(loss=generic, metrics=[vtd.MeanAveragePrecision()])
    assert model.evaluate(images, labels, batch_size=2) == got
    model.compile(loss=loss)
    assert model.evaluate(images, labels, batch_size=2) == got[0]
    with pytest.raises(ValueError):
        model.evaluate(images, labels[:4])
