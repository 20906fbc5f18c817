"""Model.detection_head / vtd_head_backward_dropout on the GPU against the masked float64 head of
tests/model_dropout_oracle.py: the reference's Dropout after every head Dense + activation, head
layer j at site L (1 + q) + j over the unpadded [B 17][units_j] activation.

Measure and bars are those of tests/test_gpu_head_backward.py (per tensor max |g - g64| /
max |g64| at 2e-4 bf16x3 / 5e-2 bfloat16, the logits within the modes' forward tolerances): the
oracle is fed the device's own encoded features and upstream gradient, and a mask rescales the
device's and the oracle's terms alike.  A mask taken from padded columns, from another site or
with another row stride is an error of order one at these bars.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dropout_oracle as D
from tests import head_grad_oracle as H
from tests import model_dropout_oracle as R
from tests.test_gpu_encoder_block import same_bits
from tests.test_gpu_head_backward import TOL, within

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]
STEP = 2

modes = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
rates = pytest.mark.parametrize("rate", R.RATES)


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


def build(vtd, kw, w, mode, **compile_kw):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    model.set_weights(w)
    model.compile(loss=functools.partial(vtd.my_custom_loss), **compile_kw)
    return model


@pytest.fixture(scope="module")
def setups(vtd, cuda):
    """Per (case, mode): a model built with dropout=0.5 and no compiled seed, the device's
    encoded features and today's head_gradients on them."""
    cache = {}

    def get(name, batch, mode):
        if (name, mode) not in cache:
            kw, w, x, y = R.load_case(name, batch)
            model = build(vtd, dict(kw, dropout=0.5), w, mode)
            enc = model.encode(torch.from_numpy(x).to(cuda))
            out5, grads = model.head_gradients(None, y, encoded=enc)
            cache[(name, mode)] = dict(kw=kw, w=w, y=y, model=model, enc=enc, out5=out5,
                                       grads=grads)
        return cache[(name, mode)]
    return get


def head_pass(s, **kw):
    """(logits, dlogits, {name: grad} with "encoded_images") of detection_head -> the compiled
    loss's gradient -> backward, on fresh leaves."""
    from vision_transformer_detector_amd import loss as vloss
    model = s["model"]
    enc = s["enc"].clone().requires_grad_(True)
    hw = model.head_weights()
    for t in hw.values():
        t.requires_grad_(True)
    logits = model.detection_head(enc, hw, **kw)
    _, dlogits = vloss.loss_and_grad(s["y"], logits.detach(),
                                     params=vloss.fused_loss_params(model.loss))
    logits.backward(dlogits)
    grads = {n: t.grad for n, t in hw.items()}
    grads["encoded_images"] = enc.grad
    return logits.detach(), dlogits, grads


@rates
@modes
@cases
def test_head_against_masked_float64(setups, case, mode, rate):
    name, b = case
    s = setups(name, b, mode)
    kw = s["kw"]
    logits, dlogits, grads = head_pass(s, seed=R.SEED, step=STEP, dropout=rate)
    masks = R.head_masks(kw, b, rate, R.SEED, STEP)
    logits64, g64 = R.head_grads(s["w"], s["enc"].cpu().numpy(), dlogits.cpu().numpy(),
                                 kw.get("use_mish", True), masks, D.inv_keep(rate))
    worst = {n: H.rel_err(grads[n].cpu().numpy(), g64[n]) for n in g64}
    top = max(worst, key=worst.get)
    ln = logits.cpu().numpy()
    print(f"{name} B={b} {mode} rate {rate}: worst {worst[top]:.3g} ({top}); logits "
          f"{np.abs(ln - logits64).max() / np.abs(logits64).max():.3g}; "
          + ", ".join(f"{n} {v:.2g}" for n, v in worst.items()))
    assert set(worst) == set(s["model"].head_weight_names()) | {"encoded_images"}
    assert within(ln, logits64, TOL[mode])
    for n, v in worst.items():
        assert v <= H.BARS[mode], f"{n}: {v:.3g} > {H.BARS[mode]}"


@modes
@cases
def test_no_seed_and_rate_zero_are_todays_head_bit_for_bit(setups, case, mode):
    s = setups(*case, mode)
    for kw in (dict(), dict(seed=None, dropout=None), dict(seed=R.SEED, dropout=0.0, step=5),
               dict(dropout=0.0)):
        logits, _, grads = head_pass(s, **kw)
        assert list(s["grads"]) == s["model"].head_weight_names() + ["encoded_images"]
        for n, g in s["grads"].items():
            assert same_bits(grads[n], g), (kw, n)
    # weights=None: the model's current head weights
    assert same_bits(s["model"].detection_head(s["enc"]), logits)


@modes
@cases
def test_c_entry_rate_zero_workspace_guards_and_repeat_calls(setups, cuda, case, mode):
    """vtd_head_backward_dropout through head.run with exactly
    vtd_head_backward_workspace_bytes inside 0xA5 guard bands: rate 0 gives vtd_head_backward's
    bits, rate 0.5 the autograd op's, twice; one byte less is VTD_ERR_WORKSPACE."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import head
    name, b = case
    s = setups(name, b, mode)
    model, enc = s["model"], s["enc"]
    base = R.head_site_base(s["kw"])
    cfg = model.config(b)
    need = head.workspace_bytes(cfg)
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
    ws = buf[256:256 + need]
    weights = list(model.head_weights().values())

    def chain(drop, dlogits, ws=ws):
        logits = torch.empty((b, 17, 6), dtype=torch.float32, device=cuda)
        head.run(cfg, enc, weights, logits=logits, ws=ws, drop=drop)
        grads = [torch.empty_like(t) for t in weights]
        dx = torch.empty_like(enc)
        head.run(cfg, enc, weights, dlogits=dlogits, grads=grads, d_encoded=dx, ws=ws, drop=drop)
        torch.cuda.synchronize()
        assert bool((buf[:256] == 0xA5).all() and (buf[-256:] == 0xA5).all())
        return logits, grads + [dx]

    logits0, dl0, want0 = head_pass(s)
    zero = L.VtdBlockDropout(seed=R.SEED, step=STEP, site_base=base, rate=0.0)
    for drop in (None, zero):
        logits, got = chain(drop, dl0)
        assert same_bits(logits, logits0)
        assert all(same_bits(g, w) for g, w in zip(got, want0.values()))
    logits1, dl1, want1 = head_pass(s, seed=R.SEED, step=STEP)
    half = L.VtdBlockDropout(seed=R.SEED, step=STEP, site_base=base, rate=0.5)
    for _ in range(2):
        logits, got = chain(half, dl1)
        assert same_bits(logits, logits1) and not same_bits(logits, logits0)
        assert all(same_bits(g, w) for g, w in zip(got, want1.values()))
    with pytest.raises(L.VtdError, match="WORKSPACE"):
        chain(half, dl1, ws=buf[256:256 + need - 1])


@modes
def test_repeat_calls_and_sensitivity(setups, mode):
    s = setups("ragged_head", 3, mode)
    model, enc = s["model"], s["enc"]
    base = R.head_site_base(s["kw"])
    kw = dict(seed=R.SEED, step=STEP)
    a, _, ga = head_pass(s, **kw)
    b, _, gb = head_pass(s, **kw)
    assert same_bits(a, b) and all(same_bits(ga[n], gb[n]) for n in ga)
    # the defaults: the model's rate, site_base L (1 + q)
    assert same_bits(model.detection_head(enc, dropout=0.5, site_base=base, **kw), a)
    for other in (dict(kw, step=STEP + 1), dict(kw, seed=R.OTHER_SEED),
                  dict(kw, site_base=base + 1), dict(kw, dropout=0.1)):
        assert not same_bits(model.detection_head(enc, **other), a), other
    assert not same_bits(a, s["model"].detection_head(enc))


@modes
@pytest.mark.parametrize("name", ["tiny_mish", "ragged_head"])
def test_image_zero_does_not_depend_on_the_batch(setups, name, mode):
    s = setups(name, 3, mode)
    model, enc = s["model"], s["enc"]
    kw = dict(seed=R.SEED, step=STEP)
    three = model.detection_head(enc, **kw)
    alone = model.detection_head(enc[:1].contiguous(), **kw)
    assert same_bits(three[:1], alone)


def test_argument_checks(vtd, setups, cuda):
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import head
    s = setups("tiny_mish", 3, "bf16x3")
    model, enc = s["model"], s["enc"]
    cfg = model.config(3)
    weights = list(model.head_weights().values())
    logits = torch.empty((3, 17, 6), dtype=torch.float32, device=cuda)
    for bad in (L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=1.0),
                L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=float("nan")),
                L.VtdBlockDropout(seed=1, step=0, site_base=0xFFFFFFFE, rate=0.5)):
        with pytest.raises(ValueError):
            head.run(cfg, enc, weights, logits=logits, drop=bad)
    params = head._fill(L.VtdHeadParams(), weights)
    ws = torch.empty(head.workspace_bytes(cfg), dtype=torch.uint8, device=cuda)
    assert L.lib.vtd_head_backward_dropout(
        ctypes.byref(cfg), ctypes.byref(params), enc.data_ptr(), None, logits.data_ptr(), None,
        ws.data_ptr(), ws.numel(), L.stream_ptr(), None) == -1
    with pytest.raises(ValueError, match="seed"):
        model.detection_head(enc, dropout=0.5)
    with pytest.raises(ValueError, match="rate"):
        model.detection_head(enc, dropout=1.0, seed=1)
    with pytest.raises(ValueError, match="site_base"):
        model.detection_head(enc, seed=1, site_base=(1 << 32) - 2)
    with pytest.raises(ValueError, match="encoded"):
        model.detection_head(enc[:, :-1], seed=1)
    with pytest.raises(ValueError, match="weights"):
        model.detection_head(enc, weights[:-1])
    f32 = build(vtd, s["kw"], s["w"], "float32")
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        f32.detection_head(enc)
