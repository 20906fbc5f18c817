"""Model.encode / Model.head_gradients (vtd_forward_encoded, vtd_head_backward) on the GPU
against the float64 autograd of tests/head_grad_oracle.py.

Measure per tensor: max |g - g64| / max |g64|, g64 the oracle's gradient from the device's own
encoded features and d loss / d logits.  Bars: 2e-4 for bf16x3 (the figure the project holds
that mode to, 5x under the 1e-3 north star; the CPU emulation's worst is 4.2e-5), 5e-2 for
bfloat16 (emulation: 1.4e-2).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import head_grad_oracle as H
from tests import loss_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = {"bf16x3": 1e-4, "bfloat16": 3e-2}          # the modes' forward tolerances (test_gpu_model)
CASES = [("tiny_mish", 3), ("tiny_gelu", 2), ("tiny_seq400", 2), ("multi_tile", 16)]


def load_case(name, batch):
    if name == "multi_tile":
        kw = dict(H.MULTI_TILE)
        w = V.init_weights(seed=11, **kw)
        x = V.synthetic_images(batch, kw["input_shape"], seed=12)
    else:
        z = np.load(os.path.join(GOLD, f"{name}.npz"))
        kw = json.loads(str(z["kwargs"]))
        kw["input_shape"] = tuple(kw["input_shape"])
        w = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        x = V.synthetic_images(batch, kw["input_shape"], seed=21)
    rng = np.random.default_rng(batch)
    y, _ = O.random_loss_batch(rng, batch, 17)
    return kw, w, np.asarray(x, np.float32), np.asarray(y, np.float32)


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


def build(vtd, kw, w, mode):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    model.set_weights(w)
    model.compile(loss=functools.partial(vtd.my_custom_loss))
    return model


def within(y, ref, tol):
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.abs(y - ref) <= tol * np.abs(ref) + tol * np.abs(ref).max()))


@pytest.fixture(scope="module")
def runs(vtd, cuda):
    """One device run and one oracle run per (case, mode), shared by the tests below."""
    cache = {}

    def get(name, batch, mode):
        key = (name, mode)
        if key not in cache:
            kw, w, x, y = load_case(name, batch)
            model = build(vtd, kw, w, mode)
            xd = torch.from_numpy(x).to(cuda)
            enc = model.encode(xd)
            out5, grads = model.head_gradients(xd, y)
            # the oracle head applied to the device's encoded features
            logits64, _ = H.head_grads(w, enc.cpu().numpy(), np.zeros((batch, 17, 6)),
                                       kw.get("use_mish", True))
            inf = model(xd, training=False)
            cache[key] = dict(kw=kw, w=w, x=xd, y=y, model=model, enc=enc, out5=out5,
                              grads=grads, logits64=logits64, inference=inf)
        return cache[key]
    return get


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_head_gradients_against_float64_autograd(vtd, cuda, runs, case, mode):
    from vision_transformer_detector_amd import loss as vloss
    r = runs(*case, mode)
    model, kw = r["model"], r["kw"]
    assert list(r["grads"]) == model.head_weight_names() + ["encoded_images"]
    assert all(n in model.weight_names() for n in model.head_weight_names())
    # d loss / d logits as head_gradients forms it: vtd_loss_grad at the training forward's
    # logits, which the forward-only call of vtd_head_backward returns
    b = case[1]
    logits = train_logits(model, r["enc"])
    _, dlogits = vloss.loss_and_grad(r["y"], logits, params=vloss.fused_loss_params(model.loss))
    _, g64 = H.head_grads(r["w"], r["enc"].cpu().numpy(), dlogits.cpu().numpy(),
                          kw.get("use_mish", True))
    worst = {}
    for n, g in r["grads"].items():
        assert tuple(g.shape) == g64[n].shape and g.dtype == torch.float32
        worst[n] = H.rel_err(g.cpu().numpy(), g64[n])
    top = max(worst, key=worst.get)
    print(f"{case[0]} B={b} {mode}: worst {worst[top]:.3g} ({top}); "
          + ", ".join(f"{n} {v:.2g}" for n, v in worst.items()))
    assert worst[top] <= H.BARS[mode], f"{top}: {worst[top]:.3g} > {H.BARS[mode]}"
    # the training forward's logits: the mode's tolerance of model(images), and of the oracle
    # head applied to encode(images)
    assert within(logits.cpu().numpy(), r["inference"].cpu().numpy(), TOL[mode])
    assert within(r["inference"].cpu().numpy(), r["logits64"], TOL[mode])
    assert within(logits.cpu().numpy(), r["logits64"], TOL[mode])


def train_logits(model, enc):
    """The training forward's logits: vtd_head_backward with dlogits_dev = NULL."""
    import ctypes
    from vision_transformer_detector_amd import _lib as L
    b = enc.shape[0]
    cfg = model.config(b)
    need = ctypes.c_size_t()
    L.check(L.lib.vtd_head_backward_workspace_bytes(ctypes.byref(cfg), ctypes.byref(need)), "ws")
    ws = torch.empty(need.value, dtype=torch.uint8, device=enc.device)
    wdev = model._head_master()
    P = L.VtdHeadParams()
    P.w_det, P.b_det = wdev["dense/kernel"].data_ptr(), wdev["dense/bias"].data_ptr()
    for j in range(model.dims.n_head):
        P.w_head[j] = wdev[f"dense_{j + 1}/kernel"].data_ptr()
        P.b_head[j] = wdev[f"dense_{j + 1}/bias"].data_ptr()
    P.w_final = wdev["MLP_Head_no_Sigmoid/kernel"].data_ptr()
    P.b_final = wdev["MLP_Head_no_Sigmoid/bias"].data_ptr()
    logits = torch.empty((b, 17, 6), dtype=torch.float32, device=enc.device)
    L.check(L.lib.vtd_head_backward(ctypes.byref(cfg), ctypes.byref(P), enc.data_ptr(), None,
                                    logits.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                    L.stream_ptr()), "vtd_head_backward")
    torch.cuda.synchronize()
    return logits


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
def test_cached_features_and_repeat_calls_are_bit_identical(vtd, cuda, runs, mode):
    r = runs("tiny_mish", 3, mode)
    model = r["model"]
    out_a, g_a = model.head_gradients(None, r["y"], encoded=r["enc"])
    out_b, g_b = model.head_gradients(r["x"], r["y"])
    for other_out, other in ((out_a, g_a), (out_b, g_b)):
        assert torch.equal(other_out, r["out5"])
        for n, g in r["grads"].items():
            assert torch.equal(g, other[n]), n


def test_descent_step_lowers_the_loss_as_the_gradient_predicts(vtd, cuda, runs):
    """w' = w - eps g on the head's weights: loss(w') - loss(w) within 10 % of -eps |g|^2, eps
    chosen so that the change is about 1 % of the loss (far above the forward's 1e-5 noise)."""
    r = runs("tiny_mish", 3, "bf16x3")
    model, y = r["model"], r["y"]
    names = model.head_weight_names()
    g2 = sum(float((r["grads"][n].double() ** 2).sum()) for n in names)
    loss0 = float(r["out5"][0])
    eps = 0.01 * loss0 / g2
    wd = model.get_weight_dict()
    stepped = dict(wd)
    for n in names:
        stepped[n] = wd[n] - eps * r["grads"][n].cpu().numpy()
    try:
        model.set_weights(stepped)
        out5, _ = model.head_gradients(None, y, encoded=r["enc"])
        change = float(out5[0]) - loss0
    finally:
        model.set_weights(wd)
    print(f"descent: loss {loss0:.6g}, eps {eps:.3g}, change {change:.6g}, "
          f"predicted {-eps * g2:.6g}")
    assert abs(change - (-eps * g2)) <= 0.1 * eps * g2


@pytest.mark.parametrize("mode", ["float32", "float8"])
def test_unsupported_modes_raise(vtd, cuda, mode):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = build(vtd, kw, w, mode)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.head_gradients(torch.from_numpy(x).to(cuda), y)


def test_needs_a_compiled_loss(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = vtd.create_vision_transformer_detector(**kw, dtype="bf16x3")
    with pytest.raises(ValueError, match="compile"):
        model.head_gradients(torch.from_numpy(x).to(cuda), y)
