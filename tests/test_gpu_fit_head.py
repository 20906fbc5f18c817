"""Model.train_head_on_batch / fit_head on the GPU: the optimizer step at model level.

The step's arithmetic is pinned bit for bit: the head weights after a step equal
tests/adam_oracle.py step32 applied on the host to the previous weights with the gradients
head_gradients returns for the same state.  The trajectory test compares five steps with the
float64 head oracle (tests/head_grad_oracle.py + tests/loss_grad_oracle.py + step64) run on the
device's encoded features.
"""
import functools

import numpy as np
import pytest
import torch

from tests import adam_oracle as A
from tests import head_grad_oracle as H
from tests import loss_grad_oracle as G
from tests.test_gpu_head_backward import load_case

pytestmark = pytest.mark.gpu
CASES = [("tiny_mish", 3), ("multi_tile", 16)]
MODES = ["bf16x3", "bfloat16"]
LR = 1e-3
# the number of steps after which the float64 oracle's own loss on tiny_mish (B = 3, lr 1e-3,
# clipvalue 10) has fallen by at least 10 %: checked on the CPU, and again by the test
DESCENT_STEPS = 10
# worst relative deviation of the device's five losses from the float64 trajectory measured on
# the MI355X (bf16x3, tiny_mish, B = 3), and the bar at 4 x that
TRAJECTORY_MEASURED = 2.37e-6
TRAJECTORY_BAR = 4 * TRAJECTORY_MEASURED          # 9.48e-6


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


def build(vtd, kw, w, mode, lr=LR, **extra):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode, **extra)
    model.set_weights(w)
    model.compile(optimizer=vtd.optimizers.Adam(learning_rate=lr, clipvalue=10),
                  loss=functools.partial(vtd.my_custom_loss))
    return model


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def host_step(w, m, v, g, t, lr, **kw):
    return A.step32(w, m, v, g, t, lr, clipvalue=10.0, max_weight=10.0, constrain=True, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_one_step_is_step32_of_the_head_gradients(vtd, cuda, case, mode):
    kw, w, x, y = load_case(*case)
    model = build(vtd, kw, w, mode)
    xd = torch.from_numpy(x).to(cuda)
    before = model.get_weight_dict()
    out5_ref, grads = model.head_gradients(xd, y)
    out5 = model.train_head_on_batch(xd, y)
    assert torch.equal(out5, out5_ref)
    assert model.optimizer.iterations == 1
    after = model.get_weight_dict()
    head = model.head_weight_names()
    live = model._head_master()
    for n in model.weight_names():
        if n in head:
            z = np.zeros_like(before[n])
            want, m1, v1 = host_step(before[n], z, z, grads[n].cpu().numpy(), 1, LR)
            assert same_bits(after[n], want), n
            assert same_bits(live[n].cpu().numpy(), want), n
            mom_m, mom_v = model.optimizer.moments(model)
            assert same_bits(mom_m[n].cpu().numpy(), m1) and same_bits(mom_v[n].cpu().numpy(), v1)
            assert not same_bits(after[n], before[n]), n
        else:
            assert same_bits(after[n], before[n]), n
    # a second step continues from the moments (t = 2)
    _, grads = model.head_gradients(xd, y)
    mom_m, mom_v = model.optimizer.moments(model)
    m1 = {n: mom_m[n].cpu().numpy() for n in head}
    v1 = {n: mom_v[n].cpu().numpy() for n in head}
    model.train_head_on_batch(None, y, encoded=model.encode(xd))
    again = model.get_weight_dict()
    for n in head:
        want, _, _ = host_step(after[n], m1[n], v1[n], grads[n].cpu().numpy(), 2, LR)
        assert same_bits(again[n], want), n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_packed_operands_are_live_and_weights_round_trip(vtd, cuda, case, mode, tmp_path):
    kw, w, x, y = load_case(*case)
    model = build(vtd, kw, w, mode)
    xd = torch.from_numpy(x).to(cuda)
    untrained = model(xd).clone()
    for _ in range(3):
        model.train_head_on_batch(xd, y)
    logits = model(xd)
    assert not torch.equal(logits, untrained)
    fresh = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    fresh.set_weights(model.get_weight_dict())
    assert torch.equal(fresh(xd), logits)
    assert [same_bits(a, b) for a, b in zip(model.get_weights(), fresh.get_weights())] == \
        [True] * len(model.weight_names())
    # save / load: the file holds the trained weights
    path = str(tmp_path / "trained.npz")
    model.save_weights(path)
    loaded = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    loaded.load_weights(path)
    assert torch.equal(loaded(xd), logits)
    # set_weights resets the optimizer's state for the model
    assert model.optimizer.iterations == 3
    model.load_weights(path)
    assert model.optimizer.iterations == 0
    m, v = model.optimizer.moments(model)
    assert all(not t.any() for t in m.values()) and all(not t.any() for t in v.values())
    assert torch.equal(model(xd), logits)


def oracle_trajectory(w, enc, y, use_mish, steps, lr=LR):
    """The float64 losses of `steps` Adam steps on the head from fixed encoded features."""
    names = [f"{n}/{p}" for n in H.head_names(w) for p in ("kernel", "bias")]
    cur = {n: np.asarray(w[n], np.float64) for n in names}
    m = {n: np.zeros_like(cur[n]) for n in names}
    v = {n: np.zeros_like(cur[n]) for n in names}
    losses = []
    enc64 = torch.tensor(np.asarray(enc), dtype=torch.float64)
    for t in range(1, steps + 1):
        logits = H.head_forward(H.head_weights(cur), enc64, use_mish).numpy()
        values, dlogits = G.loss_and_grad(y, logits)
        losses.append(values[3])
        _, grads = H.head_grads(cur, enc, dlogits, use_mish)
        for n in names:
            cur[n], m[n], v[n] = A.step64(cur[n], m[n], v[n], grads[n], t, lr, clipvalue=10.0,
                                          max_weight=10.0, constrain=True)
    return losses


def test_trajectory_follows_the_float64_oracle(vtd, cuda):
    """Five steps at lr 1e-3, clipvalue 10, tiny_mish B = 3, bf16x3: the device's losses against
    the float64 oracle's on the device's encoded features.  Adam's near-sign update amplifies
    gradient noise where |g| ~ epsilon, hence a measured bar: worst relative deviation on the
    MI355X 2.37e-6 (TRAJECTORY_MEASURED; the five were 6.5e-7, 1.9e-6, 3.8e-7, 2.6e-7, 2.4e-6),
    bar 4 x that, 9.48e-6 (TRAJECTORY_BAR).  Then DESCENT_STEPS steps in all:
    the oracle's own loss falls by at least 10 % and the device's loss is below its first."""
    kw, w, x, y = load_case("tiny_mish", 3)
    model = build(vtd, kw, w, "bf16x3")
    enc = model.encode(torch.from_numpy(x).to(cuda))
    ref = oracle_trajectory(w, enc.cpu().numpy(), y, kw.get("use_mish", True), DESCENT_STEPS)
    got = [model.train_head_on_batch(None, y, encoded=enc) for _ in range(DESCENT_STEPS)]
    got = [float(v) for v in torch.stack(got)[:, 0].cpu()]
    dev = [abs(a - b) / abs(b) for a, b in zip(got[:5], ref[:5])]
    print("device losses", got[:5], "oracle", ref[:5], "relative deviation", dev,
          f"worst {max(dev):.3g}; after {DESCENT_STEPS} steps: device {got[-1]:.6g} "
          f"oracle {ref[-1]:.6g}")
    assert max(dev) <= TRAJECTORY_BAR
    assert ref[-1] <= 0.9 * ref[0]
    assert got[-1] < got[0]


def test_fit_head_history_batches_cache_and_schedule(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 5)
    xd = torch.from_numpy(x).to(cuda)
    # a manual loop over batches of 2, 2, 1 for two epochs
    manual = build(vtd, kw, w, "bf16x3")
    want = []
    for _ in range(2):
        total, count = 0.0, 0
        for i in range(0, 5, 2):
            out5 = manual.train_head_on_batch(xd[i:i + 2], y[i:i + 2])
            n = len(y[i:i + 2])
            total += float(out5[0].double()) * n
            count += n
        want.append(total / count)
    results = {}
    for cache in (True, False):
        model = build(vtd, kw, w, "bf16x3")
        hist = model.fit_head(xd, y, batch_size=2, epochs=2, cache_features=cache)
        assert hist.history["loss"] == want, cache
        assert model.optimizer.iterations == 6
        results[cache] = model.get_weights()
    for a, b, c in zip(results[True], results[False], manual.get_weights()):
        assert same_bits(a, b) and same_bits(a, c)
    # encoded= for the whole of x, and an iterable of batches with y=None
    model = build(vtd, kw, w, "bf16x3")
    hist = model.fit_head(None, y, batch_size=2, epochs=2, encoded=manual.encode(xd))
    assert hist.history["loss"] == want
    model = build(vtd, kw, w, "bf16x3")
    hist = model.fit_head([(xd[i:i + 2], y[i:i + 2]) for i in range(0, 5, 2)], epochs=2)
    assert hist.history["loss"] == want

    # the schedule: called with (epoch, current lr) at the start of each epoch, its return used
    calls = []

    def schedule(epoch, lr):
        calls.append((epoch, lr))
        return lr * 0.5 if epoch == 1 else lr

    model = build(vtd, kw, w, "bf16x3")
    model.fit_head(xd, y, batch_size=5, epochs=2, lr_schedule=schedule)
    assert calls == [(0, LR), (1, LR)] and model.optimizer.learning_rate == LR * 0.5
    other = build(vtd, kw, w, "bf16x3")
    other.train_head_on_batch(xd, y)                               # epoch 0 at LR
    w1 = other.get_weight_dict()
    m1, v1 = other.optimizer.moments(other)
    _, grads = other.head_gradients(xd, y)
    got = model.get_weight_dict()
    for n in model.head_weight_names():
        expect, _, _ = host_step(w1[n], m1[n].cpu().numpy(), v1[n].cpu().numpy(),
                                 grads[n].cpu().numpy(), 2, LR * 0.5)
        assert same_bits(got[n], expect), n


def test_clip_weight_false_and_max_weight_reach_the_kernel(vtd, cuda):
    """max_weight / clip_weight stop being no-ops: with max_weight below the weights' range the
    step clips every head weight to it; clip_weight=False leaves them free."""
    kw, w, x, y = load_case("tiny_mish", 3)
    xd = torch.from_numpy(x).to(cuda)
    bound = 0.01
    clipped = build(vtd, dict(kw, max_weight=bound), w, "bf16x3")
    free = build(vtd, dict(kw, max_weight=bound, clip_weight=False), w, "bf16x3")
    clipped.train_head_on_batch(xd, y)
    free.train_head_on_batch(xd, y)
    a, b = clipped.get_weight_dict(), free.get_weight_dict()
    for n in clipped.head_weight_names():
        assert np.abs(a[n]).max() <= np.float32(bound)
        assert same_bits(a[n], np.clip(b[n], -np.float32(bound), np.float32(bound))), n
    assert max(np.abs(b[n]).max() for n in free.head_weight_names()) > bound


@pytest.mark.parametrize("mode", ["float32", "float8"])
def test_unsupported_modes_raise(vtd, cuda, mode):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = build(vtd, kw, w, mode)
    xd = torch.from_numpy(x).to(cuda)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.train_head_on_batch(xd, y)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.fit_head(xd, y)


def test_needs_a_compiled_loss_and_an_optimizer(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    xd = torch.from_numpy(x).to(cuda)
    model = vtd.create_vision_transformer_detector(**kw, dtype="bf16x3")
    model.compile(optimizer="adam")                                # no loss
    assert isinstance(model.optimizer, vtd.optimizers.Adam)
    with pytest.raises(ValueError, match="compile"):
        model.train_head_on_batch(xd, y)
    model.compile(loss=functools.partial(vtd.my_custom_loss))      # no optimizer
    with pytest.raises(ValueError, match="optimizer"):
        model.train_head_on_batch(xd, y)
    with pytest.raises(ValueError, match="optimizer"):
        model.fit_head(xd, y)
    model.compile(optimizer=object(), loss=vtd.my_custom_loss)     # accepted, refused when used
    with pytest.raises(ValueError, match="unsupported optimizer"):
        model.train_head_on_batch(xd, y)
    assert model.optimizer is not None and same_bits(model.get_weights()[0], model.get_weights()[0])
