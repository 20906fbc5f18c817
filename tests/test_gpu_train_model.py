"""Model.train_on_batch / fit on the GPU: the optimizer step over every weight at model level.

The step's arithmetic is pinned bit for bit: every weight and both moments after a step equal the
host oracle (tests/adam_oracle.py step32; tests/train_oracle.py sparse32 for the position
embedding) applied to the previous weights with the gradients Model.gradients returns for the
same state.  The invariant -- the device masters and every packed operand hold what a fresh
model's set_weights(get_weight_dict()) would build -- is checked through the inference forward
(packed operands, folded ones included) and through gradients (device masters), bit for bit.  The
trajectory test compares five steps with the float64 whole-model oracle
(train_oracle.model_trajectory).
"""
import functools

import numpy as np
import pytest
import torch

from tests import train_oracle as T
from tests.test_gpu_head_backward import load_case

pytestmark = pytest.mark.gpu
CASES = [("tiny_mish", 3), ("tiny_gelu", 2), ("multi_tile", 16)]
MODES = ["bf16x3", "bfloat16"]
LR = 1e-3
# the number of steps after which the float64 oracle's own loss on tiny_mish (B = 3, lr 1e-3,
# clipvalue 10) has fallen by at least 10 % (97.57 -> 85.71 after one): found on the CPU,
# asserted again by the test
DESCENT_STEPS = 1
# worst relative deviation of the device's five losses from the float64 trajectory measured on
# the MI355X (bf16x3, tiny_mish, B = 3), and the bar at 4 x that
TRAJECTORY_MEASURED = 1.76e-6
TRAJECTORY_BAR = 4 * TRAJECTORY_MEASURED          # 7.04e-6


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


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_one_step_is_the_host_oracle_on_the_model_gradients(vtd, cuda, case, mode):
    kw, w, x, y = load_case(*case)
    model = build(vtd, kw, w, mode)
    xd = torch.from_numpy(x).to(cuda)
    names = model.weight_names()
    before = model.get_weight_dict()
    out5_ref, grads = model.gradients(xd, y)
    out5 = model.train_on_batch(xd, y)
    assert torch.equal(out5, out5_ref)
    assert model.optimizer.iterations == 1
    after = model.get_weight_dict()
    mom_m, mom_v = model.optimizer.moments(model)
    assert list(mom_m) == names and list(model.optimizer.gradient_buffers(model)) == names
    live = dict(model._encoder_master(), **model._head_master())
    m1, v1 = {}, {}
    for n in names:
        z = np.zeros_like(before[n])
        want, m1[n], v1[n] = T.host_step(n, before[n], z, z, host(grads[n]), 1, LR)
        assert same_bits(after[n], want), n
        assert same_bits(host(live[n]), want), n
        assert same_bits(host(mom_m[n]), m1[n]) and same_bits(host(mom_v[n]), v1[n]), n
        assert not same_bits(after[n], before[n]), n
        assert same_bits(host(model.optimizer.gradient_buffers(model)[n]), host(grads[n])), n
    # a second step continues from the moments (t = 2)
    _, grads = model.gradients(xd, y)
    model.train_on_batch(xd, y)
    assert model.optimizer.iterations == 2
    again = model.get_weight_dict()
    for n in names:
        want, m2, v2 = T.host_step(n, after[n], m1[n], v1[n], host(grads[n]), 2, LR)
        assert same_bits(again[n], want), n
        assert same_bits(host(mom_m[n]), m2) and same_bits(host(mom_v[n]), v2), n


def check_live(vtd, cuda, kw, model, mode, xd, y, tmp_path):
    """The invariant after steps: a fresh model given get_weight_dict() computes the same bits,
    in the inference forward (every packed operand) and in gradients (the device masters)."""
    logits = model(xd)
    fresh = build(vtd, kw, model.get_weight_dict(), mode)
    assert torch.equal(fresh(xd), logits)
    out5, grads = model.gradients(xd, y)
    out5_f, grads_f = fresh.gradients(xd, y)
    assert torch.equal(out5, out5_f)
    for n in model.weight_names():
        assert torch.equal(grads[n], grads_f[n]), n
    assert [same_bits(a, b) for a, b in zip(model.get_weights(), fresh.get_weights())] == \
        [True] * len(model.weight_names())
    # encoder_block_weights / stem_weights hand out the trained tensors
    trained = model.get_weight_dict()
    handed = dict(model.stem_weights())
    for i in range(model.kwargs["encoder_repeat_times"]):
        handed.update(model.encoder_block_weights(i))
    assert len(handed) == len(trained) - len(model.head_weight_names())
    for n, t in handed.items():
        assert same_bits(host(t), trained[n]), n
    return logits


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_masters_and_packed_operands_are_live_and_weights_round_trip(vtd, cuda, case, mode,
                                                                      tmp_path):
    kw, w, x, y = load_case(*case)
    model = build(vtd, kw, w, mode)
    # bfloat16 packs with the LayerNorm fold: two jobs per block; bf16x3 has none
    reps = model.kwargs["encoder_repeat_times"]
    assert len(model._fold_jobs) == (2 * reps if mode == "bfloat16" else 0)
    xd = torch.from_numpy(x).to(cuda)
    untrained = model(xd).clone()
    start = model.get_weight_dict()
    for _ in range(3):
        model.train_on_batch(xd, y)
    logits = check_live(vtd, cuda, kw, model, mode, xd, y, tmp_path)
    assert not torch.equal(logits, untrained)
    trained = model.get_weight_dict()
    assert all(not same_bits(trained[n], start[n]) for n in trained)
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
    m, v = model.optimizer.moments(model, scope="all")
    assert list(m) == model.weight_names()
    assert all(not t.any() for t in m.values()) and all(not t.any() for t in v.values())
    assert torch.equal(model(xd), logits)


def test_a_model_packed_without_the_fold_has_no_second_launch(vtd, cuda, monkeypatch, tmp_path):
    monkeypatch.setenv("VTD_LN_FOLD", "0")
    kw, w, x, y = load_case("tiny_mish", 3)
    model = build(vtd, kw, w, "bfloat16")
    assert model._fold_jobs == []
    xd = torch.from_numpy(x).to(cuda)
    for _ in range(3):
        model.train_on_batch(xd, y)
    # what _pack decided holds, whatever the switch says when the steps run
    monkeypatch.delenv("VTD_LN_FOLD")
    folded = build(vtd, kw, w, "bfloat16")
    assert len(folded._fold_jobs) == 2 * model.kwargs["encoder_repeat_times"]
    monkeypatch.setenv("VTD_LN_FOLD", "0")
    for _ in range(3):
        folded.train_on_batch(xd, y)
    assert [same_bits(a, b) for a, b in zip(model.get_weights(), folded.get_weights())] == \
        [True] * len(model.weight_names())
    check_live(vtd, cuda, kw, model, "bfloat16", xd, y, tmp_path)          # fresh: unfolded too
    monkeypatch.delenv("VTD_LN_FOLD")
    check_live(vtd, cuda, kw, folded, "bfloat16", xd, y, tmp_path)         # fresh: folded too


def test_trajectory_follows_the_float64_oracle(vtd, cuda):
    """Five steps at lr 1e-3, clipvalue 10, tiny_mish B = 3, bf16x3: the device's losses against
    the float64 whole-model oracle's.  The bar is 4 x the worst relative deviation measured on
    the MI355X: 1.76e-6 (TRAJECTORY_MEASURED; the five were 5.8e-8, 1.3e-6, 5.2e-7, 1.4e-6,
    1.76e-6), bar 7.04e-6.  For scale: the fp32 CPU port of the same trajectory (float32
    autograd, step32) deviates by 5.2e-8 at worst, so the device is some 30 x above fp32
    arithmetic.  That is the mode, not the step: the CPU emulation of the device's chain of
    split-bf16 roundings (model_grad_oracle.emulated_model_backward in 'bf16x3', loss in
    float64, step32) deviates by 2.2e-7, 7.3e-7, 1.9e-7, 6.6e-7, 1.6e-6 over the same five
    steps, the device's order; a split-bf16 product drops the lo x lo term (2^-16 relative),
    where an fp32 product rounds at 2^-24.  The head-only trajectory (test_gpu_fit_head.py)
    measured 2.37e-6 in the same mode.  After DESCENT_STEPS step(s) the oracle's own loss has
    fallen by 10 % and the device's is below its first."""
    kw, w, x, y = load_case("tiny_mish", 3)
    model = build(vtd, kw, w, "bf16x3")
    xd = torch.from_numpy(x).to(cuda)
    ref = T.model_trajectory(kw, w, x, y, 5, LR)
    got = [model.train_on_batch(xd, y) for _ in range(5)]
    got = [float(v) for v in torch.stack(got)[:, 0].cpu()]
    dev = [abs(a - b) / abs(b) for a, b in zip(got, ref)]
    print("device losses", got, "oracle", ref, "relative deviation", dev,
          f"worst {max(dev):.3g}")
    assert max(dev) <= TRAJECTORY_BAR
    assert ref[DESCENT_STEPS] <= 0.9 * ref[0] < min(ref[:DESCENT_STEPS])
    assert got[DESCENT_STEPS] < got[0]


class Recorder:
    def __init__(self):
        self.model, self.calls = [], []

    def set_model(self, model):
        self.model.append(model)

    def on_epoch_end(self, epoch, logs):
        self.calls.append((epoch, dict(logs)))


class EndOnly:
    """A callback without set_model."""

    def __init__(self):
        self.epochs = []

    def on_epoch_end(self, epoch, logs):
        self.epochs.append(epoch)


def test_fit_history_batches_schedule_and_callbacks(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 5)
    xd = torch.from_numpy(x).to(cuda)
    # an identical second model, stepped by hand over batches of 2, 2, 1 for two epochs
    manual = build(vtd, kw, w, "bf16x3")
    want = []
    for _ in range(2):
        total, count = 0.0, 0
        for i in range(0, 5, 2):
            out5 = manual.train_on_batch(xd[i:i + 2], y[i:i + 2])
            n = len(y[i:i + 2])
            total += float(out5[0].double()) * n
            count += n
        want.append(total / count)
    model = build(vtd, kw, w, "bf16x3")
    rec, end = Recorder(), EndOnly()
    hist = model.fit(xd, y, batch_size=2, epochs=2, callbacks=[rec, end])
    assert hist.history["loss"] == want and hist.epoch == [0, 1]
    assert model.optimizer.iterations == 6
    assert rec.model == [model] and rec.calls == [(0, {"loss": want[0]}), (1, {"loss": want[1]})]
    assert end.epochs == [0, 1]
    for a, b in zip(model.get_weights(), manual.get_weights()):
        assert same_bits(a, b)
    # a re-iterable of batches with y=None
    model = build(vtd, kw, w, "bf16x3")
    hist = model.fit([(xd[i:i + 2], y[i:i + 2]) for i in range(0, 5, 2)], epochs=2)
    assert hist.history["loss"] == want
    # the reference's step schedule: called with (epoch, current lr) at the start of each epoch
    opt = vtd.optimizers
    opt._allowed_decay_times.assign(3)
    schedule = functools.partial(opt.learning_rate_step_decay, epochs_first_lr_decay=1,
                                 epochs_second_lr_decay=5, epochs_third_lr_decay=5,
                                 rate_lr_decay=0.5)
    try:
        model = build(vtd, kw, w, "bf16x3")
        model.fit(xd, y, batch_size=5, epochs=2, lr_schedule=schedule)
        assert model.optimizer.learning_rate == LR * 0.5
        assert int(opt._allowed_decay_times.numpy()) == 2
    finally:
        opt._allowed_decay_times.assign(3)
    other = build(vtd, kw, w, "bf16x3")
    other.train_on_batch(xd, y)                                    # epoch 0 at LR
    w1 = other.get_weight_dict()
    m1, v1 = other.optimizer.moments(other)
    _, grads = other.gradients(xd, y)
    got = model.get_weight_dict()
    for n in model.weight_names():
        expect, _, _ = T.host_step(n, w1[n], host(m1[n]), host(v1[n]), host(grads[n]), 2, LR * 0.5)
        assert same_bits(got[n], expect), n


def test_clip_weight_false_and_max_weight_reach_the_kernel(vtd, cuda):
    """With max_weight below the weights' range the step clips every weight to it but the
    position embedding, which the reference leaves unconstrained; clip_weight=False leaves all
    of them free."""
    kw, w, x, y = load_case("tiny_mish", 3)
    xd = torch.from_numpy(x).to(cuda)
    bound = 0.01
    clipped = build(vtd, dict(kw, max_weight=bound), w, "bf16x3")
    free = build(vtd, dict(kw, max_weight=bound, clip_weight=False), w, "bf16x3")
    clipped.train_on_batch(xd, y)
    free.train_on_batch(xd, y)
    a, b = clipped.get_weight_dict(), free.get_weight_dict()
    for n in clipped.weight_names():
        if n == T.POS:
            assert same_bits(a[n], b[n]) and np.abs(a[n]).max() > bound
        else:
            assert np.abs(a[n]).max() <= np.float32(bound)
            assert same_bits(a[n], np.clip(b[n], -np.float32(bound), np.float32(bound))), n
    assert max(np.abs(v).max() for v in b.values()) > bound


def test_scopes_do_not_mix_on_one_optimizer(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    xd = torch.from_numpy(x).to(cuda)
    model = build(vtd, kw, w, "bf16x3")
    model.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="train_on_batch / fit.*compile a new optimizer"):
        model.train_head_on_batch(xd, y)
    with pytest.raises(ValueError, match="compile a new optimizer"):
        model.fit_head(xd, y)
    model = build(vtd, kw, w, "bf16x3")
    model.train_head_on_batch(xd, y)
    with pytest.raises(ValueError, match="train_head_on_batch / fit_head.*compile a new optimizer"):
        model.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="compile a new optimizer"):
        model.fit(xd, y)
    # a new optimizer switches; so does one that has taken no step
    model.compile(optimizer=vtd.optimizers.Adam(LR, clipvalue=10), loss=model.loss)
    assert len(model.optimizer.moments(model)[0]) == len(model.head_weight_names())
    model.train_on_batch(xd, y)
    assert len(model.optimizer.moments(model)[0]) == len(model.weight_names())


@pytest.mark.parametrize("mode", ["float32", "float8"])
def test_unsupported_modes_raise(vtd, cuda, mode):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = build(vtd, kw, w, mode)
    xd = torch.from_numpy(x).to(cuda)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.fit(xd, y)


def test_needs_a_compiled_loss_an_optimizer_and_no_dropout(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    xd = torch.from_numpy(x).to(cuda)
    model = vtd.create_vision_transformer_detector(**kw, dtype="bf16x3")
    model.compile(optimizer="adam")                                # no loss
    with pytest.raises(ValueError, match="compile"):
        model.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="compile"):
        model.fit(xd, y)
    model.compile(loss=functools.partial(vtd.my_custom_loss))      # no optimizer
    with pytest.raises(ValueError, match="optimizer"):
        model.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="optimizer"):
        model.fit(xd, y)
    model.compile(optimizer=object(), loss=vtd.my_custom_loss)
    with pytest.raises(ValueError, match="unsupported optimizer"):
        model.train_on_batch(xd, y)
    dropped = build(vtd, dict(kw, dropout=0.1), w, "bf16x3")
    with pytest.raises(ValueError, match="dropout"):
        dropped.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="dropout"):
        dropped.fit(xd, y)
    assert build(vtd, dict(kw, dropout=0.0), w, "bf16x3").train_on_batch(xd, y).shape == (5,)
