"""Model.train_on_batch / fit / train_head_on_batch / fit_head on a model built with `dropout` and
compiled with a `dropout_seed`, on the GPU.

The step's arithmetic is pinned as tests/test_gpu_train_model.py pins it: the losses a step
returns and every weight and moment after it equal the host oracle (train_oracle.host_step)
applied to the gradients Model.gradients(step=t) returns for the same state, t the optimizer's
`iterations` as read before the step.  What those gradients are is tests/test_gpu_model_dropout.py's
matter.
"""
import functools

import numpy as np
import pytest
import torch

from tests import model_dropout_oracle as R
from tests import train_oracle as T

pytestmark = pytest.mark.gpu
CASES = R.CASES
MODES = ["bf16x3", "bfloat16"]
LR = 1e-3

modes = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
rates = pytest.mark.parametrize("rate", R.RATES)


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


def build(vtd, kw, w, mode, lr=LR, **compile_kw):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    model.set_weights(w)
    model.compile(optimizer=vtd.optimizers.Adam(learning_rate=lr, clipvalue=10),
                  loss=functools.partial(vtd.my_custom_loss), **compile_kw)
    return model


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def host(t):
    return t.cpu().numpy()


@rates
@modes
@cases
def test_steps_are_the_host_oracle_on_the_gradients_of_their_step(vtd, cuda, case, mode, rate):
    kw, w, x, y = R.load_case(*case)
    model = build(vtd, dict(kw, dropout=rate), w, mode, dropout_seed=R.SEED)
    xd = torch.from_numpy(x).to(cuda)
    names = model.weight_names()
    before = model.get_weight_dict()
    out5_ref, grads = model.gradients(xd, y, step=0)
    out5_other, _ = model.gradients(xd, y, step=1)
    assert not torch.equal(out5_ref, out5_other)
    out5 = model.train_on_batch(xd, y)
    assert torch.equal(out5, out5_ref)
    assert model.optimizer.iterations == 1
    after = model.get_weight_dict()
    mom_m, mom_v = model.optimizer.moments(model)
    m1, v1 = {}, {}
    for n in names:
        z = np.zeros_like(before[n])
        want, m1[n], v1[n] = T.host_step(n, before[n], z, z, host(grads[n]), 1, LR)
        assert same_bits(after[n], want), n
        assert same_bits(host(mom_m[n]), m1[n]) and same_bits(host(mom_v[n]), v1[n]), n
        assert same_bits(host(model.optimizer.gradient_buffers(model)[n]), host(grads[n])), n
    # the second step takes the masks of step 1
    out5_ref, grads = model.gradients(xd, y, step=1)
    out5_zero, _ = model.gradients(xd, y, step=0)
    assert not torch.equal(out5_ref, out5_zero)
    out5 = model.train_on_batch(xd, y)
    assert torch.equal(out5, out5_ref)
    assert model.optimizer.iterations == 2
    again = model.get_weight_dict()
    for n in names:
        want, m2, v2 = T.host_step(n, after[n], m1[n], v1[n], host(grads[n]), 2, LR)
        assert same_bits(again[n], want), n
        assert same_bits(host(mom_m[n]), m2) and same_bits(host(mom_v[n]), v2), n


@modes
def test_the_seed_decides_the_trajectory(vtd, cuda, mode):
    kw, w, x, y = R.load_case("ragged_head", 3)
    xd = torch.from_numpy(x).to(cuda)
    kw = dict(kw, dropout=0.5)
    trained = []
    for seed in (R.SEED, R.SEED, R.OTHER_SEED):
        model = build(vtd, kw, w, mode, dropout_seed=seed)
        losses = torch.stack([model.train_on_batch(xd, y) for _ in range(3)])
        assert bool(torch.isfinite(losses).all())
        trained.append(model.get_weights())
    assert all(same_bits(a, b) for a, b in zip(trained[0], trained[1]))
    assert not all(same_bits(a, b) for a, b in zip(trained[0], trained[2]))


@rates
@modes
@cases
def test_frozen_encoder_steps_take_the_heads_sites_only(vtd, cuda, case, mode, rate):
    kw, w, x, y = R.load_case(*case)
    model = build(vtd, dict(kw, dropout=rate), w, mode, dropout_seed=R.SEED)
    xd = torch.from_numpy(x).to(cuda)
    feats = model.encode(xd)
    # encode is the inference forward, with or without the seed
    assert torch.equal(feats, build(vtd, kw, w, mode).encode(xd))
    head = model.head_weight_names()
    before = model.get_weight_dict()
    for t in range(2):
        out5_ref, grads = model.head_gradients(None, y, encoded=feats, step=t)
        assert model.optimizer.iterations == t
        out5 = model.train_head_on_batch(None, y, encoded=feats)
        assert torch.equal(out5, out5_ref)
        buffers = model.optimizer.gradient_buffers(model, scope="head")
        assert list(buffers) == head
        for n in head:
            assert torch.equal(buffers[n], grads[n]), (t, n)
    out5_three, _ = model.head_gradients(None, y, encoded=feats, step=3)
    assert not torch.equal(out5_three, model.head_gradients(None, y, encoded=feats, step=2)[0])
    after = model.get_weight_dict()
    for n in model.weight_names():
        assert same_bits(after[n], before[n]) == (n not in head), n


@modes
def test_fit_head_with_cached_features_counts_the_steps(vtd, cuda, mode):
    kw, w, x, y = R.load_case("ragged_head", 4)
    xd = torch.from_numpy(x).to(cuda)
    kw = dict(kw, dropout=0.1)
    manual = build(vtd, kw, w, mode, dropout_seed=R.SEED)
    feats = {i: manual.encode(xd[i:i + 2]) for i in range(0, 4, 2)}     # as fit_head caches them
    step = 0
    for _ in range(2):                                   # two epochs over batches of 2
        for i in range(0, 4, 2):
            ref5, grads = manual.head_gradients(None, y[i:i + 2], encoded=feats[i], step=step)
            out5 = manual.train_head_on_batch(None, y[i:i + 2], encoded=feats[i])
            assert torch.equal(out5, ref5)
            step += 1
    model = build(vtd, kw, w, mode, dropout_seed=R.SEED)
    hist = model.fit_head(xd, y, batch_size=2, epochs=2)
    assert model.optimizer.iterations == 4 and all(np.isfinite(hist.history["loss"]))
    for a, b in zip(model.get_weights(), manual.get_weights()):
        assert same_bits(a, b)
    enc_names = [n for n in model.weight_names() if n not in model.head_weight_names()]
    start, end = manual.get_weight_dict(), model.get_weight_dict()
    assert all(same_bits(end[n], w[n]) and same_bits(start[n], w[n]) for n in enc_names)


@modes
def test_fit_runs_and_leaves_the_model_live(vtd, cuda, mode):
    kw, w, x, y = R.load_case("ragged_head", 5)
    xd = torch.from_numpy(x).to(cuda)
    kw = dict(kw, dropout=0.1)
    model = build(vtd, kw, w, mode, dropout_seed=R.SEED)
    hist = model.fit(xd, y, batch_size=2, epochs=2)
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"]))
    assert model.optimizer.iterations == 6
    # the invariant of test_gpu_train_model.check_live: a fresh model given get_weight_dict()
    # computes the same inference logits, bit for bit
    logits = model(xd)
    fresh = build(vtd, kw, model.get_weight_dict(), mode)
    assert torch.equal(fresh(xd), logits)
    assert not torch.equal(logits, build(vtd, kw, w, mode)(xd))
    # the same steps by hand
    manual = build(vtd, kw, w, mode, dropout_seed=R.SEED)
    for _ in range(2):
        for i in range(0, 5, 2):
            manual.train_on_batch(xd[i:i + 2], y[i:i + 2])
    for a, b in zip(model.get_weights(), manual.get_weights()):
        assert same_bits(a, b)


def test_no_seed_raises_and_rate_zero_is_the_dropout_none_model(vtd, cuda):
    kw, w, x, y = R.load_case("tiny_mish", 2)
    xd = torch.from_numpy(x).to(cuda)
    dropped = build(vtd, dict(kw, dropout=0.1), w, "bf16x3")
    with pytest.raises(ValueError, match="dropout"):
        dropped.train_on_batch(xd, y)
    with pytest.raises(ValueError, match="dropout"):
        dropped.fit(xd, y)
    # compiling the seed makes the same model trainable; compiling again without it does not
    dropped.compile(optimizer=dropped.optimizer, loss=dropped.loss, dropout_seed=R.SEED)
    assert dropped.train_on_batch(xd, y).shape == (5,)
    dropped.compile(optimizer=dropped.optimizer, loss=dropped.loss)
    with pytest.raises(ValueError, match="dropout"):
        dropped.train_on_batch(xd, y)
    plain = build(vtd, kw, w, "bf16x3")
    zero = build(vtd, dict(kw, dropout=0.0), w, "bf16x3", dropout_seed=R.SEED)
    unseeded_head = build(vtd, dict(kw, dropout=0.1), w, "bf16x3")
    plain_head = build(vtd, kw, w, "bf16x3")
    for _ in range(2):
        assert torch.equal(zero.train_on_batch(xd, y), plain.train_on_batch(xd, y))
        assert torch.equal(unseeded_head.train_head_on_batch(xd, y),
                           plain_head.train_head_on_batch(xd, y))
    for a, b in zip(zero.get_weights(), plain.get_weights()):
        assert same_bits(a, b)
    for a, b in zip(unseeded_head.get_weights(), plain_head.get_weights()):
        assert same_bits(a, b)
