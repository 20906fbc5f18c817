"""Numerical health on the GPU: vtd_tensor_stats' records against the numpy oracle
(tests/health_oracle.py) on designed vectors -- every n around the vector width, the workgroup
size and the chunk size c, bases 0 / 4 / 8 / 12 bytes past a 16-B boundary, NaN / +inf / -inf at
element 0, the last element and both sides of a chunk boundary, all-NaN, a subnormal maximum,
-0.0 as the maximum, magnitudes 1e-20 .. 1e19 -- placement independence, the NaN-replaced copy,
and the model-level surface: weight_stats / gradient_stats / moment_stats / global_norm,
check_weights, check_inf_nan, and fit with CheckModelWeight and stop_training.

Exact fields are compared exactly (max / min by value), sumsq within n 2^-53 relative: the derived
bound of the oracle's docstring.  All designed vectors go through ONE table, so one launch pair
and one oracle pass serve the module."""
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import health_oracle as H
from tests.test_gpu_head_backward import load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def designed(vtd, cuda):
    """The designed vectors as slices of one device buffer, their records from one call, and the
    oracle's records (computed once, never changed)."""
    from vision_transformer_detector_amd import _lib as L
    table = H.designs(L.STATS_CHUNK)
    buf, spans = H.layout(table)
    dev = torch.from_numpy(buf).to(cuda)
    assert dev.data_ptr() % 16 == 0
    views = OrderedDict((name, dev[s:s + n]) for name, (s, n) in spans.items())
    for name, (off, _) in table.items():
        assert views[name].data_ptr() % 16 == 4 * off
    got = vtd.tensor_stats(views)
    want = OrderedDict((name, H.stats64(x)) for name, (_, x) in table.items())
    return dict(table=table, buf=buf, dev=dev, spans=spans, views=views, got=got, want=want,
                c=L.STATS_CHUNK)


def as_tuple(s):
    return (np.float32(s.max).tobytes(), np.float32(s.min).tobytes(), s.n, s.nan, s.pos_inf,
            s.neg_inf, np.float64(s.sumsq).tobytes())


def test_every_designed_record_equals_the_oracle(vtd, designed):
    assert list(designed["got"]) == list(designed["table"])
    wrong, worst = {}, 0.0
    for name, got in designed["got"].items():
        want = designed["want"][name]
        bad = H.mismatch(got, want)
        if bad:
            wrong[name] = bad
        if want["sumsq"]:
            worst = max(worst, abs(got.sumsq - want["sumsq"]) / want["sumsq"] / 2.0 ** -53)
        expect = H.norm(want)
        assert (math.isnan(got.norm) if math.isnan(expect) else
                got.norm == math.sqrt(got.sumsq) if math.isfinite(expect) else
                got.norm == math.inf), name
    print(f"worst sumsq deviation: {worst:.2f} x 2^-53 relative (bound: n)")
    assert not wrong, (len(wrong), dict(list(wrong.items())[:8]))
    # the run wrote nothing but its records: the vectors and the guard bands keep their bits
    assert H.same_bits(designed["dev"].cpu().numpy(), designed["buf"])


def test_special_values_are_counted_where_they_were_planted(vtd, designed):
    c = designed["c"]
    s = designed["got"][f"all_nan/n{2 * c + 7}/o1"]
    assert (s.nan, s.max, s.min, s.sumsq) == (2 * c + 7, -math.inf, math.inf, 0.0)
    assert math.isnan(s.norm) and not s.finite
    s = designed["got"][f"special_0/n{2 * c + 7}/o0"]
    assert (s.nan, s.pos_inf, s.neg_inf) == (2, 2, 2) and s.max == math.inf and s.min == -math.inf
    s = designed["got"]["subnormal_max/n257/o2"]
    assert 0.0 < s.max < float(np.finfo(np.float32).tiny) and s.finite
    s = designed["got"][f"negzero_max/n{c + 1}/o3"]
    assert s.max == 0.0 and s.min < 0.0
    s = designed["got"][f"plain/n{2 * c + 7}/o0"]
    assert s.sumsq > 1e38 and math.isfinite(s.norm)      # past what an fp32 sum could hold


def test_a_record_does_not_depend_on_placement_or_on_the_run(vtd, designed):
    c = designed["c"]
    views = designed["views"]
    fillers = [views[n] for n in (f"plain/n{c + 1}/o1", "special_1/n255/o3", f"all_nan/n{c}/o0",
                                  "plain/n5/o2", f"special_2/n{2 * c + 7}/o2", "plain/n1/o0")]
    for name in (f"special_0/n{2 * c + 7}/o0", f"plain/n{2 * c + 7}/o3", f"plain/n{c - 1}/o2",
                 "special_2/n1023/o1", "plain/n3/o0"):
        t = views[name]
        alone = vtd.tensor_stats(t)
        assert isinstance(alone, vtd.TensorStat)
        assert as_tuple(alone) == as_tuple(designed["got"][name]), name
        for at in (0, 3, 6):
            table = fillers[:at] + [t] + fillers[at:]
            got = vtd.tensor_stats(table)
            assert isinstance(got, list) and len(got) == 7
            assert as_tuple(got[at]) == as_tuple(alone), (name, at)
        assert as_tuple(vtd.tensor_stats(t)) == as_tuple(alone), name       # a second call


def nan_cases(designed):
    c = designed["c"]
    return [n for n in designed["table"]
            if n.startswith(("special_", "all_nan")) or n in (f"plain/n{c + 1}/o1", "plain/n4/o0")]


@pytest.mark.parametrize("replace_nan", [0.5, float("inf")])
def test_out_is_the_oracles_replace_out_of_place_and_aliased(vtd, designed, cuda, replace_nan):
    health = vtd.health
    names = nan_cases(designed)
    spans, buf = designed["spans"], designed["buf"]
    expect = buf.copy()
    for name in names:
        s, n = spans[name]
        expect[s:s + n] = H.replace(buf[s:s + n], replace_nan)
    src = [designed["views"][n] for n in names]
    # out of place: the same layout in a second buffer of sentinels, so the alignments match
    other = torch.full_like(designed["dev"], float(H.SENTINEL))
    outs = [other[spans[n][0]:spans[n][0] + spans[n][1]] for n in names]
    got = health._Plan(src, outs).run(replace_nan)
    want_other = np.full_like(buf, H.SENTINEL)
    for name in names:
        s, n = spans[name]
        want_other[s:s + n] = expect[s:s + n]
    assert H.same_bits(other.cpu().numpy(), want_other)             # guard bands included
    assert H.same_bits(designed["dev"].cpu().numpy(), buf)          # x untouched
    for name, s in zip(names, got):
        assert as_tuple(s) == as_tuple(designed["got"][name]), name     # the record of x
    # out at another alignment than x: a fresh, 16-B aligned tensor per vector
    few = [n for n in names if n.startswith("special_1/")]
    fresh = [torch.empty(spans[n][1], device=cuda) for n in few]
    health._Plan([designed["views"][n] for n in few], fresh).run(replace_nan)
    for name, t in zip(few, fresh):
        s, n = spans[name]
        assert H.same_bits(t.cpu().numpy(), expect[s:s + n]), name
    # aliased: out is x, in a copy of the buffer
    alias = designed["dev"].clone()
    xs = [alias[spans[n][0]:spans[n][0] + spans[n][1]] for n in names]
    got = health._Plan(xs, xs).run(replace_nan)
    assert H.same_bits(alias.cpu().numpy(), expect)
    for name, s in zip(names, got):
        assert as_tuple(s) == as_tuple(designed["got"][name]), name


def test_payload_bits_survive_the_copy(vtd, cuda):
    bits = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001,
                     0x807fffff, 0x7f7fffff, 0x7fa00000, 0x3f800000], np.uint32)   # 0x7fa..: sNaN
    x = torch.from_numpy(bits.view(np.float32).copy()).to(cuda)
    out = torch.empty_like(x)
    s, = vtd.health._Plan([x], [out]).run(-2.0)
    want = bits.copy()
    want[[0, 1, 8]] = np.float32(-2.0).view(np.uint32)
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert (s.nan, s.pos_inf, s.neg_inf, s.n) == (3, 1, 1, 10)
    assert H.mismatch(s, H.stats64(bits.view(np.float32))) == ""


def test_refusals(vtd, cuda):
    x = torch.zeros(8, 6, device=cuda)
    for bad in (x.double(), x.half(), x.t(), x[:, ::2], x.cpu(), torch.zeros(0, device=cuda)):
        with pytest.raises(ValueError):
            vtd.tensor_stats(bad)
    with pytest.raises(ValueError):
        vtd.tensor_stats([x, x.double()])
    with pytest.raises(ValueError):
        vtd.tensor_stats([])
    got = vtd.tensor_stats(OrderedDict(b=x, a=x[1:]))
    assert list(got) == ["b", "a"] and (got["a"].n, got["b"].n) == (42, 48)


# ------------------------------------------------------------------ model level
def build(vtd, kw, w, mode, lr=1e-3, **extra):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode, **extra)
    model.set_weights(w)
    model.compile(optimizer=vtd.optimizers.Adam(learning_rate=lr, clipvalue=10),
                  loss=functools.partial(vtd.my_custom_loss))
    return model


def assert_records(got, arrays):
    assert list(got) == list(arrays)
    for name, a in arrays.items():
        bad = H.mismatch(got[name], H.stats64(a))
        assert not bad, (name, bad)


def host(d):
    return OrderedDict((n, t.cpu().numpy()) for n, t in d.items())


@pytest.fixture(scope="module")
def case():
    return load_case("tiny_mish", 3)


def test_weight_gradient_and_moment_stats_follow_the_device(vtd, cuda, case):
    kw, w, x, y = case
    model = build(vtd, kw, w, "bf16x3")
    xd = torch.from_numpy(x).to(cuda)
    assert_records(model.weight_stats(), model.get_weight_dict())
    assert list(model.weight_stats()) == model.weight_names()
    model.train_on_batch(xd, y)
    _, grads = model.gradients(xd, y)                # of the weights the second step starts from
    model.train_on_batch(xd, y)
    # first, so it must have read the device masters: the host copies are still the old ones
    assert model._enc_dirty and model._head_dirty
    stepped = model.weight_stats()
    assert model._enc_dirty and model._head_dirty    # and it read nothing back
    assert_records(stepped, model.get_weight_dict())
    assert any(stepped[n].sumsq != H.stats64(w[n])["sumsq"] for n in stepped)
    opt = model.optimizer
    grads = host(grads)
    assert_records(opt.gradient_stats(model), grads)
    n = sum(g.size for g in grads.values())
    want = math.sqrt(math.fsum(H.stats64(g)["sumsq"] for g in grads.values()))
    got = opt.global_norm(model)
    print(f"global_norm {got!r} vs fp64 {want!r}, n = {n}")
    assert isinstance(got, float) and abs(got - want) <= n * 2.0 ** -53 * want
    m, v = opt.moments(model)
    ms, vs = opt.moment_stats(model)
    assert_records(ms, host(m))
    assert_records(vs, host(v))
    assert all(s.min >= 0.0 for s in vs.values())
    # a new set of weights: the cached plan follows the new masters
    model.set_weights(w)
    assert_records(model.weight_stats(), {n: np.asarray(a, np.float32) for n, a in
                                          model.get_weight_dict().items()})


def test_weight_stats_in_a_mode_that_does_not_train(vtd, cuda, case):
    kw, w, _, _ = case
    model = vtd.create_vision_transformer_detector(**kw, dtype="float32")
    model.set_weights(w)
    assert_records(model.weight_stats(), model.get_weight_dict())


def test_check_weights_is_the_reference_arithmetic(vtd, cuda, case, capsys):
    kw, w, _, _ = case
    model = build(vtd, kw, w, "bf16x3")
    got = vtd.check_weights(model)
    assert got == H.check_weights_ref(model.get_weight_dict())
    text = capsys.readouterr().out
    assert "Checking the weights ..." in text
    assert f"The status is OK, max_weight is: {got:.1f}" in text and "Alert" not in text
    # a NaN in the tensor that holds the largest weight: the maximum over the other tensors
    wd = model.get_weight_dict()
    top = max(wd, key=lambda n: wd[n].max())
    assert wd[top].max() == got
    wd[top].reshape(-1)[0] = np.nan
    model.set_weights(wd)
    second = vtd.check_weights(model)
    assert second == H.check_weights_ref(wd) == max(a.max() for n, a in wd.items() if n != top)
    assert second < got
    text = capsys.readouterr().out
    assert f"{top}: 1 NaN, 0 +Inf, 0 -Inf of {wd[top].size}" in text
    # above the red line
    wd[top].reshape(-1)[0] = 0.0
    wd["dense/bias"][3] = 777.25
    model.set_weights(wd)
    assert vtd.check_weights(model) == 777.25 == H.check_weights_ref(wd)
    text = capsys.readouterr().out
    assert "Alert! max_weight is: 777.2" in text and "use a smaller learning_rate" in text
    assert "NaN or Inf found" not in text
    # nothing positive: the reference starts from 0
    model.set_weights({n: -np.abs(a) - 1 for n, a in wd.items()})
    assert vtd.check_weights(model) == 0


def test_check_inf_nan(vtd, cuda, capsys):
    x = torch.linspace(-3, 3, 40, device=cuda).reshape(5, 8)
    assert vtd.check_inf_nan(x, "x") is x and capsys.readouterr().out == ""
    assert vtd.check_inf_nan(x, "x", replace_nan=0.0) is x           # no NaN: the object itself
    assert vtd.check_inf_nan(x, "x", max_value=2) is x
    text = capsys.readouterr().out
    assert "In x, its shape:  (5, 8)" in text and "max_value:  3.0" in text
    bad = x.clone()
    bad[1, 2], bad[4, 7], bad[0, 0] = float("nan"), float("inf"), float("nan")
    assert vtd.check_inf_nan(bad, "act") is bad                       # replace_nan None
    text = capsys.readouterr().out
    assert "Inf! Found in act, its shape:  (5, 8)" in text
    assert "NaN! Found in act, its shape:  (5, 8)" in text and "max_value" not in text
    before = bad.clone()
    fixed = vtd.check_inf_nan(bad, "act", replace_nan=-1.5)
    assert fixed is not bad and fixed.shape == bad.shape and fixed.device == bad.device
    assert H.same_bits(fixed.cpu().numpy(), H.replace(before.cpu().numpy(), -1.5))
    assert H.same_bits(bad.cpu().numpy(), before.cpu().numpy())      # the input is not written
    assert "max_value:  inf" in capsys.readouterr().out                # the +inf is the maximum
    # numpy in, numpy out
    a = before.cpu().numpy()
    assert vtd.check_inf_nan(a[2:4], "a") is not None and capsys.readouterr().out == ""
    rows = a[2:4]
    assert vtd.check_inf_nan(rows, "a") is rows
    fixed = vtd.check_inf_nan(a, "a", replace_nan=9.0)
    assert isinstance(fixed, np.ndarray) and H.same_bits(fixed, H.replace(a, 9.0))
    capsys.readouterr()
    # the tuple branch: name_i, one launch, the tuple itself comes back
    pair = (x, 3, bad, x[3:] * 1e5)
    assert vtd.check_inf_nan(pair, "out", replace_nan=0.0) is pair
    text = capsys.readouterr().out
    assert "Inf! Found found in out_2, its shape:  (5, 8)" in text
    assert "NaN! Found in out_2, its shape:  (5, 8)" in text and "out_0" not in text
    assert "In out_2, its shape:  (5, 8)" in text and "max_value change to:  inf" in text
    assert "out_3" not in text                        # 3e5 does not exceed the maximum so far
    vtd.check_inf_nan((x, x[3:] * 1e5), "out")
    text = capsys.readouterr().out
    assert "In out_1, its shape:  (2, 8)" in text and "max_value change to:  300000.0" in text
    with pytest.raises(ValueError):
        vtd.check_inf_nan(x.double(), "x")


class Recorder:
    def __init__(self):
        self.weights = []

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        self.weights.append(self.model.get_weight_dict())


class StopAt:
    def __init__(self, epoch):
        self.epoch = epoch

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        if epoch == self.epoch:
            self.model.stop_training = True


def test_fit_with_check_model_weight_and_stop_training(vtd, cuda, case, capsys):
    kw, w, x, y = case
    xd = torch.from_numpy(x).to(cuda)
    model = build(vtd, kw, w, "bf16x3", lr=1e-2)
    cb, rec = vtd.CheckModelWeight(1, 1, 0.0), Recorder()
    hist = model.fit(xd, y, batch_size=3, epochs=3, callbacks=[cb, rec])
    assert hist.epoch == [0, 1, 2] and len(rec.weights) == 3 and model.stop_training is False
    ref = H.CheckModelWeightRef(1, 1, 0.0)
    for e, wd in enumerate(rec.weights):
        ref.on_epoch_end(e, wd)
    assert ref.checked == [1, 2]
    assert (cb.max_weight, cb.min_weight) == (ref.max_weight, ref.min_weight)
    assert cb.max_weight > 0.0 and "Largest_weight changed to: " in capsys.readouterr().out
    # a callback that sets stop_training in epoch 0: one epoch; the next fit starts afresh
    hist = model.fit(xd, y, batch_size=3, epochs=3, callbacks=[StopAt(0)])
    assert hist.epoch == [0] and model.stop_training is True
    hist = model.fit_head(xd, y, batch_size=3, epochs=0)
    assert hist.epoch == [] and model.stop_training is False
    # a NaN planted before fit (the position embedding has no ClipWeight to turn it into 1.0):
    # stop_on_nan ends fit after the first check, at epoch 1
    wd = model.get_weight_dict()
    pos = "position_encoding/position_embedding/embeddings"
    wd[pos].reshape(-1)[0] = np.nan
    model = build(vtd, kw, wd, "bf16x3")
    hist = model.fit(xd, y, batch_size=3, epochs=4,
                     callbacks=[vtd.CheckModelWeight(1, 1, 0.0, stop_on_nan=True)])
    assert hist.epoch == [0, 1] and len(hist.history["loss"]) == 2 and model.stop_training
    assert f"{pos}: " in capsys.readouterr().out
    # fit_head takes callbacks too
    model = build(vtd, kw, w, "bf16x3")
    head_cb = vtd.CheckModelWeight(0, 2, 0.0)
    hist = model.fit_head(xd, y, batch_size=3, epochs=3, callbacks=[head_cb, StopAt(1)])
    assert hist.epoch == [0, 1] and head_cb.max_weight > 0.0
