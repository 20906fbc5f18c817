"""Numerical health without a GPU: the oracle's self-checks and its sumsq bound, the C ABI's
new entries and every argument check (fake addresses, rejected before any device call and never
dereferenced), the plan's sizes, the Python surface, and CheckModelWeight's bookkeeping against
the reference arithmetic with `weight_stats` stubbed."""
import ctypes
import inspect
import math
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pytest

from tests import health_oracle as H


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def vtd():
    import vision_transformer_detector_amd as m
    return m


# ------------------------------------------------------------------ the oracle
def test_oracle_records_of_hand_made_vectors():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    s = H.stats64(np.array([1.0, nan, -2.0, inf, -inf, inf, 0.5], np.float32))
    assert (s["n"], s["nan"], s["pos_inf"], s["neg_inf"]) == (7, 1, 2, 1)
    assert s["max"] == inf and s["min"] == -inf and s["sumsq"] == 5.25
    assert math.isnan(H.norm(s))                                  # a NaN wins over the infinities
    assert math.isinf(H.norm(H.stats64(np.array([1.0, -inf], np.float32))))
    s = H.stats64(np.array([nan, nan], np.float32))
    assert (s["nan"], s["max"], s["min"], s["sumsq"]) == (2, -inf, inf, 0.0)
    assert math.isnan(H.norm(s))
    s = H.stats64(np.array([-3.0, -0.0, -1.0], np.float32))
    assert s["max"] == 0.0 and s["min"] == -3.0 and H.norm(s) == math.sqrt(10.0)
    s = H.stats64(np.array([-1.0, 3e-42], np.float32))
    assert 0.0 < s["max"] < np.finfo(np.float32).tiny             # the subnormal is kept
    # fp32 squares of these overflow and underflow; the fp64 sum is exact
    s = H.stats64(np.array([1e30, 1e-30, -1e30], np.float32))
    exact = sum(Fraction(float(v)) ** 2 for v in np.array([1e30, 1e-30, -1e30], np.float32))
    assert Fraction(s["sumsq"]) == Fraction(float(exact)) and s["sumsq"] > 1e59


def test_oracle_replace_keeps_every_other_bit():
    x = np.array([1.0, np.nan, np.inf, -np.inf, -0.0, 3e-42], np.float32)
    x.view(np.uint32)[1] = 0x7fc12345                              # a NaN with a payload
    y = H.replace(x, 7.5)
    assert y[1] == np.float32(7.5)
    keep = [0, 2, 3, 4, 5]
    assert (y.view(np.uint32)[keep] == x.view(np.uint32)[keep]).all()
    assert H.same_bits(H.replace(x[keep], 1.0), x[keep])
    assert np.isnan(H.replace(x, np.nan)[1])


def test_designs_cover_what_they_claim(L):
    c = L.STATS_CHUNK
    table = H.designs(c)
    assert len(table) == 13 * 4 * 7 and c == 16384
    assert sorted({x.size for _, x in table.values()}) == sorted(H.NS(c))
    # each special at element 0, the last element and both sides of a chunk boundary
    seen = set()
    for name, (_, x) in table.items():
        if not name.startswith("special_"):
            continue
        n = x.size
        for where, p in (("first", 0), ("last", n - 1), ("before", c - 1), ("after", c)):
            if p < n and n > 1:
                kind = "nan" if np.isnan(x[p]) else "pinf" if x[p] == np.inf else "ninf"
                assert not np.isfinite(x[p])
                seen.add((kind, where))
    assert len(seen) == 12
    big = table[f"plain/n{2 * c + 7}/o0"][1]
    assert np.abs(big).max() > 1e18 and np.abs(big).min() < 1e-19
    with np.errstate(over="ignore", under="ignore"):
        sq32 = big * big
        total32 = sq32.sum(dtype=np.float32)
    # fp32: the sum overflows, and the smallest squares fall below the normal range (bits lost)
    assert np.isinf(total32) and (sq32 < np.finfo(np.float32).tiny).any()
    assert np.isfinite(H.stats64(big)["sumsq"])
    s = H.stats64(table["subnormal_max/n1025/o3"][1])
    assert 0 < s["max"] < np.finfo(np.float32).tiny
    s = H.stats64(table["negzero_max/n257/o1"][1])
    assert s["max"] == 0.0 and s["min"] < 0
    buf, spans = H.layout(table)
    for name, (off, x) in table.items():
        start, n = spans[name]
        assert start % 4 == off and H.same_bits(buf[start:start + n], x)
        assert (buf[start - 4:start] == H.SENTINEL).all() and (buf[start + n:start + n + 4]
                                                                == H.SENTINEL).all()


def test_sumsq_bound_holds_for_sequential_and_pairwise_sums(L):
    """Any fp64 summation order is within n 2^-53 of the exact sum: numpy's sequential
    (cumsum) and pairwise (sum) orders on the designed vectors, and the bound is not vacuous --
    the fp32 sum of fp32 squares misses it."""
    worst = 0.0
    missed32 = 0
    for name, (_, x) in H.designs(L.STATS_CHUNK).items():
        want = H.stats64(x)
        d = x[np.isfinite(x)].astype(np.float64)
        sq = d * d
        for got in (float(np.cumsum(sq)[-1]) if sq.size else 0.0, float(np.sum(sq))):
            assert abs(got - want["sumsq"]) <= H.sumsq_bound(want), name
            if want["sumsq"]:
                worst = max(worst, abs(got - want["sumsq"]) / H.sumsq_bound(want))
        with np.errstate(over="ignore", under="ignore"):
            f = x[np.isfinite(x)]
            got32 = float(np.sum(f * f, dtype=np.float32))
        missed32 += not abs(got32 - want["sumsq"]) <= H.sumsq_bound(want)
    assert worst <= 1.0 and missed32 > 100


def test_reference_arithmetic_restated():
    w = OrderedDict(a=np.array([-3.0, 2.0], np.float32), b=np.array([np.nan, 9.0], np.float32),
                    c=np.array([-7.0, -1.0], np.float32))
    assert H.check_weights_ref(w) == 2.0                            # b's amax is NaN: skipped
    assert H.check_weights_ref(OrderedDict(c=w["c"])) == 0          # starts from 0
    ref = H.CheckModelWeightRef(1, 2, 2.5)
    assert [e for e in range(7) if ref.due(e)] == [1, 3, 5]
    ref.on_epoch_end(0, w)
    assert (ref.max_weight, ref.min_weight, ref.checked) == (2.5, -2.5, [])
    ref.on_epoch_end(1, w)
    # a: max 2 <= 2.5, so the elif: min -3 < -2.5.  b: max 9 > 2.5 (NaN dropped).  c: min -7
    assert (ref.max_weight, ref.min_weight) == (9.0, -7.0)
    ref = H.CheckModelWeightRef(0, 1, 1.0)
    ref.on_epoch_end(0, OrderedDict(a=np.array([5.0, -5.0], np.float32)))
    assert (ref.max_weight, ref.min_weight) == (5.0, -1.0)          # elif: the minimum waits


# ------------------------------------------------------------------ the C ABI
NEW = ("vtd_stats_plan_bytes", "vtd_stats_plan_upload", "vtd_tensor_stats")


def test_new_symbols_and_abi_version(L):
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert L.ABI_VERSION == 17 and L.lib.vtd_abi_version() == 17
    assert ctypes.sizeof(L.VtdTensorStat) == 48 and ctypes.sizeof(L.VtdStatsTensor) == 24
    assert [getattr(L.VtdTensorStat, f).offset for f in
            ("max", "min", "n", "nan", "pos_inf", "neg_inf", "sumsq")] == [0, 4, 8, 16, 24, 32, 40]


def table_of(L, entries):
    t = (L.VtdStatsTensor * len(entries))()
    for d, (x, out, n) in zip(t, entries):
        d.x, d.out, d.n = x, out, n
    return t


def sizes(L, entries):
    plan, ws, chunks = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    rc = L.lib.vtd_stats_plan_bytes(table_of(L, entries), len(entries), ctypes.byref(plan),
                                    ctypes.byref(ws), ctypes.byref(chunks))
    return rc, plan.value, ws.value, chunks.value


def refused(L, rc, text):
    assert rc == -1, rc
    assert text.encode() in L.lib.vtd_last_error(), L.lib.vtd_last_error()


def test_plan_sizes_of_a_known_table(L):
    c = L.STATS_CHUNK
    ns = [1, c - 1, c, c + 1, 5 * c + 3, 768 * 3072]
    rc, plan, ws, chunks = sizes(L, [(0x1000 * (i + 1), None, n) for i, n in enumerate(ns)])
    want = sum(-(-n // c) for n in ns)
    assert rc == 0 and chunks == want == 1 + 1 + 1 + 2 + 6 + 144
    assert ws == 32 * want
    assert plan == -(-len(ns) * 40 // 16) * 16 + 8 * want
    # the sizes do not depend on alignment or on `out`
    assert sizes(L, [(0x1004 * (i + 1), 0x70000 + 4 * i, n) for i, n in enumerate(ns)]) == \
        (0, plan, ws, chunks)


def test_plan_bytes_argument_checks(L):
    A = 0x10000                                                     # never dereferenced
    plan, ws, chunks = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
    one = table_of(L, [(A, None, 8)])
    f = L.lib.vtd_stats_plan_bytes
    refused(L, f(None, 1, ctypes.byref(plan), ctypes.byref(ws), ctypes.byref(chunks)),
            "null tensor table")
    for outs in ((None, ctypes.byref(ws), ctypes.byref(chunks)),
                 (ctypes.byref(plan), None, ctypes.byref(chunks)),
                 (ctypes.byref(plan), ctypes.byref(ws), None)):
        refused(L, f(one, 1, *outs), "null output")
    for n_tensors in (0, -3):
        refused(L, f(one, n_tensors, ctypes.byref(plan), ctypes.byref(ws), ctypes.byref(chunks)),
                "n_tensors must be positive")
    for entries, text in (([(A, None, 0)], "n must be positive"),
                          ([(A, None, -5)], "n must be positive"),
                          ([(None, None, 4)], "null x"),
                          ([(A + 2, None, 4)], "x needs a 4-B aligned base"),
                          ([(A + 1, None, 4)], "x needs a 4-B aligned base"),
                          ([(A, A + 0x1002, 4)], "out needs a 4-B aligned base"),
                          ([(A, None, 4), (A, None, 1 << 62)], "too many chunks"),
                          ([(A, None, (1 << 31) * L.STATS_CHUNK)], "too many chunks")):
        refused(L, sizes(L, entries)[0], text)
    # the most an int holds is accepted
    assert sizes(L, [(A, None, ((1 << 31) - 1) * L.STATS_CHUNK)])[3] == (1 << 31) - 1
    # a 4-B aligned base works: a torch view can start anywhere
    assert sizes(L, [(A + 4, A + 0x100c, 7)])[0] == 0


def test_plan_upload_and_launch_argument_checks(L):
    A, P = 0x10000, 0x200000
    one = table_of(L, [(A, None, 8)])
    rc, need, ws, chunks = sizes(L, [(A, None, 8)])
    assert rc == 0 and chunks == 1
    up = L.lib.vtd_stats_plan_upload
    refused(L, up(None, 1, P, need, None), "null tensor table")
    refused(L, up(one, 0, P, need, None), "n_tensors must be positive")
    refused(L, up(table_of(L, [(A + 2, None, 8)]), 1, P, need, None), "4-B aligned")
    refused(L, up(one, 1, None, need, None), "null plan_dev")
    refused(L, up(one, 1, P + 8, need, None), "16-B aligned")
    refused(L, up(one, 1, P, need - 1, None), "plan_bytes too small")
    run = L.lib.vtd_tensor_stats
    W, S = 0x300000, 0x400000
    refused(L, run(None, 1, 1, W, ws, S, 0.0, None), "null plan_dev")
    refused(L, run(P + 4, 1, 1, W, ws, S, 0.0, None), "16-B aligned")
    refused(L, run(P, 0, 1, W, ws, S, 0.0, None), "non-positive")
    refused(L, run(P, 1, 0, W, ws, S, 0.0, None), "non-positive")
    refused(L, run(P, 1, 1, None, ws, S, 0.0, None), "null workspace")
    refused(L, run(P, 1, 1, W, ws, None, 0.0, None), "null stats_dev")
    refused(L, run(P, 1, 1, W + 4, ws, S, 0.0, None), "8-B aligned")
    refused(L, run(P, 1, 1, W, ws, S + 4, 0.0, None), "8-B aligned")
    refused(L, run(P, 1, 1, W, ws - 1, S, 0.0, None), "workspace_bytes too small")
    refused(L, run(P, 1, 3, W, 2 * ws, S, 0.0, None), "workspace_bytes too small")


# ------------------------------------------------------------------ the Python surface
def test_python_surface(vtd):
    for name in ("health", "tensor_stats", "TensorStat", "check_weights", "check_inf_nan",
                 "CheckModelWeight"):
        assert name in vtd.__all__ and hasattr(vtd, name)
    sig = inspect.signature
    assert list(sig(vtd.tensor_stats).parameters) == ["tensors"]
    assert list(sig(vtd.check_weights).parameters) == ["model_input"]
    p = sig(vtd.check_inf_nan).parameters
    assert list(p) == ["inputs", "name", "max_value", "replace_nan"]
    assert p["max_value"].default == 50000 and p["replace_nan"].default is None
    p = sig(vtd.CheckModelWeight).parameters
    assert list(p) == ["start_epochs", "skip_epochs", "weight_threshold", "stop_on_nan"]
    assert p["stop_on_nan"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["stop_on_nan"].default is False
    assert list(sig(vtd.Model.weight_stats).parameters) == ["self"]
    for m in ("gradient_stats", "moment_stats", "global_norm"):
        p = sig(getattr(vtd.optimizers.Adam, m)).parameters
        assert list(p) == ["self", "model", "scope"] and p["scope"].default is None
    for m in ("fit", "fit_head"):
        assert sig(getattr(vtd.Model, m)).parameters["callbacks"].default is None
    # the norm-clipping arguments still raise: the statistics report, they do not clip
    for kw in ("clipnorm", "global_clipnorm"):
        with pytest.raises(ValueError, match=kw):
            vtd.optimizers.Adam(**{kw: 1.0})


def test_tensor_stat_norm_rule(vtd):
    S = vtd.TensorStat
    assert S(3.0, -4.0, 2, 0, 0, 0, 25.0).norm == 5.0
    assert math.isnan(S(3.0, -4.0, 3, 1, 1, 0, 25.0).norm)
    assert S(math.inf, -4.0, 3, 0, 1, 0, 16.0).norm == math.inf
    assert S(3.0, -math.inf, 3, 0, 0, 1, 9.0).norm == math.inf
    assert S(3.0, -4.0, 2, 0, 0, 0, 25.0).finite and not S(3.0, 0.0, 2, 0, 0, 1, 9.0).finite
    g = vtd.health.global_norm
    assert g([S(3.0, 3.0, 1, 0, 0, 0, 9.0), S(4.0, 4.0, 1, 0, 0, 0, 16.0)]) == 5.0
    assert math.isnan(g(dict(a=S(3.0, 3.0, 1, 0, 0, 0, 9.0), b=S(0.0, 0.0, 1, 1, 0, 0, 0.0))))
    assert g([S(3.0, 3.0, 1, 0, 0, 0, 9.0), S(math.inf, 0.0, 2, 0, 1, 0, 0.0)]) == math.inf


def test_host_inputs_are_refused_or_passed_through(vtd):
    import torch
    assert vtd.check_inf_nan(3, 'a') == 3
    v = 2.5
    assert vtd.check_inf_nan(v, 'a', replace_nan=0.0) is v
    for bad in (torch.zeros(4), np.zeros(4, np.float32), 3.0, None):
        with pytest.raises(ValueError):
            vtd.tensor_stats(bad)
    with pytest.raises(ValueError):
        vtd.tensor_stats([torch.zeros(4)])
    with pytest.raises(ValueError):
        vtd.tensor_stats({"a": torch.zeros(4, dtype=torch.float64)})


# ------------------------------------------------------------------ CheckModelWeight, stubbed
class StubModel:
    """weight_stats from host arrays through the oracle: what the device call returns."""

    def __init__(self, vtd, per_epoch):
        self.vtd, self.per_epoch, self.epoch, self.calls = vtd, per_epoch, 0, 0
        self.stop_training = False
        self.weight_shapes = OrderedDict((n, w.shape) for n, w in per_epoch[0].items())

    def weight_stats(self):
        self.calls += 1
        out = OrderedDict()
        for n, w in self.per_epoch[self.epoch].items():
            s = H.stats64(w)
            out[n] = self.vtd.TensorStat(float(s["max"]), float(s["min"]), s["n"], s["nan"],
                                         s["pos_inf"], s["neg_inf"], s["sumsq"])
        return out


def epochs_of_weights(rng, epochs, nan_at=None):
    out = []
    for e in range(epochs):
        w = OrderedDict((f"w{i}", (rng.standard_normal((3, 5)) * (1 + e) * (i + 1))
                         .astype(np.float32)) for i in range(4))
        if nan_at is not None and e >= nan_at:
            w["w2"][1, 2] = np.nan
        out.append(w)
    return out


@pytest.mark.parametrize("start,skip,threshold", [(0, 1, 0.0), (1, 1, 0.0), (2, 3, 4.0),
                                                  (1, 2, 100.0)])
def test_check_model_weight_bookkeeping_matches_the_reference(vtd, capsys, start, skip, threshold):
    per_epoch = epochs_of_weights(np.random.default_rng(start * 10 + skip), 9, nan_at=4)
    model = StubModel(vtd, per_epoch)
    cb = vtd.CheckModelWeight(start, skip, threshold)
    cb.set_model(model)
    ref = H.CheckModelWeightRef(start, skip, threshold)
    assert (cb.max_weight, cb.min_weight) == (threshold, -threshold)
    for e in range(9):
        model.epoch = e
        cb.on_epoch_end(e, {"loss": 1.0})
        ref.on_epoch_end(e, per_epoch[e])
        assert (cb.max_weight, cb.min_weight) == (ref.max_weight, ref.min_weight), e
    assert model.calls == len(ref.checked) == len([e for e in range(9) if ref.due(e)])
    assert model.stop_training is False                            # stop_on_nan is off
    text = capsys.readouterr().out
    if threshold < 100:
        assert "Largest_weight changed to: " in text and "Layer name:, w" in text
    else:
        assert "Largest_weight" not in text and "Smallest_weight" not in text
    if any(ref.due(e) for e in range(4, 9)):
        assert "NaN! Found in weight, its shape:  (3, 5)" in text


def test_check_model_weight_stop_on_nan(vtd, capsys):
    per_epoch = epochs_of_weights(np.random.default_rng(5), 6, nan_at=3)
    per_epoch[5]["w0"][0, 0] = -np.inf
    model = StubModel(vtd, per_epoch)
    cb = vtd.CheckModelWeight(0, 1, 0.0, stop_on_nan=True)
    cb.set_model(model)
    for e in range(3):
        model.epoch = e
        cb.on_epoch_end(e)
        assert model.stop_training is False
    model.epoch = 3
    cb.on_epoch_end(3)
    assert model.stop_training is True
    assert "w2: 1 NaN, 0 +Inf, 0 -Inf of 15" in capsys.readouterr().out
    model.stop_training, model.epoch = False, 5
    cb.on_epoch_end(5)
    assert model.stop_training is True
    text = capsys.readouterr().out
    assert "w0: 0 NaN, 0 +Inf, 1 -Inf of 15" in text and "Inf! Found in weight" in text
