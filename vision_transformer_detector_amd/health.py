"""Numerical health of tensors on the device: the reference's training diagnostics
`check_inf_nan` (vtd.py:46-116), `check_weights` (vtd.py:731-758) and the `CheckModelWeight`
callback (vtd.py:650-687) without moving a tensor to the host.

Everything here reads records of vtd_tensor_stats (csrc/vtd_health.hip; include/vtd.h "Numerical
health"): per tensor the NaN / +inf / -inf counts, the largest and smallest non-NaN value and the
fp64 sum of squares of the finite elements, from one pass over a table of fp32 device tensors --
one launch pair and one host read per call, however many tensors.  `Model.weight_stats()` runs it
over the device masters, `optimizers.Adam.gradient_stats / moment_stats / global_norm` over the
optimizer's buffers.  There is no host fallback: a tensor that is not fp32, contiguous and on the
device raises.
"""
from __future__ import annotations

import ctypes
import math
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L

_RECORD = np.dtype([("max", "<f4"), ("min", "<f4"), ("n", "<i8"), ("nan", "<i8"),
                    ("pos_inf", "<i8"), ("neg_inf", "<i8"), ("sumsq", "<f8")])
assert _RECORD.itemsize == ctypes.sizeof(L.VtdTensorStat) == 48


@dataclass(frozen=True)
class TensorStat:
    """One vtd_tensor_stat record.  `max` / `min` are over the elements that are not NaN
    (infinities included; -inf / +inf when there is none), `sumsq` is the fp64 sum of squares of
    the finite elements, `n` the element count."""
    max: float
    min: float
    n: int
    nan: int
    pos_inf: int
    neg_inf: int
    sumsq: float

    @property
    def norm(self) -> float:
        """The L2 norm as the tensor's own arithmetic would give it: nan if any element is NaN,
        else inf if any is infinite, else sqrt(sumsq)."""
        return _norm(self.sumsq, self.nan, self.pos_inf + self.neg_inf)

    @property
    def finite(self) -> bool:
        return self.nan == 0 and self.pos_inf == 0 and self.neg_inf == 0


def _norm(sumsq, nan, inf):
    if nan > 0:
        return float("nan")
    if inf > 0:
        return float("inf")
    return math.sqrt(sumsq)


def _check(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 \
            or not t.is_contiguous():
        kind = (f"{t.dtype} on {t.device}, contiguous={t.is_contiguous()}" if torch.is_tensor(t)
                else type(t).__name__)
        raise ValueError(f"{what}: needs a contiguous float32 device tensor, got {kind} (there "
                         "is no host path)")
    if t.numel() == 0:
        raise ValueError(f"{what}: an empty tensor has no statistics")
    return t


class _Plan:
    """The uploaded vtd_stats plan of a list of tensors with its workspace and record buffer:
    built once, run any number of times.  Holds the tensors, so the table's pointers stay valid."""

    def __init__(self, tensors, outs=None, what="tensor_stats"):
        self.tensors = [_check(t, what) for t in tensors]
        if not self.tensors:
            raise ValueError(f"{what}: no tensors")
        dev = self.tensors[0].device
        if any(t.device != dev for t in self.tensors):
            raise ValueError(f"{what}: the tensors must be on one device")
        self.outs = list(outs) if outs is not None else [None] * len(self.tensors)
        self.device, self.n = dev, len(self.tensors)
        table = (L.VtdStatsTensor * self.n)()
        for d, t, o in zip(table, self.tensors, self.outs):
            d.x, d.out, d.n = t.data_ptr(), L.ptr(o), t.numel()
        need, ws, chunks = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        L.check(L.lib.vtd_stats_plan_bytes(table, self.n, ctypes.byref(need), ctypes.byref(ws),
                                           ctypes.byref(chunks)), "vtd_stats_plan_bytes")
        with torch.cuda.device(dev):
            self.plan = torch.empty(need.value, dtype=torch.uint8, device=dev)
            self.workspace = torch.empty(ws.value, dtype=torch.uint8, device=dev)
            self.records = torch.empty(self.n * _RECORD.itemsize, dtype=torch.uint8, device=dev)
            L.check(L.lib.vtd_stats_plan_upload(table, self.n, self.plan.data_ptr(), need.value,
                                                L.stream_ptr()), "vtd_stats_plan_upload")
        self.chunks = int(chunks.value)

    def launch(self, replace_nan=0.0, stream=None):
        """The launch pair on the stream; nothing is read."""
        with torch.cuda.device(self.device):
            L.check(L.lib.vtd_tensor_stats(self.plan.data_ptr(), self.n, self.chunks,
                                           self.workspace.data_ptr(), self.workspace.numel(),
                                           self.records.data_ptr(), float(replace_nan),
                                           L.stream_ptr(stream)), "vtd_tensor_stats")

    def run(self, replace_nan=0.0):
        """The launch pair and the one host read: a list of TensorStat in table order."""
        self.launch(replace_nan)
        rec = self.records.cpu().numpy().view(_RECORD)
        return [TensorStat(float(r["max"]), float(r["min"]), int(r["n"]), int(r["nan"]),
                           int(r["pos_inf"]), int(r["neg_inf"]), float(r["sumsq"])) for r in rec]


def tensor_stats(tensors):
    """The statistics of one float32 device tensor (-> TensorStat), of a list or tuple of them
    (-> list) or of a dict (-> OrderedDict with the same keys): one launch pair and one host
    read.  Anything not float32, not contiguous or not on the device raises ValueError."""
    if torch.is_tensor(tensors):
        return _Plan([tensors]).run()[0]
    if isinstance(tensors, dict):
        return OrderedDict(zip(tensors, _Plan(list(tensors.values())).run()))
    if isinstance(tensors, (list, tuple)):
        return _Plan(list(tensors)).run()
    raise ValueError(f"tensor_stats: expected a tensor, a list or a dict, got "
                     f"{type(tensors).__name__}")


def global_norm(stats) -> float:
    """sqrt(sum of sumsq) over records (an iterable, or a dict's values): what
    tf.linalg.global_norm gives for the tensors, with TensorStat.norm's NaN / Inf rule."""
    stats = list(stats.values()) if isinstance(stats, dict) else list(stats)
    return _norm(math.fsum(s.sumsq for s in stats), sum(s.nan for s in stats),
                 sum(s.pos_inf + s.neg_inf for s in stats))


def _unhealthy(stats):
    """The lines naming the tensors of a dict of records that hold a NaN or an infinity."""
    return [f"{name}: {s.nan} NaN, {s.pos_inf} +Inf, {s.neg_inf} -Inf of {s.n}"
            for name, s in stats.items() if not s.finite]


# ------------------------------------------------------------------ check_weights
def check_weights(model_input):
    """The reference's check_weights (vtd.py:731-758) from one Model.weight_stats() call: the
    largest weight, with the reference's arithmetic -- it starts from 0 and takes a tensor's
    maximum only when `max_weight < np.amax(weight)` holds, so a tensor holding a NaN (whose amax
    is NaN) never moves it and the result is at least 0 -- its red line of 500 and its messages.
    Beyond the reference: the names of the tensors holding NaN or Inf are printed."""
    red_line_weight = 500
    max_weight = 0
    print('\nChecking the weights ...')
    stats = model_input.weight_stats()
    for s in stats.values():
        amax = float("nan") if s.nan else s.max
        if max_weight < amax:
            max_weight = amax
    bad = _unhealthy(stats)
    if bad:
        print('\nNaN or Inf found in the weights:\n' + '\n'.join(bad))
    if max_weight > red_line_weight:
        print(f'\nAlert! max_weight is: {max_weight:.1f}')
        print('\nVery high weight could lead to a big model output '
              'value, then cause the NaN loss. Please consider:\n'
              '1. use a smaller learning_rate;\n2. reduce the loss value.\n')
    else:
        print(f'\nThe status is OK, max_weight is: {max_weight:.1f}\n')
    return max_weight


# ------------------------------------------------------------------ check_inf_nan
def _report(stat, name, shape, max_value, replace_nan, changed=''):
    """check_inf_nan's messages for one tensor from its record; returns the new max_value."""
    if stat.pos_inf or stat.neg_inf:
        print(f'\nInf! Found {"found " if changed else ""}in {name}, its shape: ', tuple(shape))
    current_max = stat.max
    if stat.nan:
        print(f'\nNaN! Found in {name}, its shape: ', tuple(shape))
        # tf.math.reduce_max of a tensor that holds a NaN is NaN; of the replaced one, the
        # larger of the non-NaN maximum and the replacement
        current_max = float("nan") if replace_nan is None else max(stat.max, float(
            np.float32(replace_nan)))
    if current_max > max_value:
        max_value = current_max
        print(f'\nIn {name}, its shape: ', tuple(shape))
        print(f'max_value{changed}: ', max_value)
    return max_value


def _stage(x, what):
    """A float32 contiguous device tensor of a numpy array or CPU tensor (moved to the current
    device); a device tensor must already be one."""
    if torch.is_tensor(x) and x.is_cuda:
        return _check(x, what)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} runs on the HIP device and none is available")
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    dev = torch.device("cuda", torch.cuda.current_device())
    return _check(t.to(device=dev, dtype=torch.float32).contiguous(), what)


def check_inf_nan(inputs, name, max_value=50000, replace_nan=None):
    """The reference's check_inf_nan (vtd.py:46-116): report Inf, NaN and a maximum above
    `max_value` in `inputs`, with its messages, from one record (one launch pair, one host read).
    An int or float is returned unchanged.  A float32 device tensor -- or a numpy array / CPU
    tensor, which is moved to the device -- gets the three checks; with `replace_nan` and a NaN
    present the result is a NEW tensor with every NaN replaced (written by the same kernel pass;
    numpy in, numpy out), otherwise the input object itself is returned.  A tuple (the model's
    outputs) is walked as `name_0`, `name_1`, ... in one launch and returned as it came, as the
    reference does."""
    if type(inputs) is not tuple:
        if isinstance(inputs, (int, float)):
            return inputs
        x = _stage(inputs, "check_inf_nan")
        out = torch.empty_like(x) if replace_nan is not None else None
        stat, = _Plan([x], [out], what="check_inf_nan").run(
            0.0 if replace_nan is None else replace_nan)
        _report(stat, name, inputs.shape, max_value, replace_nan)
        if out is None or not stat.nan:
            return inputs
        if torch.is_tensor(inputs):
            return out if inputs.is_cuda else out.cpu()
        return out.cpu().numpy()
    items = [(f'{name}_{i}', each) for i, each in enumerate(inputs)
             if not isinstance(each, (int, float))]
    if items:
        stats = _Plan([_stage(each, "check_inf_nan") for _, each in items],
                      what="check_inf_nan").run()
        for (subname, each), stat in zip(items, stats):
            max_value = _report(stat, subname, each.shape, max_value, replace_nan, ' change to')
    return inputs


# ------------------------------------------------------------------ CheckModelWeight
class CheckModelWeight:
    """The reference's CheckModelWeight callback (vtd.py:650-687) for `fit` / `fit_head`
    `callbacks=`: after epoch `start_epochs` and then every `skip_epochs` epochs, one
    `model.weight_stats()` call; per weight in `weight_names()` order the check_inf_nan messages,
    then `max_weight` moves up to the weight's maximum if that is larger, ELSE `min_weight` down
    to its minimum if that is smaller (the reference's if / elif), both starting at
    +-`weight_threshold`.  The maximum and minimum are the record's: over the non-NaN elements.
    `stop_on_nan`: a check that finds a NaN or an infinity in any weight sets
    `model.stop_training = True`, which ends `fit` after that epoch."""

    def __init__(self, start_epochs, skip_epochs, weight_threshold, *, stop_on_nan=False):
        self.max_weight = weight_threshold
        self.min_weight = -weight_threshold
        self.start_epochs = start_epochs
        self.skip_epochs = skip_epochs
        self.stop_on_nan = bool(stop_on_nan)
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        if not ((epoch >= self.start_epochs) and
                ((epoch - self.start_epochs) % self.skip_epochs == 0)):
            return
        stats = self.model.weight_stats()
        shapes = self.model.weight_shapes
        for name, s in stats.items():
            shape = tuple(shapes[name])
            _report(s, 'weight', shape, 50000, None)
            if s.max > self.max_weight:
                self.max_weight = s.max
                print(f'\nLargest_weight changed to: '
                      f'{self.max_weight:.3f}, at epoch {epoch}.'
                      f'\tWeight shape: {shape}\t\t'
                      f'Layer name:, {name}')
            elif s.min < self.min_weight:
                self.min_weight = s.min
                print(f'\nSmallest_weight changed to: '
                      f'{self.min_weight:.3f}, at epoch {epoch}.'
                      f'\tWeight shape: {shape}\t\t'
                      f'Layer name:, {name}')
        if self.stop_on_nan:
            bad = _unhealthy(stats)
            if bad:
                print(f'\nNaN or Inf in the weights at epoch {epoch}; stopping:\n' +
                      '\n'.join(bad))
                self.model.stop_training = True
