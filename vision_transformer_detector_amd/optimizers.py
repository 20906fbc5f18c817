"""The training side of the notebook's compile / fit for the detection head (ipynb cell
defc2073): keras.optimizers.Adam with `clipvalue`, the ClipWeight constraint (vtd.py:209-236)
and the step schedule `learning_rate_step_decay` (vtd.py:696-728).

The update itself is one launch of vtd_adam_step per training step (csrc/vtd_optimizer.hip):
Adam, the constraint and the re-pack of the forward's head operands, over a table of the
head's tensors that is uploaded once.  There is no host arithmetic on the weights.
"""
from __future__ import annotations

import ctypes
import weakref
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L


class Adam:
    """keras.optimizers.Adam(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
    clipvalue=None): Keras's argument names and defaults.  `learning_rate` is a writable
    attribute, `iterations` counts the steps taken.  Per element, in fp32 (TF's ApplyAdam):
    g = clip(g, +-clipvalue); m += (g - m)(1 - beta_1); v += (g^2 - v)(1 - beta_2);
    w -= m alpha / (sqrt(v) + epsilon), alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) formed in
    double.  `amsgrad`, `clipnorm` and `global_clipnorm` are not implemented and raise."""

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
                 amsgrad=False, clipvalue=None, clipnorm=None, global_clipnorm=None,
                 name="Adam"):
        if amsgrad:
            raise ValueError("Adam: amsgrad=True is not supported")
        if clipnorm is not None:
            raise ValueError("Adam: clipnorm is not supported (clipvalue is)")
        if global_clipnorm is not None:
            raise ValueError("Adam: global_clipnorm is not supported (clipvalue is)")
        if clipvalue is not None and not float(clipvalue) > 0.0:
            raise ValueError(f"Adam: clipvalue must be positive, got {clipvalue}")
        for arg, val in (("beta_1", beta_1), ("beta_2", beta_2)):
            if not 0.0 <= float(val) < 1.0:
                raise ValueError(f"Adam: {arg} must be in [0, 1), got {val}")
        if float(epsilon) < 0.0:
            raise ValueError(f"Adam: epsilon must be >= 0, got {epsilon}")
        self.learning_rate = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.clipvalue = None if clipvalue is None else float(clipvalue)
        self.name = name
        self.iterations = 0
        self._state = None             # per-model device state (_State), built on first use

    lr = property(lambda self: self.learning_rate,
                  lambda self, value: setattr(self, "learning_rate", float(value)))

    # ---- per-model state
    def _reset(self, model=None):
        """Forget the moments and the step count (Model.set_weights calls this: the table
        points at the device masters it has just replaced)."""
        if model is None or self._state is None or self._state.model() is model:
            self._state = None
            self.iterations = 0

    def _state_for(self, model):
        st = self._state
        if st is None or st.model() is not model or st.master_of is not model._master:
            self.iterations = 0
            st = self._state = _State(model)
        return st

    def gradient_buffers(self, model):
        """The persistent fp32 gradient buffers of `model`'s head, keyed by Keras weight name:
        what the next `apply` reads."""
        return self._state_for(model).grads

    def moments(self, model):
        """(m, v) as dicts of the live fp32 device tensors, keyed by Keras weight name."""
        st = self._state_for(model)
        return st.m, st.v

    def apply(self, model, stream=None):
        """One step on `model`'s head from the gradient buffers: a single vtd_adam_step launch
        that updates the device masters, the moments and the forward's packed operands."""
        st = self._state_for(model)
        constrain = bool(model.kwargs.get("clip_weight", True))
        max_weight = float(model.kwargs.get("max_weight", 10) or 0.0)
        if constrain and not max_weight > 0.0:
            raise ValueError(f"Adam: clip_weight needs a positive max_weight, got "
                             f"{model.kwargs.get('max_weight')!r}")
        with torch.cuda.device(model.device):
            L.check(L.lib.vtd_adam_step(st.plan.data_ptr(), st.n, st.tiles, self.iterations + 1,
                                        float(self.learning_rate), self.beta_1, self.beta_2,
                                        self.epsilon, self.clipvalue or 0.0, int(constrain),
                                        max_weight if constrain else 0.0,
                                        L.stream_ptr(stream)), "vtd_adam_step")
        self.iterations += 1
        model._head_dirty = True


class _State:
    """m, v, the gradient buffers and the uploaded table for one model's head."""

    def __init__(self, model):
        if model.dtype not in (L.BF16X3, L.BF16):
            raise ValueError("Adam: the head trains in the 'bf16x3' and 'bfloat16' modes only "
                             "(not float32 / float8)")
        self.model = weakref.ref(model)
        self.master_of = model._master
        w = model._head_master()
        with torch.cuda.device(model.device):
            self.m = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            self.v = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            self.grads = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            table = (L.VtdAdamTensor * len(w))()
            for d, (n, t) in zip(table, w.items()):
                packed = model._head_packed[n]
                d.w, d.m, d.v, d.g = (t.data_ptr(), self.m[n].data_ptr(), self.v[n].data_ptr(),
                                      self.grads[n].data_ptr())
                d.packed = packed.data_ptr()
                if t.dim() == 2:
                    d.kind, d.K, d.N, d.ld = L.ADAM_MATRIX, t.shape[0], t.shape[1], packed.shape[1]
                else:
                    d.kind, d.K, d.N, d.ld = L.ADAM_VECTOR, 1, t.numel(), 0
            need, tiles = ctypes.c_size_t(), ctypes.c_int()
            L.check(L.lib.vtd_adam_plan_bytes(table, len(w), model.dtype, ctypes.byref(need),
                                              ctypes.byref(tiles)), "vtd_adam_plan_bytes")
            self.plan = torch.empty(need.value, dtype=torch.uint8, device=model.device)
            L.check(L.lib.vtd_adam_plan_upload(table, len(w), model.dtype, self.plan.data_ptr(),
                                               need.value, L.stream_ptr()), "vtd_adam_plan_upload")
        self.n, self.tiles = len(w), int(tiles.value)


def resolve(optimizer):
    """compile()'s optimizer argument -> an optimizer that can train the head, or raise."""
    if isinstance(optimizer, str) and optimizer.lower() == "adam":
        return Adam()
    if isinstance(optimizer, Adam):
        return optimizer
    if optimizer is None:
        raise ValueError("no optimizer: call compile(optimizer=optimizers.Adam(...) or 'adam', "
                         "loss=...) first")
    raise ValueError(f"unsupported optimizer {optimizer!r}: use optimizers.Adam or 'adam'")


class History:
    """What fit_head returns: `.history["loss"]` holds one float per epoch, `.epoch` the epoch
    numbers (keras.callbacks.History)."""

    def __init__(self):
        self.history = {"loss": []}
        self.epoch = []


# ------------------------------------------------------------------ the step schedule
class _Counter:
    """The remaining learning-rate decays (the reference keeps a tf.Variable, vtd.py:693, and
    the notebook sets it with `.assign(n)`)."""

    def __init__(self, value=3):
        self.value = int(value)

    def assign(self, value):
        self.value = int(value)
        return self

    def assign_sub(self, value=1):
        self.value -= int(value)
        return self

    def numpy(self):
        return np.int32(self.value)

    def __int__(self):
        return self.value

    def __repr__(self):
        return f"<allowed decay times: {self.value}>"


_allowed_decay_times = _Counter(3)


def learning_rate_step_decay(epoch, lr, epochs_first_lr_decay, epochs_second_lr_decay,
                             epochs_third_lr_decay, rate_lr_decay):
    """The reference's step schedule (vtd.py:696-728): at epoch == first, first + second and
    first + second + third the rate is multiplied by `rate_lr_decay`, while the module counter
    `_allowed_decay_times` (3 by default; the notebook assigns it) is positive; each decay
    takes one off it.  Used as `lr_schedule=functools.partial(learning_rate_step_decay,
    epochs_first_lr_decay=..., ...)`."""
    first = epochs_first_lr_decay
    second = first + epochs_second_lr_decay
    third = second + epochs_third_lr_decay
    if epoch in (first, second, third) and _allowed_decay_times.value > 0:
        lr *= rate_lr_decay
        _allowed_decay_times.assign_sub(1)
    return lr
