"""The training side of the notebook's compile / fit for the detection head (ipynb cell
defc2073): keras.optimizers.Adam with `clipvalue`, the ClipWeight constraint (vtd.py:209-236)
and the step schedule `learning_rate_step_decay` (vtd.py:696-728).

The update itself is one launch of vtd_train_step per training step (csrc/vtd_optimizer.hip):
Adam, the constraint and the re-pack of the forward's operands, over a table of tensors that is
uploaded once -- the head's (Model.train_head_on_batch / fit_head, scope "head") or every
weight's (Model.train_on_batch / fit, scope "all").  Its entries carry the grouping, destination
format, constraint flag and update rule of each tensor; where the table holds layers whose
LayerNorm is folded into the next GEMM's operands, one launch of vtd_fold_layernorm_batch
follows.  There is no host arithmetic on the weights.
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

    _METHODS = {"head": "train_head_on_batch / fit_head", "all": "train_on_batch / fit"}

    def _state_for(self, model, scope=None):
        """The state of `model` in `scope`: "head" (the detection head on a frozen encoder) or
        "all" (every weight); None keeps the scope of the state there is, "head" if none."""
        st = self._state
        fresh = st is None or st.model() is not model or st.master_of is not model._master
        if scope is None:
            scope = "head" if fresh else st.scope
        if scope not in self._METHODS:
            raise ValueError(f"Adam: scope must be 'head' or 'all', got {scope!r}")
        if not fresh and st.scope != scope:
            if self.iterations > 0:
                raise ValueError(
                    f"Adam: this optimizer has taken {self.iterations} step(s) with "
                    f"{self._METHODS[st.scope]} (scope {st.scope!r}); its moments do not carry "
                    f"over to {self._METHODS[scope]}: compile a new optimizer to switch")
            fresh = True
        if fresh:
            self.iterations = 0
            st = self._state = _State(model, scope)
        return st

    def gradient_buffers(self, model, scope=None):
        """The persistent fp32 gradient buffers of `model`, keyed by Keras weight name: what the
        next `apply` reads -- the head's tensors or, in scope "all", every tensor of
        `weight_names()`."""
        return self._state_for(model, scope).grads

    def moments(self, model, scope=None):
        """(m, v) as dicts of the live fp32 device tensors, keyed by Keras weight name, over
        whatever the scope covers."""
        st = self._state_for(model, scope)
        return st.m, st.v

    # ---- numerical health of the optimizer's buffers (vtd_tensor_stats; health.py)
    def _health(self, model, scope, which):
        """The records of the state's gradient buffers ("g") or moments ("mv"): the uploaded
        plan is kept on the state, which is rebuilt whenever its tensors are."""
        from . import health as _health
        st = self._state_for(model, scope)
        plans = st.__dict__.setdefault("health_plans", {})
        if which not in plans:
            tensors = (list(st.grads.values()) if which == "g"
                       else list(st.m.values()) + list(st.v.values()))
            plans[which] = _health._Plan(tensors, what="Adam health")
        return st, plans[which].run()

    def gradient_stats(self, model, scope=None):
        """health.TensorStat per gradient buffer, an OrderedDict keyed like `gradient_buffers`:
        the gradients the last training call wrote (zeros before the first), NaN / Inf counts,
        max / min, sum of squares and norm, from one launch pair and one host read."""
        st, rec = self._health(model, scope, "g")
        return OrderedDict(zip(st.grads, rec))

    def moment_stats(self, model, scope=None):
        """(m, v) as OrderedDicts of health.TensorStat keyed like `moments`: one launch pair
        over both and one host read."""
        st, rec = self._health(model, scope, "mv")
        return (OrderedDict(zip(st.m, rec[:len(st.m)])), OrderedDict(zip(st.v, rec[len(st.m):])))

    def global_norm(self, model, scope=None):
        """sqrt(sum of squares over every gradient buffer), a float: what tf.linalg.global_norm
        gives for the last step's gradients -- nan if any holds a NaN, else inf if any holds an
        infinity.  Reporting only: the step does not clip by it (`clipnorm` and
        `global_clipnorm` raise)."""
        from . import health as _health
        return _health.global_norm(self.gradient_stats(model, scope))

    def apply(self, model, stream=None, scope=None):
        """One step on `model` from the gradient buffers: a single vtd_train_step launch that
        updates the device masters, moments and packed operands of the scope's tensors (the
        head's, or every weight's) and, where the scope holds tensors packed with the LayerNorm
        fold (never the head), one vtd_fold_layernorm_batch launch that refreshes the folded
        operands from the staging the step wrote."""
        st = self._state_for(model, scope)
        constrain = bool(model.kwargs.get("clip_weight", True))
        max_weight = float(model.kwargs.get("max_weight", 10) or 0.0)
        if constrain and not max_weight > 0.0:
            raise ValueError(f"Adam: clip_weight needs a positive max_weight, got "
                             f"{model.kwargs.get('max_weight')!r}")
        with torch.cuda.device(model.device):
            L.check(L.lib.vtd_train_step(
                st.plan.data_ptr(), st.n, st.tiles, self.iterations + 1,
                float(self.learning_rate), self.beta_1, self.beta_2, self.epsilon,
                self.clipvalue or 0.0, int(constrain), max_weight if constrain else 0.0,
                L.stream_ptr(stream)), "vtd_train_step")
            if st.fold_jobs:
                L.check(L.lib.vtd_fold_layernorm_batch(st.fold_plan.data_ptr(), st.fold_jobs,
                                                       st.fold_rows, L.BF16,
                                                       L.stream_ptr(stream)),
                        "vtd_fold_layernorm_batch")
        self.iterations += 1
        model._head_dirty = True
        if st.scope == "all":
            model._enc_dirty = True


class _State:
    """m, v, the gradient buffers and the uploaded vtd_train_step table for one model: over its
    head (scope "head": `head_weight_names()`, the device masters of `_head_master()` alone) or
    over every weight (scope "all": `weight_names()`, `_encoder_master()` + `_head_master()`, the
    masters `gradients` reads).  Per tensor the destination is what `Model._pack` recorded in
    `_train_packed` -- the packed operand in the mode's format with vtd_pack_dense's /
    vtd_pack_vector's grouping, or for a layer whose LayerNorm is folded a persistent fp32
    staging operand [N_p][K_p] (allocated here, not at model construction) that the fold job
    reads after the step.  The staging and the fold job table exist only where the scope's
    tensors include folded ones: never for the head."""

    def __init__(self, model, scope="head"):
        if model.dtype not in (L.BF16X3, L.BF16):
            raise ValueError("Adam: the model trains in the 'bf16x3' and 'bfloat16' modes only "
                             "(not float32 / float8)")
        self.model = weakref.ref(model)
        self.master_of = model._master
        self.scope = scope
        self.fold_jobs = 0
        w = OrderedDict(model._encoder_master()) if scope == "all" else OrderedDict()
        w.update(model._head_master())
        assert list(w) == (model.weight_names() if scope == "all" else model.head_weight_names())
        where = {n: model._train_packed[n] for n in w}
        folds = model._fold_jobs if any(p["fold"] is not None for p in where.values()) else []
        with torch.cuda.device(model.device):
            self.m = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            self.v = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            self.grads = OrderedDict((n, torch.zeros_like(t)) for n, t in w.items())
            self.staging = [torch.zeros(j["shape"], dtype=torch.float32, device=model.device)
                            for j in folds]
            table = (L.VtdTrainTensor * len(w))()
            for d, (n, t) in zip(table, w.items()):
                at = where[n]
                d.w, d.m, d.v, d.g = (t.data_ptr(), self.m[n].data_ptr(), self.v[n].data_ptr(),
                                      self.grads[n].data_ptr())
                folded = at["fold"] is not None
                packed = self.staging[at["fold"]] if folded else at["t"]
                d.packed = packed.data_ptr()
                d.packed_dtype = L.TRAIN_PACK_F32 if folded else L.TRAIN_PACK_MODE
                d.row_offset = at["off"]
                d.constrain, d.rule = 1, L.TRAIN_RULE_DENSE
                if n.endswith("/embeddings"):
                    # the position embedding (tokens, 1): Keras's sparse Adam path, and the
                    # reference leaves it without the ClipWeight constraint
                    d.kind, d.K, d.N, d.ld = L.ADAM_VECTOR, 1, t.numel(), 0
                    d.constrain, d.rule = 0, L.TRAIN_RULE_SPARSE
                elif n.endswith("/kernel"):
                    # EinsumDense kernels: (D, H, dk) is [D][H dk], grouped along N;
                    # attention_output (H, dk, D) is [H dk][D], grouped along K
                    w2 = (t.reshape(-1, t.shape[-1]) if t.dim() == 3 and at["kg"] is not None
                          else t.reshape(t.shape[0], -1))
                    d.kind, d.K, d.N, d.ld = L.ADAM_MATRIX, w2.shape[0], w2.shape[1], packed.shape[1]
                    kp = d.ld // 3 if model.dtype == L.BF16X3 and not folded else d.ld
                    d.k_group, d.k_group_p = at["kg"] or d.K, at["kgp"] or kp
                else:
                    d.kind, d.K, d.N, d.ld = L.ADAM_VECTOR, 1, t.numel(), 0
                d.n_group, d.n_group_p = at["ng"] or d.N, at["ngp"] or d.N
            need, tiles = ctypes.c_size_t(), ctypes.c_int()
            L.check(L.lib.vtd_train_plan_bytes(table, len(w), model.dtype, ctypes.byref(need),
                                               ctypes.byref(tiles)), "vtd_train_plan_bytes")
            self.plan = torch.empty(need.value, dtype=torch.uint8, device=model.device)
            L.check(L.lib.vtd_train_plan_upload(table, len(w), model.dtype, self.plan.data_ptr(),
                                                need.value, L.stream_ptr()),
                    "vtd_train_plan_upload")
            if folds:
                jobs = (L.VtdFoldJob * len(folds))()
                for j, job, w32 in zip(jobs, folds, self.staging):
                    n_p, k_p = job["shape"]
                    j.w32, j.gamma, j.beta = (w32.data_ptr(), job["gamma"].data_ptr(),
                                              job["beta"].data_ptr())
                    j.bias_in, j.w_out = job["bias_in"].data_ptr(), job["wo"].data_ptr()
                    j.bias_out, j.colsum = job["bo"].data_ptr(), job["cs"].data_ptr()
                    j.N, j.K, j.ldw, j.ldo = n_p, k_p, k_p, k_p
                self.fold_plan = torch.empty(ctypes.sizeof(jobs), dtype=torch.uint8,
                                             device=model.device)
                rows = ctypes.c_int()
                L.check(L.lib.vtd_fold_plan_upload(jobs, len(jobs), L.BF16,
                                                   self.fold_plan.data_ptr(), ctypes.sizeof(jobs),
                                                   ctypes.byref(rows), L.stream_ptr()),
                        "vtd_fold_plan_upload")
                self.fold_jobs, self.fold_rows = len(jobs), int(rows.value)
        self.n, self.tiles = len(w), int(tiles.value)


def resolve(optimizer):
    """compile()'s optimizer argument -> an optimizer that can train the model, or raise."""
    if isinstance(optimizer, str) and optimizer.lower() == "adam":
        return Adam()
    if isinstance(optimizer, Adam):
        return optimizer
    if optimizer is None:
        raise ValueError("no optimizer: call compile(optimizer=optimizers.Adam(...) or 'adam', "
                         "loss=...) first")
    raise ValueError(f"unsupported optimizer {optimizer!r}: use optimizers.Adam or 'adam'")


class History:
    """What fit and fit_head return: `.history["loss"]` holds one float per epoch, `.epoch` the
    epoch numbers (keras.callbacks.History)."""

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
