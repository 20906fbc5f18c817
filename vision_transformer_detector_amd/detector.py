"""Host-side mirror of the reference model API, backed by libvtd.so.

Reference: /root/reference/vision_transformer_detector.py (cited vtd.py:N).
  create_vision_transformer_detector(...)   vtd.py:498-583  -> Model
  Model.__call__(images, training=False)    keras.Model call (vtd.py:331-335)
  Model.predict(images, batch_size=32)      keras.Model.predict (ipynb:836)
  Model.get_weights() / set_weights()       keras (vtd.py:2155-2157), Keras layer names
  transform_predictions(logits)             vtd.py:586-647
  Constants                                 vtd.py:19-43

Every compute call goes through the C-ABI (`_lib`); there is no CPU/torch fallback.
Caller-visible layout is the reference's: NHWC fp32 images in [-1, 1] in, (B, 17, 6)
fp32 pre-sigmoid logits out.
"""
from __future__ import annotations

import ctypes
import os
import math
from collections import OrderedDict
from enum import Enum

import numpy as np
import torch

from . import _lib as L


class Constants(Enum):                                   # vtd.py:19-43
    CLASSES = 80
    MODEL_IMAGE_SIZE = 608, 608
    EPSILON = 1e-8
    MAX_DETECT_OBJECTS_QUANTITY = 17
    LATEST_RELATED_IMAGES = 3
    BBOXES_PER_IMAGE = 14
    OBJECTNESS_THRESHOLD = 0.5
    CLASSIFICATION_CONFIDENCE_THRESHOLD = 0.5


_DTYPES = {"float32": L.F32, "fp32": L.F32, "f32": L.F32, "bfloat16": L.BF16,
           "bf16": L.BF16, "float8": L.FP8, "fp8": L.FP8, "mxfp8": L.FP8,
           "bfloat16x3": L.BF16X3, "bf16x3": L.BF16X3, "split_bf16": L.BF16X3}
# storage dtype of the activations and of the matrices outside the MX-fp8 layers (the
# split-bf16 mode stores its matrices as bf16 rows of three pieces, include/vtd.h)
_TORCH_DTYPE = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.FP8: torch.bfloat16,
                L.BF16X3: torch.bfloat16}


def _resolve_dtype(dtype) -> int:
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float32: "f32", torch.bfloat16: "bf16"}.get(dtype, str(dtype))
    try:
        return _DTYPES[str(dtype).lower()]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype!r}: use 'float32' (parity), 'bf16x3' "
                         "(split-bf16 parity mode), 'bfloat16' or 'float8' (MX-fp8 encoder "
                         "Dense layers)")


# ------------------------------------------------------------------------- names
def keras_weight_names(kw: dict, dims: L.VtdDims) -> "OrderedDict[str, tuple]":
    """Keras weight name -> shape of the graph vtd.py:498-583 builds (after
    keras.backend.clear_session(), vtd.py:548, layer names are deterministic)."""
    d, nh, dk = kw["embedding_dim"], kw["encoder_num_heads"], kw["encoder_key_dim"]
    out = OrderedDict()
    out["position_encoding/position_embedding/embeddings"] = (dims.tokens, 1)
    out["linear_projection/kernel"] = (dims.patch_dim, d)
    out["linear_projection/bias"] = (d,)
    q = kw["encoder_mlp_quantities"]
    for i in range(1, kw["encoder_repeat_times"] + 1):
        ln1 = "layer_normalization" if i == 1 else f"layer_normalization_{2 * i - 2}"
        ln2 = f"layer_normalization_{2 * i - 1}"
        mha = "multi_head_attention" if i == 1 else f"multi_head_attention_{i - 1}"
        out[f"{ln1}/gamma"] = (d,)
        out[f"{ln1}/beta"] = (d,)
        for part in ("query", "key", "value"):
            out[f"{mha}/{part}/kernel"] = (d, nh, dk)
            out[f"{mha}/{part}/bias"] = (nh, dk)
        out[f"{mha}/attention_output/kernel"] = (nh, dk, d)
        out[f"{mha}/attention_output/bias"] = (d,)
        out[f"{ln2}/gamma"] = (d,)
        out[f"{ln2}/beta"] = (d,)
        k = d
        for j in range(q):
            n = dims.mlp_units[j]
            out[f"MLP_{i}_{j + 1}/kernel"] = (k, n)
            out[f"MLP_{i}_{j + 1}/bias"] = (n,)
            k = n
    out["dense/kernel"] = (d, L.MAX_DETECT)
    out["dense/bias"] = (L.MAX_DETECT,)
    k = dims.tokens
    for j in range(dims.n_head):
        n = dims.head_units[j]
        out[f"dense_{j + 1}/kernel"] = (k, n)
        out[f"dense_{j + 1}/bias"] = (n,)
        k = n
    out["MLP_Head_no_Sigmoid/kernel"] = (k, 6)
    out["MLP_Head_no_Sigmoid/bias"] = (6,)
    return out


def _glorot_fans(shape):
    if len(shape) == 2:
        return shape[0], shape[1]
    rf = int(np.prod(shape[:-2]))
    return shape[-2] * rf, shape[-1] * rf


def keras_default_init(names: "OrderedDict[str, tuple]", seed: int = 0):
    """Keras defaults [upstream]: glorot_uniform kernels, zero biases, LN gamma=1 beta=0,
    Embedding U(-0.05, 0.05).  Returns fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    for name, shape in names.items():
        if name.endswith("/embeddings"):
            t = torch.rand(shape, generator=g) * 0.1 - 0.05
        elif name.endswith("/kernel"):
            fi, fo = _glorot_fans(shape)
            lim = math.sqrt(6.0 / (fi + fo))
            t = torch.rand(shape, generator=g) * (2 * lim) - lim
        elif name.endswith("/gamma"):
            t = torch.ones(shape)
        else:
            t = torch.zeros(shape)
        out[name] = t.float()
    return out


# ------------------------------------------------------------------------- model
class Model:
    """Inference model equivalent to the keras.Model `vision_transformer_detector`."""

    name = "vision_transformer_detector"

    def __init__(self, kwargs: dict, dtype="bf16x3", device=None, seed: int = 0):
        self.kwargs = dict(kwargs)
        self.dtype = _resolve_dtype(dtype)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise ValueError("Model runs on a HIP device only (device='cuda[:i]')")
        h, w, c = self.kwargs["input_shape"]
        self.input_shape = (int(h), int(w), int(c))
        self._cfg_template = dict(
            image_h=h, image_w=w, channels=c, patch_size=self.kwargs["patch_size"],
            embedding_dim=self.kwargs["embedding_dim"],
            num_heads=self.kwargs["encoder_num_heads"], key_dim=self.kwargs["encoder_key_dim"],
            mlp_quantities=self.kwargs["encoder_mlp_quantities"],
            repeat_times=self.kwargs["encoder_repeat_times"],
            head_last_units=self.kwargs["mlp_head_last_units"],
            head_layers=self.kwargs["mlp_head_dense_layers_quantity"],
            head_repeats=self.kwargs["mlp_head_dense_mish_block_repeats"],
            use_mish=1 if self.kwargs["use_mish"] else 0, dtype=self.dtype)
        self.dims = self._derive(1)
        self.weight_shapes = keras_weight_names(self.kwargs, self.dims)
        self._master = None            # fp32 CPU tensors keyed by Keras name
        self._packed = []              # keeps device buffers alive
        self._ws = None
        self._ws_bytes = 0
        self.loss = None               # compile(): the loss callable and the metric objects
        self.metrics = []
        self.optimizer = None          # compile(): stored as given, resolved by a training call
        self.dropout_seed = None       # compile(dropout_seed=): dropout in the training graph
        self.stop_training = False     # set by a callback: fit / fit_head end after that epoch
        self._head_dirty = False       # the head's device masters are ahead of self._master
        self._enc_dirty = False        # so are the encoder's and the stem's (train_on_batch)
        self.set_weights(keras_default_init(self.weight_shapes, seed))

    # ---- config helpers
    def config(self, batch: int) -> L.VtdConfig:
        return L.VtdConfig(batch=int(batch), **self._cfg_template)

    def _derive(self, batch: int) -> L.VtdDims:
        cfg, dims = self.config(batch), L.VtdDims()
        L.check(L.lib.vtd_derive_dims(ctypes.byref(cfg), ctypes.byref(dims)), "derive_dims")
        return dims

    def workspace_bytes(self, batch: int) -> int:
        cfg, n = self.config(batch), ctypes.c_size_t()
        L.check(L.lib.vtd_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)), "workspace")
        return int(n.value)

    # ---- weights
    def get_weights(self):
        """Weights as a list in Keras creation order (names: `weight_names()`)."""
        self._sync_master()
        return [self._master[n].numpy().copy() for n in self.weight_shapes]

    def weight_names(self):
        return list(self.weight_shapes)

    def _sync_master(self):
        """After optimizer steps the device masters are the truth -- the head's after head-only
        steps, every tensor's after all-weights steps: read back what is dirty into the fp32 CPU
        masters (once per run of steps)."""
        if self._enc_dirty:               # an all-weights step: the encoder and the stem too
            for n, t in self._encoder_master().items():
                self._master[n] = t.cpu()
            self._enc_dirty = False
        if self._head_dirty:
            for n, t in self._head_master().items():
                self._master[n] = t.cpu()
            self._head_dirty = False

    def get_weight_dict(self):
        self._sync_master()
        return OrderedDict((n, self._master[n].numpy().copy()) for n in self.weight_shapes)

    def set_weights(self, weights):
        """Accepts a dict keyed by Keras weight names or a list in `weight_names()` order."""
        if isinstance(weights, dict):
            missing = [n for n in self.weight_shapes if n not in weights]
            extra = [n for n in weights if n not in self.weight_shapes]
            if missing or extra:
                raise ValueError(f"set_weights: missing {missing[:5]} unexpected {extra[:5]}")
            items = [(n, weights[n]) for n in self.weight_shapes]
        else:
            weights = list(weights)
            if len(weights) != len(self.weight_shapes):
                raise ValueError(f"set_weights: expected {len(self.weight_shapes)} arrays, "
                                 f"got {len(weights)}")
            items = list(zip(self.weight_shapes, weights))
        master = OrderedDict()
        for n, v in items:
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).float().cpu()
            if tuple(t.shape) != tuple(self.weight_shapes[n]):
                raise ValueError(f"set_weights: {n} has shape {tuple(t.shape)}, expected "
                                 f"{self.weight_shapes[n]}")
            master[n] = t.contiguous()
        self._master = master
        self._head_dirty = self._enc_dirty = False
        self._pack()
        if hasattr(self.optimizer, "_reset"):       # its table points at the old device masters
            self.optimizer._reset(self)

    # ---- weight files (Keras-name keyed; see tools/keras_weights_to_npz.py)
    def save_weights(self, path: str) -> None:
        """Write the fp32 master weights keyed by Keras weight names to `.npz` or
        `.safetensors` (the interchange format of this package)."""
        self._sync_master()
        d = {n: t.numpy() for n, t in self._master.items()}
        if path.endswith(".safetensors"):
            from safetensors.numpy import save_file
            save_file(d, path)
        else:
            np.savez(path, **d)

    def load_weights(self, path: str) -> None:
        """Read weights from a Keras 2.x HDF5 file -- the reference's `model.save('*.keras')`
        (vtd.py:2146, 2179; HDF5 under TF 2.9) or `save_weights('*.h5')` -- by Keras weight
        name (keras_h5.read_keras_weights), or from files written by save_weights /
        tools/keras_weights_to_npz.py (names may carry TF's ':0' suffix).  Only loaders
        that execute nothing from the file are used (the HDF5 parser here, np.load
        allow_pickle=False, safetensors)."""
        if path.endswith((".keras", ".h5", ".hdf5")):
            from .keras_h5 import read_keras_weights
            raw, _ = read_keras_weights(path)
        elif path.endswith(".safetensors"):
            from safetensors.numpy import load_file
            raw = load_file(path)
        else:
            with np.load(path, allow_pickle=False) as z:
                raw = {k: z[k] for k in z.files}
        self.set_weights({k.split(":")[0]: v for k, v in raw.items()})

    def _pack(self):
        dims = self.dims
        fp8 = self.dtype == L.FP8
        x3 = self.dtype == L.BF16X3             # split-bf16: packed in f32, then split
        dt = L.BF16 if fp8 else self.dtype      # dtype of the non-MX matrices
        tdt = _TORCH_DTYPE[dt]
        dev = self.device
        keep, staging = [], []
        # Keras name -> where the forward's copy of that tensor lives (vtd_train_step re-packs
        # it): the packed tensor `t` and vtd_pack_dense's / vtd_pack_vector's grouping, or
        # `fold`: the index in `folds` of the LayerNorm fold job whose fp32 staging operand it
        # belongs to.  Not filled for the MX-fp8 layers (no training in that mode).  `rec` returns
        # the packed tensor's device pointer, for the forward's weight struct.
        train, folds = {}, []

        def rec(name, t=None, fold=None, kg=None, kgp=None, ng=None, ngp=None, off=0):
            train[name] = dict(t=t, fold=fold, kg=kg, kgp=kgp, ng=ng, ngp=ngp, off=off)
            return None if t is None else t.data_ptr()
        stream = L.stream_ptr(torch.cuda.current_stream(dev))

        def zeros(*shape, dtype=tdt):
            t = torch.zeros(shape, dtype=dtype, device=dev)
            keep.append(t)
            return t

        def src(name):
            t = self._master[name].to(dev).contiguous()
            staging.append(t)
            return t

        def split3(w32):
            """split-bf16 B operand [hi | hi | lo] of a packed fp32 matrix [rows_p][k_p]."""
            rows_p, k_p = w32.shape
            out = zeros(rows_p, 3 * k_p, dtype=torch.bfloat16)
            L.check(L.lib.vtd_split_bf16x3(w32.data_ptr(), rows_p, k_p, k_p, out.data_ptr(),
                                           3 * k_p, 1, stream), "split_bf16x3")
            return out

        def dense(name, rows_p, k_p, kg=None, kgp=None, ng=None, ngp=None, dst=None, off=0,
                  pdt=None):
            if x3 and dst is None and pdt is None:
                return split3(dense(name, rows_p, k_p, kg, kgp, ng, ngp,
                                    dst=f32_staging(rows_p, k_p), off=off, pdt=L.F32))
            w = src(name + "/kernel")
            w2 = w.reshape(-1, w.shape[-1]) if w.dim() == 3 and kg is not None else w.reshape(w.shape[0], -1)
            K, N = w2.shape
            if dst is None:
                dst = zeros(rows_p, k_p)
            L.check(L.lib.vtd_pack_dense(w2.data_ptr(), K, N, kg or K, kgp or K, ng or N,
                                         ngp or N, dst.data_ptr(), k_p, off,
                                         dt if pdt is None else pdt, stream),
                    f"pack {name}")
            return dst

        def f32_staging(rows_p, k_p):
            t = torch.zeros((rows_p, k_p), dtype=torch.float32, device=dev)
            staging.append(t)
            return t

        def mx8(w32, name):
            """MX-fp8 copy of a packed fp32 matrix [rows_p][k_p]: e4m3 [rows_p][K8] and
            scales [K8/128][rows_p][4] (vtd_quantize_mx8)."""
            rows_p, k_p = w32.shape
            k8 = -(-k_p // 128) * 128
            q = zeros(rows_p, k8, dtype=torch.uint8)
            sc = zeros(k8 // 128 * rows_p * 4, dtype=torch.uint8)
            L.check(L.lib.vtd_quantize_mx8(w32.data_ptr(), L.F32, rows_p, k_p, k_p, k8,
                                           q.data_ptr(), k8, sc.data_ptr(), rows_p, stream),
                    f"quantize {name}")
            return q.data_ptr(), sc.data_ptr()

        def enc(name, rows_p, k_p, **kw):
            """Encoder Dense layer: packed in the compute dtype, or MX-fp8 in FP8 mode.
            Returns (matrix pointer, scale pointer or None)."""
            if not fp8:
                t = dense(name, rows_p, k_p, **kw)
                rec(name + "/kernel", t, kg=kw.get("kg"), kgp=kw.get("kgp"))
                return t.data_ptr(), None
            return mx8(dense(name, rows_p, k_p, dst=f32_staging(rows_p, k_p), pdt=L.F32, **kw),
                       name)

        # LayerNorm fold (bf16 mode): LN1 into query/key/value, LN2 into the first MLP
        # layer (vtd_fold_layernorm); the forward then runs vtd_layernorm_stats instead of
        # the LayerNorm passes.  VTD_LN_FOLD=0 keeps the LayerNorm passes (A/B switch).
        # The folded GEMMs read the residual stream x as their bf16 A operand, so the fold
        # needs the bf16 stream: VTD_RESID_F32=1 (an f32 stream) turns it off.
        fold = (self.dtype == L.BF16 and os.environ.get("VTD_LN_FOLD", "1") != "0"
                and os.environ.get("VTD_RESID_F32", "0") in ("", "0"))

        def fold_ln(w32, b32, gamma, beta):
            """(W * diag(gamma), b + W beta, colsum) of a packed fp32 [N_p][K_p] matrix; the
            job is kept in `folds` for the refresh after an optimizer step."""
            n_p, k_p = w32.shape
            wo = zeros(n_p, k_p)
            bo = zeros(n_p, dtype=torch.float32)
            cs = zeros(n_p, dtype=torch.float32)
            L.check(L.lib.vtd_fold_layernorm(w32.data_ptr(), n_p, k_p, k_p, gamma.data_ptr(),
                                             beta.data_ptr(), b32.data_ptr(), wo.data_ptr(),
                                             k_p, dt, bo.data_ptr(), cs.data_ptr(), stream),
                    "fold_layernorm")
            folds.append(dict(shape=(n_p, k_p), gamma=gamma, beta=beta, bias_in=b32, wo=wo,
                              bo=bo, cs=cs))
            return wo.data_ptr(), bo.data_ptr(), cs.data_ptr()

        def vector(name, n_p, ng=None, ngp=None, dst=None, off=0):
            v = src(name).reshape(-1)
            if dst is None:
                dst = zeros(n_p, dtype=torch.float32)
            N = v.numel()
            L.check(L.lib.vtd_pack_vector(v.data_ptr(), N, ng or N, ngp or N, dst.data_ptr(),
                                          off, stream), f"pack {name}")
            return dst

        kw = self.kwargs
        dk, dkp = kw["encoder_key_dim"], dims.key_dim_p
        W = L.VtdWeights()
        W.w_patch = rec("linear_projection/kernel",
                        dense("linear_projection", dims.d_p, dims.patch_dim_p))
        W.b_patch = rec("linear_projection/bias", vector("linear_projection/bias", dims.d_p))
        pos = src("position_encoding/position_embedding/embeddings").reshape(-1)
        keep.append(pos)
        rec("position_encoding/position_embedding/embeddings", pos)
        W.pos_embedding = pos.data_ptr()
        nl = kw["encoder_repeat_times"]
        layers = (L.VtdLayerWeights * nl)()
        for i in range(1, nl + 1):
            ln1 = "layer_normalization" if i == 1 else f"layer_normalization_{2 * i - 2}"
            ln2 = f"layer_normalization_{2 * i - 1}"
            mha = "multi_head_attention" if i == 1 else f"multi_head_attention_{i - 1}"
            Ly = layers[i - 1]
            g1, b1 = vector(f"{ln1}/gamma", dims.d_p), vector(f"{ln1}/beta", dims.d_p)
            g2, b2 = vector(f"{ln2}/gamma", dims.d_p), vector(f"{ln2}/beta", dims.d_p)
            Ly.ln1_gamma, Ly.ln1_beta = g1.data_ptr(), b1.data_ptr()
            Ly.ln2_gamma, Ly.ln2_beta = g2.data_ptr(), b2.data_ptr()
            for n, t in ((f"{ln1}/gamma", g1), (f"{ln1}/beta", b1), (f"{ln2}/gamma", g2),
                         (f"{ln2}/beta", b2)):
                rec(n, t)
            wqkv = (f32_staging(dims.qkv_p, dims.d_p) if fp8 or fold or x3
                    else zeros(dims.qkv_p, dims.d_p))
            bqkv = zeros(dims.qkv_p, dtype=torch.float32)
            for part_i, part in enumerate(("query", "key", "value")):
                off = part_i * dims.inner_p
                # EinsumDense kernel (D, H, dk) -> (D, H*dk); columns padded per head
                dense(f"{mha}/{part}", None, dims.d_p, ng=dk, ngp=dkp, dst=wqkv, off=off,
                      pdt=L.F32 if fp8 or fold or x3 else None)
                vector(f"{mha}/{part}/bias", None, ng=dk, ngp=dkp, dst=bqkv, off=off)
            wqkv_op = None if fp8 or fold else split3(wqkv) if x3 else wqkv
            Ly.w_qkv, Ly.s_qkv = (mx8(wqkv, f"{mha}/qkv") if fp8 else
                                  (wqkv.data_ptr() if fold else wqkv_op.data_ptr(), None))
            Ly.b_qkv = bqkv.data_ptr()
            if fold:
                Ly.w_qkv, Ly.b_qkv, Ly.ln1_colsum = fold_ln(wqkv, bqkv, g1, b1)
            for part_i, part in enumerate(("query", "key", "value")):
                off = part_i * dims.inner_p
                if not fp8:
                    rec(f"{mha}/{part}/kernel", wqkv_op, fold=len(folds) - 1 if fold else None,
                        ng=dk, ngp=dkp, off=off)
                rec(f"{mha}/{part}/bias", bqkv, ng=dk, ngp=dkp, off=off)
            # attention_output kernel (H, dk, D) -> (H*dk, D); rows padded per head
            Ly.w_out, Ly.s_out = enc(f"{mha}/attention_output", dims.d_p, dims.inner_p, kg=dk,
                                     kgp=dkp)
            Ly.b_out = rec(f"{mha}/attention_output/bias",
                           vector(f"{mha}/attention_output/bias", dims.d_p))
            k_p = dims.d_p
            for j in range(kw["encoder_mlp_quantities"]):
                n_p = dims.mlp_units_p[j]
                bm = vector(f"MLP_{i}_{j + 1}/bias", n_p)
                rec(f"MLP_{i}_{j + 1}/bias", bm)
                if fold and j == 0:
                    w32 = dense(f"MLP_{i}_{j + 1}", n_p, k_p, dst=f32_staging(n_p, k_p), pdt=L.F32)
                    Ly.w_mlp[j], Ly.b_mlp[j], Ly.ln2_colsum = fold_ln(w32, bm, g2, b2)
                    rec(f"MLP_{i}_{j + 1}/kernel", fold=len(folds) - 1)
                else:
                    Ly.w_mlp[j], Ly.s_mlp[j] = enc(f"MLP_{i}_{j + 1}", n_p, k_p)
                    Ly.b_mlp[j] = bm.data_ptr()
                k_p = n_p
        W.layers = ctypes.cast(layers, ctypes.POINTER(L.VtdLayerWeights))
        W.w_det = rec("dense/kernel", dense("dense", L.KALIGN, dims.d_p))
        W.b_det = rec("dense/bias", vector("dense/bias", L.KALIGN))
        k_p = dims.tokens_p
        for j in range(dims.n_head):
            n_p = dims.head_units_p[j]
            W.w_head[j] = rec(f"dense_{j + 1}/kernel", dense(f"dense_{j + 1}", n_p, k_p))
            W.b_head[j] = rec(f"dense_{j + 1}/bias", vector(f"dense_{j + 1}/bias", n_p))
            k_p = n_p
        W.w_final = rec("MLP_Head_no_Sigmoid/kernel", dense("MLP_Head_no_Sigmoid", L.KALIGN, k_p))
        W.b_final = rec("MLP_Head_no_Sigmoid/bias", vector("MLP_Head_no_Sigmoid/bias", L.KALIGN))
        torch.cuda.current_stream(dev).synchronize()
        del staging      # fp32 staging copies; the packed buffers stay alive in `keep`
        self._packed = keep
        self._train_packed, self._fold_jobs = train, folds
        self._layers_c = layers
        self._weights_c = W

    # ---- forward
    def _workspace(self, batch: int):
        need = self.workspace_bytes(batch)
        if self._ws is None or self._ws_bytes < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        return self._ws

    def _as_images(self, images) -> torch.Tensor:
        x = images if torch.is_tensor(images) else torch.as_tensor(np.asarray(images))
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_shape:
            raise ValueError(
                f"Input 0 of layer \"{self.name}\" is incompatible with the layer: expected "
                f"shape=(None, {', '.join(map(str, self.input_shape))}), found shape="
                f"{tuple(x.shape)}")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def forward(self, images, with_detections: bool = False, stream=None):
        x = self._as_images(images)
        b = x.shape[0]
        logits = torch.empty((b, L.MAX_DETECT, 6), dtype=torch.float32, device=self.device)
        dets = torch.empty_like(logits) if with_detections else None
        ws = self._workspace(b)
        cfg = self.config(b)
        with torch.cuda.device(self.device):
            st = L.stream_ptr(stream)
            L.check(L.lib.vtd_forward(ctypes.byref(cfg), ctypes.byref(self._weights_c),
                                      x.data_ptr(), logits.data_ptr(), L.ptr(dets),
                                      ws.data_ptr(), ws.numel(), st), "vtd_forward")
        return (logits, dets) if with_detections else logits

    def __call__(self, images, training=None, **_):
        if training:
            raise ValueError("this forward path is inference-only (training=False)")
        return self.forward(images)

    def detect(self, images):
        """(logits, transform_predictions(logits)) with the decode fused on device."""
        return self.forward(images, with_detections=True)

    def detections(self, images, objectness_threshold: float = 0.5,
                   classification_threshold: float = 0.5):
        """Forward + transform_predictions + the prediction test MeanAveragePrecision
        applies (vtd.py:1359-1384), fused on the device.  Returns (logits, dets,
        category int32, valid bool), all (B, 17[, 6]) device tensors."""
        logits = self.forward(images)
        return (logits,) + decode_detections(logits, objectness_threshold,
                                             classification_threshold)

    def predict(self, x, batch_size: int = 32, verbose=0):
        """keras.Model.predict: numpy in, numpy (N, 17, 6) logits out, batches of 32."""
        x = np.asarray(x, dtype=np.float32)
        outs = []
        for i in range(0, x.shape[0], batch_size):
            outs.append(self.forward(x[i:i + batch_size]).cpu().numpy())
        return np.concatenate(outs, axis=0) if outs else np.zeros((0, L.MAX_DETECT, 6),
                                                                  np.float32)

    # ---- compile / evaluate (ipynb:408-435, 835; vtd.py:2172)
    def compile(self, optimizer=None, loss=None, metrics=None, dropout_seed=None, **_):
        """keras.Model.compile: stores `optimizer`, `loss`, `metrics` and `dropout_seed`.
        `optimizer` is kept as
        given and never refused here -- optimizers.Adam or the string "adam" (= Adam()) train the
        head (train_head_on_batch, fit_head) or every weight (train_on_batch, fit); anything
        else raises only when a training call needs it.  `loss` is my_custom_loss or a
        functools.partial of it (its keywords are read off and evaluate runs the fused
        from-logits kernel), or any callable (y_true, logits) -> scalar, called per batch.
        `metrics`: objects with update_state / result / reset_state (MeanAveragePrecision).
        `dropout_seed` (an int below 2^64, kept as `model.dropout_seed`; None, the default, clears
        it as a missing `loss` clears the loss): with it a model built with `dropout` > 0 applies
        that dropout in the gradient and training calls -- every mask a function of (this seed,
        the step, the site, the index) alone, DESIGN.md "Dropout" -- and without it those calls
        run the dropout=None graph (train_on_batch / fit raise).  It changes nothing for a model
        without dropout, and nothing in model(images), predict or evaluate."""
        if dropout_seed is not None:
            if isinstance(dropout_seed, bool) or not isinstance(dropout_seed, (int, np.integer)) \
                    or not 0 <= int(dropout_seed) < 1 << 64:
                raise ValueError(f"compile: dropout_seed must be an int in [0, 2^64), got "
                                 f"{dropout_seed!r}")
            dropout_seed = int(dropout_seed)
        if loss is not None and not callable(loss):
            raise TypeError(f"compile: loss must be callable, got {type(loss).__name__}")
        metrics = list(metrics or [])
        for m in metrics:
            if not all(callable(getattr(m, a, None)) for a in ("update_state", "result",
                                                               "reset_state")):
                raise TypeError(f"compile: metric {m!r} needs update_state / result / reset_state")
        if isinstance(optimizer, str) and optimizer.lower() == "adam":
            from .optimizers import Adam
            optimizer = Adam()
        self.loss, self.metrics, self.optimizer = loss, metrics, optimizer
        self.dropout_seed = dropout_seed

    def _evaluate_batches(self, x, y, batch_size):
        if y is None:
            yield from x
            return
        if len(x) != len(y):
            raise ValueError(f"evaluate: {len(x)} images but {len(y)} labels")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"evaluate: batch_size must be >= 1, got {batch_size}")
        for i in range(0, len(x), batch_size):
            yield x[i:i + batch_size], y[i:i + batch_size]

    def evaluate(self, x, y=None, batch_size=32, verbose=0, return_dict=False, **_):
        """keras.Model.evaluate: the loss (the Keras loss metric: the mean over batches
        weighted by batch size) and the compiled metrics over a dataset.  With `y`, `x` and
        `y` are arrays / tensors split into batches of `batch_size` (the last may be short);
        with y=None `x` is an iterable of (images, labels) batches.  Per batch the forward,
        the loss (vtd_loss on the logits, adding into a device accumulator) and every
        metric's update_state(labels, logits) are queued on the current stream; the one host
        read comes at the end.  Metrics are reset first, as Keras does.  Returns the loss
        (no metrics), [loss, *metric results] as Python floats, or with return_dict
        {"loss": ..., "<metric.name>": ...}."""
        del verbose
        if self.loss is None:
            raise RuntimeError("evaluate: the model has no loss; call "
                               "compile(loss=my_custom_loss or a functools.partial of it) first")
        from . import loss as _loss
        from .metrics import _device_f32
        params = _loss.fused_loss_params(self.loss)
        for m in self.metrics:
            m.reset_state()
        with torch.cuda.device(self.device):
            running = torch.zeros(2, dtype=torch.float64, device=self.device)
            for images, labels in self._evaluate_batches(x, y, batch_size):
                logits = self.forward(images)
                labels = _device_f32(labels, self.device)
                if labels.shape != logits.shape:
                    raise ValueError(f"evaluate: labels {tuple(labels.shape)} do not match the "
                                     f"logits {tuple(logits.shape)}")
                n = logits.shape[0]
                if n == 0:
                    continue
                if params is not None:
                    _loss._launch(labels, logits, params, running)
                else:
                    value = torch.as_tensor(self.loss(labels, logits)).to(
                        device=self.device, dtype=torch.float64).reshape(())
                    running[0] += value * n
                    running[1] += n
                for m in self.metrics:
                    m.update_state(labels, logits)
            # one device-to-host read: the accumulator and every metric's result
            results = [torch.as_tensor(m.result()).to(device=self.device, dtype=torch.float64)
                       .reshape(1) for m in self.metrics]
            read = torch.cat([running, *results]).cpu().tolist()
        # sum(loss_b * n_b) / sum(n_b); 0 / 0 (no data) is nan, as an empty Keras mean would be
        values = [read[0] / read[1] if read[1] else float("nan")] + read[2:]
        if return_dict:
            names = ["loss"] + [getattr(m, "name", type(m).__name__) for m in self.metrics]
            return dict(zip(names, values))
        return values if self.metrics else values[0]

    def loss_and_grad(self, images, y_true):
        """The forward and the compiled loss with its gradient at the logits: (out5,
        d loss / d logits), both on the device, as loss.loss_and_grad(y_true, model(images),
        <the compiled keywords>) returns them -- where a backward pass through the model
        starts (head_gradients carries it through the detection head).  Needs compile(loss=my_custom_loss or a functools.partial of it)."""
        from . import loss as _loss
        params = _loss.fused_loss_params(self.loss) if self.loss is not None else None
        if params is None:
            raise ValueError("loss_and_grad: compile(loss=my_custom_loss or a functools.partial "
                             "of it with keyword arguments) first")
        with torch.cuda.device(self.device):
            return _loss.loss_and_grad(y_true, self.forward(images), params=params)

    # ---- head backward (vtd_forward_encoded, vtd_head_backward)
    def encode(self, images, stream=None):
        """Keras layer `encoded_images`: the encoder's output, the residual stream after the
        last layer, as a (B, N, d) fp32 device tensor (vtd_forward_encoded: the forward's own
        stages, without the head)."""
        x = self._as_images(images)
        b = x.shape[0]
        out = torch.empty((b, self.dims.tokens, self.dims.d), dtype=torch.float32,
                          device=self.device)
        ws = self._workspace(b)
        cfg = self.config(b)
        with torch.cuda.device(self.device):
            L.check(L.lib.vtd_forward_encoded(ctypes.byref(cfg), ctypes.byref(self._weights_c),
                                              x.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                              ws.numel(), L.stream_ptr(stream)),
                    "vtd_forward_encoded")
        return out

    def head_weight_names(self):
        """The Keras weight names of the detection head, in `weight_names()` order."""
        names = ["dense/kernel", "dense/bias"]
        for j in range(self.dims.n_head):
            names += [f"dense_{j + 1}/kernel", f"dense_{j + 1}/bias"]
        return names + ["MLP_Head_no_Sigmoid/kernel", "MLP_Head_no_Sigmoid/bias"]

    def encoder_block_weights(self, i: int):
        """The weights of encoder block i (0 <= i < encoder_repeat_times) as `encoder_block`
        takes them: an OrderedDict of Keras name -> fp32 device tensor in the Keras shape, in
        creation order (ln1 gamma, beta; query, key, value, attention_output kernel and bias;
        ln2 gamma, beta; the MLP kernel / bias pairs).  Fresh copies of the model's current
        weights -- ordinary tensors, the caller sets requires_grad; the packed buffers of the
        forward are not touched."""
        reps = self.kwargs["encoder_repeat_times"]
        if not isinstance(i, int) or not 0 <= i < reps:
            raise ValueError(f"encoder_block_weights: block index {i!r} must be an int in "
                             f"[0, {reps})")
        per = 12 + 2 * self.kwargs["encoder_mlp_quantities"]
        names = list(self.weight_shapes)[3 + i * per: 3 + (i + 1) * per]
        return self._current(names)

    def _current(self, names):
        """Fresh device copies of encoder / stem weights: of the device masters where optimizer
        steps have moved them ahead of the CPU masters, else of the CPU masters."""
        if self._enc_dirty:
            live = self._encoder_master()
            return OrderedDict((n, live[n].clone()) for n in names)
        return OrderedDict((n, self._master[n].to(self.device).contiguous()) for n in names)

    def _device_master(self, part, names):
        """fp32 device copies of the weights `names` in the Keras layout, made once per
        set_weights and held under `part`."""
        held = self.__dict__.setdefault("_dev_masters", {})
        if part not in held or held[part][0] is not self._master:
            held[part] = (self._master, OrderedDict(
                (n, self._master[n].to(self.device).contiguous()) for n in names))
        return held[part][1]

    def _head_master(self):
        """The device masters of the head's weights (vtd_head_params)."""
        return self._device_master("head", self.head_weight_names())

    def head_weights(self):
        """The weights of the detection head as `detection_head` takes them: an OrderedDict of
        Keras name -> fp32 device tensor in the Keras shape, in creation order
        (`head_weight_names()`).  Fresh copies of the model's current weights, as
        `stem_weights` returns the stem's."""
        return OrderedDict((n, t.clone()) for n, t in self._head_master().items())

    def detection_head(self, encoded, weights=None, *, seed=None, step=0, dropout=None,
                       site_base=None):
        """The detection head (mlp_head, vtd.py:454-493) as a differentiable op: logits
        (B, 17, 6) from `encoded` (B, N, d), a float32 device tensor.  backward() fills
        encoded.grad and the gradient of every tensor of `weights` that requires grad.
        `weights`: the head's tensors in creation order and Keras shapes (a sequence, or a dict
        whose values are taken; `head_weights()` returns them so); None: the model's current
        head weights.  The forward is vtd_head_backward's forward-only call, the backward one
        forward + backward call; so patch_embedding -> encoder_block x L -> detection_head ->
        my_custom_loss is one autograd chain.

        Dropout: `seed` None is the dropout=None head, bit for bit.  With a seed, `dropout`
        (default: the rate the model was built with) follows every head Dense + activation --
        none after Dense(17) or MLP_Head_no_Sigmoid -- head layer j at site `site_base + j`
        (default site_base: encoder_repeat_times * (1 + encoder_mlp_quantities), after the
        blocks' sites), over the unpadded [B 17][units_j] activation; the backward regenerates
        the forward's masks from (seed, step, site).  A positive `dropout` given without a seed
        raises.  Needs dtype 'bf16x3' or 'bfloat16'."""
        from . import head as _head
        from .dropout import spec
        what = "detection_head"
        self._require(what, loss=False)
        dims = self.dims
        if not torch.is_tensor(encoded) or not encoded.is_cuda or encoded.dtype != torch.float32:
            raise ValueError(f"{what}: encoded must be a float32 device tensor")
        if encoded.dim() != 3 or tuple(encoded.shape[1:]) != (dims.tokens, dims.d) \
                or encoded.shape[0] < 1:
            raise ValueError(f"{what}: encoded must be (B, {dims.tokens}, {dims.d}), got "
                             f"{tuple(encoded.shape)}")
        names = self.head_weight_names()
        if weights is None:
            weights = list(self._head_master().values())
        else:
            weights = list(weights.values()) if isinstance(weights, dict) else list(weights)
            if len(weights) != len(names):
                raise ValueError(f"{what}: weights must hold {len(names)} tensors "
                                 f"({', '.join(names)}), got {len(weights)}")
            for n, t in zip(names, weights):
                if not torch.is_tensor(t) or t.dtype != torch.float32 \
                        or t.device != encoded.device:
                    raise ValueError(f"{what}: {n} must be a float32 tensor on encoded's device")
                if tuple(t.shape) != tuple(self.weight_shapes[n]):
                    raise ValueError(f"{what}: {n} has shape {tuple(t.shape)}, expected "
                                     f"{self.weight_shapes[n]}")
        if dropout is None and seed is not None:
            dropout = self.kwargs.get("dropout")
        if site_base is None:
            site_base = self._head_site_base()
        d1 = spec(what, dropout, seed, step, site_base)
        drop = None
        if d1 is not None:
            if int(site_base) + dims.n_head >= 1 << 32:
                raise ValueError(f"{what}: site_base + the head's layers must fit 32 bits")
            drop = L.VtdBlockDropout(seed=d1.seed, step=d1.step, site_base=d1.site, rate=d1.rate)
        return _head.DetectionHead.apply(encoded.contiguous(),
                                         (self.config(encoded.shape[0]), drop), *weights)

    # ---- dropout in the gradient and training calls (compile(dropout_seed=))
    def _head_site_base(self):
        """The head's first dropout site: after block i's site_base = i * (1 + q)."""
        return self.kwargs["encoder_repeat_times"] * (1 + self.kwargs["encoder_mlp_quantities"])

    def _call_dropout(self, what, step):
        """The dropout of one gradient / training call: None -- a model without dropout, or no
        compiled seed -- or (rate, seed, step)."""
        rate = self.kwargs.get("dropout")
        if not rate or self.dropout_seed is None:
            return None
        from .dropout import spec
        d1 = spec(what, rate, self.dropout_seed, step)
        return d1.rate, d1.seed, d1.step

    def _site_dropout(self, drop, block=None):
        """The VtdBlockDropout of encoder block `block` (site_base = block * (1 + q)), or of the
        head (block=None), for a `_call_dropout` result; None for None."""
        if drop is None:
            return None
        base = (self._head_site_base() if block is None
                else block * (1 + self.kwargs["encoder_mlp_quantities"]))
        return L.VtdBlockDropout(seed=drop[1], step=drop[2], site_base=base, rate=drop[0])

    def head_gradients(self, images, y_true, encoded=None, step=0):
        """One frozen-encoder training step up to the optimizer update: encoder features ->
        head -> compiled loss -> gradients.  Returns (out5, grads): out5 as loss_and_grad
        returns it (total, objectness, class, CIoU means, positives) and `grads` an OrderedDict
        of fp32 device tensors keyed by the head's Keras weight names (`head_weight_names()`)
        plus "encoded_images" (B, N, d) = d loss / d encoded_images, where an encoder backward
        would start.  `encoded`: the (B, N, d) output of `encode` -- the cached-features use,
        `images` is then ignored.  The logits gradient is vtd_loss_grad's, the rest
        vtd_head_backward.  On a model built with `dropout` and compiled with a `dropout_seed`
        the head's dropout sites are on, masks of (seed, `step`, site) -- the encoder stays the
        inference forward; otherwise `step` is not used.  Needs compile(loss=my_custom_loss or a
        functools.partial of it) and dtype 'bf16x3' or 'bfloat16'."""
        return self._head_pass("head_gradients", images, y_true, encoded,
                               drop=self._call_dropout("head_gradients", step))

    # ---- whole-model gradients (vtd_stem_backward, vtd_encoder_block_backward, vtd_head_backward)
    def stem_weights(self):
        """The weights of the patch embedding as `patch_embedding` takes them: an OrderedDict of
        Keras name -> fp32 device tensor in the Keras shape, in creation order (the position
        embedding (tokens, 1), the linear_projection kernel and bias).  Fresh copies of the
        model's current weights, as `encoder_block_weights` returns a block's."""
        return self._current(list(self.weight_shapes)[:3])

    def _encoder_master(self):
        """The device masters of the stem's and every encoder block's weights (vtd_stem_params,
        vtd_block_params)."""
        per = 12 + 2 * self.kwargs["encoder_mlp_quantities"]
        names = list(self.weight_shapes)[:3 + self.kwargs["encoder_repeat_times"] * per]
        return self._device_master("encoder", names)

    def gradients(self, images, y_true, step=0, image_gradient=False):
        """The gradient of the compiled loss with respect to every weight: the training forward
        of the whole model, the loss gradient at its logits, and the backward through the head,
        every encoder block in reverse and the patch embedding.  Returns (out5, grads): out5 as
        head_gradients returns it and `grads` an OrderedDict with exactly the keys of
        `weight_names()`, in that order, of fp32 device tensors in the Keras shapes (the position
        embedding (tokens, 1)).  The loss reported is that of the training-forward chain -- an
        fp32 residual stream, every LayerNorm applied as written -- not of `model(images)`,
        whose forward folds the LayerNorms into the next kernels and, in 'bfloat16', keeps a
        bf16 residual stream; the two agree within the mode's forward tolerance.  Steps, all on
        the current stream with no host read: vtd_stem_backward (forward only),
        vtd_encoder_block_backward per block (forward only, every block input kept),
        head_gradients' pass on the last block's output, then the blocks' backward calls in
        reverse through one shared workspace and the stem's.  On a model built with `dropout`
        and compiled with a `dropout_seed` every dropout site of the reference's training graph
        is on (vtd_encoder_block_backward_dropout with site_base = i (1 + q) for block i,
        vtd_head_backward_dropout with site_base = L (1 + q)), the masks those of (seed, `step`,
        site): the same step gives the same bits; otherwise `step` is not used.
        image_gradient=True: `grads` gains one last key, "images" -- d loss / d images, an fp32
        (B, H, W, C) device tensor, of the float32 images the chain read (after `_as_images`) --
        from one vtd_stem_image_grad call on the first block's input gradient, after the stem's
        backward; out5 and every other entry keep their bits.  Needs compile(loss=my_custom_loss
        or a functools.partial of it) and dtype 'bf16x3' or 'bfloat16'."""
        return self._grad_chain("gradients", images, y_true, step=step,
                                image_gradient=image_gradient)

    def image_gradient(self, images, y_true, step=0):
        """(out5, dimages): the loss terms and d loss / d images, fp32 (B, H, W, C) -- what a
        saliency map, a sign-gradient step on the inputs or an input optimisation starts from.
        The chain of gradients(..., image_gradient=True), weight gradients included (there is no
        backward that skips them), and the bits of its "images" entry; dropout and `step` as
        there."""
        out5, grads = self._grad_chain("image_gradient", images, y_true, step=step,
                                       image_gradient=True)
        return out5, grads["images"]

    def _grad_chain(self, what, images, y_true, buffers=None, step=0, image_gradient=False):
        """The chain gradients and train_on_batch share.  `buffers`: Keras name -> fp32 device
        tensor to write each weight gradient into (the optimizer's persistent ones); None
        allocates fresh tensors.  `step`: the dropout step (`_call_dropout`).  Returns (out5,
        grads keyed by `weight_names()`, then "images" with `image_gradient`)."""
        self._require(what)
        drop = self._call_dropout(what, step)
        from . import encoder as _enc
        from . import stem as _stem
        x = self._as_images(images)
        b = x.shape[0]
        kw, dims = self.kwargs, self.dims
        reps, per = kw["encoder_repeat_times"], 12 + 2 * kw["encoder_mlp_quantities"]
        sdims = L.VtdStemDims(batch=b, H=self.input_shape[0], W=self.input_shape[1],
                              C=self.input_shape[2], patch=kw["patch_size"], d=dims.d,
                              dtype=self.dtype)
        bdims = L.VtdBlockDims(batch=b, tokens=dims.tokens, d=dims.d,
                               num_heads=kw["encoder_num_heads"], key_dim=kw["encoder_key_dim"],
                               mlp_quantities=kw["encoder_mlp_quantities"],
                               use_mish=1 if kw["use_mish"] else 0, dtype=self.dtype)
        with torch.cuda.device(self.device):
            need = (_stem.workspace_bytes(sdims), _enc.workspace_bytes(bdims))
            held = getattr(self, "_grad_ws", (None, None))
            self._grad_ws = tuple(
                t if t is not None and t.numel() >= n
                else torch.empty(n, dtype=torch.uint8, device=self.device)
                for t, n in zip(held, need))
            stem_ws, block_ws = self._grad_ws
            wdev = list(self._encoder_master().values())
            sw = wdev[:3]
            bw = [wdev[3 + i * per: 3 + (i + 1) * per] for i in range(reps)]
            xs = [_stem.run(x, sw, sdims, ws=stem_ws)[0]]
            bdrop = [self._site_dropout(drop, i) for i in range(reps)]
            for i in range(reps):
                xs.append(_enc.run(xs[i], bw[i], bdims, ws=block_ws, drop=bdrop[i])[0])
            names = list(self.weight_shapes)
            into = None if buffers is None else [buffers[n] for n in names]
            head_into = None
            if into is not None:
                head_into = OrderedDict(zip(names[3 + reps * per:], into[3 + reps * per:]))
                head_into["encoded_images"] = torch.empty_like(xs[reps])
            out5, head = self._head_pass(what, None, y_true, xs[reps], weight_grads=head_into,
                                         drop=drop)
            head = OrderedDict(head)
            dy = head.pop("encoded_images")
            found = []
            for i in range(reps - 1, -1, -1):
                out = None if into is None else (None, into[3 + i * per: 3 + (i + 1) * per], None)
                _, g, dy = _enc.run(xs[i], bw[i], bdims, dy=dy, want_y=False, ws=block_ws,
                                    out=out, drop=bdrop[i])
                found = g + found
            _, g = _stem.run(x, sw, sdims, dx0=dy, want_x0=False, ws=stem_ws,
                             out=None if into is None else (None, into[:3]))
            found = g + found + list(head.values())
            grads = OrderedDict(zip(self.weight_shapes, found))
            if image_gradient:
                n = _stem.image_grad_workspace_bytes(sdims)
                ws = getattr(self, "_image_grad_ws", None)
                if ws is None or ws.numel() < n:
                    ws = self._image_grad_ws = torch.empty(n, dtype=torch.uint8,
                                                           device=self.device)
                grads["images"] = _stem.image_grad(dy, sw[1], sdims, ws=ws)
        return out5, grads

    # ---- what the gradient and training calls share
    def _require(self, what, mode=True, loss=True, optimizer=False, whole_model=False):
        """The preconditions of the gradient and training calls, for the caller `what`, in this
        order: the mode (`mode`), for whole-model training (`whole_model`) a model without
        dropout or with a compiled dropout seed, a compiled fused loss (`loss`), a resolvable
        compiled optimizer (`optimizer`).  Returns (the fused loss parameters, the optimizer), None where not asked for."""
        if mode and self.dtype not in (L.BF16X3, L.BF16):
            does = "model trains" if whole_model else "head backward runs"
            raise ValueError(f"{what}: the {does} in the 'bf16x3' and 'bfloat16' modes only "
                             "(not float32 / float8)")
        if whole_model and self.kwargs.get("dropout") and self.dropout_seed is None:
            raise ValueError(f"{what}: this model was built with dropout="
                             f"{self.kwargs['dropout']!r} and no dropout seed is compiled; "
                             "compile(..., dropout_seed=<int>) trains it with that dropout (no "
                             "implicit randomness: the masks are a function of the seed and the "
                             "step)")
        params = resolved = None
        if loss:
            from . import loss as _loss
            params = _loss.fused_loss_params(self.loss) if self.loss is not None else None
            if params is None:
                raise ValueError(f"{what}: compile(loss=my_custom_loss or a functools.partial "
                                 "of it with keyword arguments) first")
        if optimizer:
            from . import optimizers as _opt
            try:
                resolved = _opt.resolve(self.optimizer)
            except ValueError as e:
                raise ValueError(f"{what}: {e}") from None
        return params, resolved

    def _fit_loop(self, what, optimizer, batches, step, epochs, lr_schedule, callbacks=()):
        """The epoch loop fit and fit_head share.  `batches()` yields an epoch's (images, labels)
        pairs and `step(i, images, labels)` trains on the i-th, returning out5.  `set_model(self)`
        is called once on the callbacks that have it.  Per epoch: `lr_schedule(epoch, lr)` sets
        the optimizer's rate, the batch losses weighted by batch size add up in a float64[2]
        device accumulator, ONE host read takes the mean into the History, and every callback
        that has `on_epoch_end` gets (epoch, {"loss": ...}).  `self.stop_training` is set to False
        at the start, and the loop ends after the callbacks of an epoch in which one of them set
        it to True (Keras's convention; health.CheckModelWeight(stop_on_nan=True) does)."""
        from . import optimizers as _opt
        from .metrics import _device_f32
        if int(epochs) < 0:
            raise ValueError(f"{what}: epochs must be >= 0, got {epochs}")
        self.stop_training = False
        for cb in callbacks:
            if callable(getattr(cb, "set_model", None)):
                cb.set_model(self)
        hist = _opt.History()
        with torch.cuda.device(self.device):
            running = torch.zeros(2, dtype=torch.float64, device=self.device)
            for epoch in range(int(epochs)):
                if lr_schedule is not None:
                    optimizer.learning_rate = float(lr_schedule(epoch, optimizer.learning_rate))
                running.zero_()
                for i, (images, labels) in enumerate(batches()):
                    n = len(labels)
                    if n == 0:
                        continue
                    out5 = step(i, images, _device_f32(labels, self.device))
                    running[0] += out5[0].double() * n
                    running[1] += n
                total, count = running.cpu().tolist()       # the epoch's one host read
                loss = total / count if count else float("nan")
                hist.history["loss"].append(loss)
                hist.epoch.append(epoch)
                for cb in callbacks:
                    if callable(getattr(cb, "on_epoch_end", None)):
                        cb.on_epoch_end(epoch, {"loss": loss})
                if self.stop_training:              # a callback asked for the end (Keras)
                    break
        return hist

    # ---- whole-model training (vtd_train_step, vtd_fold_layernorm_batch; optimizers.py)
    def train_on_batch(self, images, y_true):
        """keras.Model.train_on_batch over every weight: gradients' chain with each weight
        gradient written into the compiled optimizer's persistent buffers, then ONE
        vtd_train_step launch -- Adam (the position embedding in Keras's sparse-path order and
        without the constraint, as the reference builds it), ClipWeight (`max_weight` /
        `clip_weight` of the model's kwargs) and the re-pack of every operand the inference
        forward reads -- and, where the model was packed with the LayerNorm fold, one
        vtd_fold_layernorm_batch launch that refreshes the folded operands.  Returns out5 as
        gradients does, taken before the update, as Keras reports the loss; nothing is read
        back.  Afterwards the device masters are the truth for every tensor; get_weights /
        get_weight_dict / save_weights read them back on demand.  Needs
        compile(optimizer=optimizers.Adam(...) or 'adam', loss=my_custom_loss or a
        functools.partial of it) and dtype 'bf16x3' or 'bfloat16'; a model built with `dropout`
        also needs compile(dropout_seed=...), and its masks take `optimizer.iterations` as read
        before the step for the dropout step: 0 for the first step, one more per step."""
        _, optimizer = self._require("train_on_batch", optimizer=True, whole_model=True)
        buffers = optimizer.gradient_buffers(self, scope="all")   # (a fresh state counts from 0)
        out5, _ = self._grad_chain("train_on_batch", images, y_true, buffers,
                                   step=optimizer.iterations)
        optimizer.apply(self, scope="all")
        return out5

    def fit(self, x, y=None, batch_size=32, epochs=1, lr_schedule=None, callbacks=None,
            verbose=0):
        """keras.Model.fit over every weight: `epochs` passes of train_on_batch over the
        batches, formed as `evaluate` forms them (arrays split by `batch_size`, the last may be
        short; or y=None and `x` a re-iterable of (images, labels) batches).  `lr_schedule(epoch,
        lr) -> lr` is called at the start of every epoch, as keras.callbacks.
        LearningRateScheduler calls it.  `callbacks`: a list of objects; `set_model(model)` is
        called once on those that have it, `on_epoch_end(epoch, {"loss": ...})` after every
        epoch (no other Keras hook is called).  Returns an object whose .history["loss"] holds
        one float per epoch: the mean of the batch losses weighted by batch size, accumulated
        on the device and read once per epoch."""
        del verbose
        _, optimizer = self._require("fit", optimizer=True, whole_model=True)
        return self._fit_loop("fit", optimizer, lambda: self._evaluate_batches(x, y, batch_size),
                              lambda i, images, labels: self.train_on_batch(images, labels),
                              epochs, lr_schedule, list(callbacks or []))

    # ---- head training (the same vtd_train_step over the head's tensors; optimizers.py)
    def train_head_on_batch(self, images, y_true, encoded=None):
        """keras.Model.train_on_batch for the detection head on a frozen encoder: head_gradients'
        pass with the weight gradients written into the compiled optimizer's persistent buffers,
        then ONE vtd_train_step launch over the head's tensors -- Adam, the ClipWeight constraint
        (`max_weight` / `clip_weight` of the model's kwargs) and the re-pack of the forward's head
        operands.
        Returns out5 as head_gradients does, taken before the update, as Keras reports the
        loss; nothing is read back to the host.  Afterwards the device masters
        (`_head_master()`) are the truth for the head; get_weights / get_weight_dict /
        save_weights read them back on demand.  With `dropout` and a compiled `dropout_seed` the
        head's dropout sites are on, the dropout step `optimizer.iterations` as read before the
        step.  Needs compile(optimizer=optimizers.Adam(...) or 'adam', loss=my_custom_loss or a
        functools.partial of it) and dtype 'bf16x3' or 'bfloat16'."""
        # the compiled loss is _head_pass's check: a missing optimizer is reported first
        _, optimizer = self._require("train_head_on_batch", loss=False, optimizer=True)
        buffers = optimizer.gradient_buffers(self, scope="head")  # (a fresh state counts from 0)
        out5, _ = self._head_pass(
            "train_head_on_batch", images, y_true, encoded, weight_grads=buffers,
            drop=self._call_dropout("train_head_on_batch", optimizer.iterations))
        optimizer.apply(self, scope="head")
        return out5

    def fit_head(self, x, y=None, batch_size=32, epochs=1, lr_schedule=None, cache_features=True,
                 encoded=None, callbacks=None):
        """keras.Model.fit for the detection head on a frozen encoder (the notebook's "overfit
        a few images" loop): `epochs` passes of train_head_on_batch over the batches, which are
        formed as `evaluate` forms them (arrays split by `batch_size`, the last may be short; or
        y=None and `x` a re-iterable of (images, labels) batches).  `lr_schedule(epoch, lr) ->
        lr` is called at the start of every epoch with the optimizer's current rate, as
        keras.callbacks.LearningRateScheduler calls it, and its return becomes the rate.
        `cache_features`: the encoder runs once per batch and later epochs reuse its (B, N, d)
        features (the encoder is frozen, so they cannot change).  `encoded`: the features of
        the whole of `x` (len(x), N, d), as head_gradients takes them; `x` is then not read.
        `callbacks`: as `fit` takes them.  Returns an object whose .history["loss"] holds one float per epoch: the mean of the
        batch losses weighted by batch size (the Keras loss metric), accumulated on the device
        and read once per epoch."""
        # the mode and the loss are train_head_on_batch's checks, per batch
        _, optimizer = self._require("fit_head", mode=False, loss=False, optimizer=True)
        if encoded is not None:
            if y is None:
                raise ValueError("fit_head: encoded= needs the labels in y")
            fixed = list(self._evaluate_batches(encoded, y, batch_size))
            features = [b[0] for b in fixed]
            batches = lambda: fixed                                        # noqa: E731
        else:
            features = {}
            batches = lambda: self._evaluate_batches(x, y, batch_size)     # noqa: E731

        def step(i, images, labels):
            if encoded is None and cache_features and i not in features:
                features[i] = self.encode(images)
            feats = features[i] if encoded is not None or cache_features else None
            return self.train_head_on_batch(images, labels, encoded=feats)
        return self._fit_loop("fit_head", optimizer, batches, step, epochs, lr_schedule,
                              list(callbacks or []))

    def _head_pass(self, what, images, y_true, encoded, weight_grads=None, drop=None):
        """The part head_gradients and train_head_on_batch share: the checks, the encoder
        features, the training forward for the logits, the loss gradient there, and the
        backward.  `weight_grads`: buffers to write the weight gradients into (the optimizer's
        persistent ones; d loss / d encoded_images is then not computed); None allocates them
        and the encoded_images gradient.  `drop`: the call's dropout (`_call_dropout`): the
        head's sites of both chain calls.  Returns (out5, grads)."""
        from . import head as _head
        from . import loss as _loss
        params, _ = self._require(what)
        dims = self.dims
        with torch.cuda.device(self.device):
            if encoded is None:
                encoded = self.encode(images)
            else:
                encoded = torch.as_tensor(encoded).to(device=self.device,
                                                      dtype=torch.float32).contiguous()
                if encoded.dim() != 3 or tuple(encoded.shape[1:]) != (dims.tokens, dims.d):
                    raise ValueError(f"{what}: encoded must be (B, {dims.tokens}, "
                                     f"{dims.d}), got {tuple(encoded.shape)}")
            b = encoded.shape[0]
            cfg = self.config(b)
            need = _head.workspace_bytes(cfg)
            if getattr(self, "_hb_ws", None) is None or self._hb_ws.numel() < need:
                self._hb_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            wdev = self._head_master()
            if weight_grads is None:
                grads = OrderedDict((n, torch.empty_like(t)) for n, t in wdev.items())
                grads["encoded_images"] = torch.empty_like(encoded)
            else:
                grads = weight_grads
            weights = list(wdev.values())
            hdrop = self._site_dropout(drop)
            # the training forward alone for its logits, the loss gradient at those logits,
            # then the forward again with the backward (with dropout: the same masks again)
            logits = torch.empty((b, L.MAX_DETECT, 6), dtype=torch.float32, device=self.device)
            _head.run(cfg, encoded, weights, logits=logits, ws=self._hb_ws, drop=hdrop)
            out5, dlogits = _loss.loss_and_grad(y_true, logits, params=params)
            _head.run(cfg, encoded, weights, dlogits=dlogits, grads=[grads[n] for n in wdev],
                      d_encoded=grads.get("encoded_images"), ws=self._hb_ws, drop=hdrop)
        return out5, grads

    # ---- numerical health (vtd_tensor_stats; health.py)
    def weight_stats(self):
        """The statistics of every weight as it is on the device NOW: an OrderedDict over
        `weight_names()` of health.TensorStat (NaN / +Inf / -Inf counts, the non-NaN max / min, the
        fp64 sum of squares and `norm`), read from the device masters (`_encoder_master()` +
        `_head_master()`) -- after optimizer steps the stepped weights, with no read-back of the
        weights themselves (`_sync_master` is not called).  One vtd_tensor_stats launch pair and
        one host read of 48 B per tensor; the uploaded plan and its workspace are kept on the
        model and rebuilt when set_weights replaces the masters.  Works in every `dtype`."""
        from . import health as _health
        held = getattr(self, "_health_plan", None)
        if held is None or held[0] is not self._master:
            w = OrderedDict(self._encoder_master())
            w.update(self._head_master())
            assert list(w) == self.weight_names()
            held = self._health_plan = (self._master, _health._Plan(list(w.values()),
                                                                    what="weight_stats"))
        return OrderedDict(zip(self.weight_shapes, held[1].run()))

    def count_params(self) -> int:
        return int(sum(int(np.prod(s)) for s in self.weight_shapes.values()))


_DEFAULTS = dict(                                          # vtd.py:498-506
    input_shape=None, patch_size=17, embedding_dim=28, encoder_num_heads=8,
    encoder_key_dim=40, dropout=None, encoder_mlp_quantities=8, encoder_repeat_times=8,
    mlp_head_last_units=136, mlp_head_dense_layers_quantity=7,
    mlp_head_dense_mish_block_repeats=1, use_mish=True, max_weight=10, clip_weight=True,
    training=None)


def create_vision_transformer_detector(
        input_shape=None, patch_size=17, embedding_dim=28,
        encoder_num_heads=8, encoder_key_dim=40, dropout=None,
        encoder_mlp_quantities=8,
        encoder_repeat_times=8,
        mlp_head_last_units=136, mlp_head_dense_layers_quantity=7,
        mlp_head_dense_mish_block_repeats=1,
        use_mish=True,
        max_weight=10, clip_weight=True, training=None,
        *, dtype="bf16x3", device=None, seed=0) -> Model:
    """Same kwargs and defaults as vtd.py:498-506.  `dropout` (MultiHeadAttention dropout and
    the Dropout layers after every MLP / head activation, vtd.py:359-369, 404-405, 485-486)
    is the identity at inference -- those layers run with the call's `training` flag, False
    in `model(x, training=False)` / `predict` -- and Dropout has no weights, so any rate in
    [0, 1) builds the same forward and the same weight names; only a build-time
    `training=True` (dropout forced on in every call) is refused.  The gradient and training calls
    apply a rate > 0 once `compile(..., dropout_seed=<int>)` names a seed (Model.compile).  `max_weight`/`clip_weight` are weight constraints
    Keras applies only after optimizer steps (vtd.py:209-236), so they do not affect
    the forward; train_head_on_batch / fit_head apply them after every step.  Extra keyword-only options: `dtype`, `device`,
    `seed`.  `dtype` defaults to 'bf16x3', the split-bf16 parity mode: every product as three
    bf16 MFMA products with fp32 accumulation and fp32 softmax / LayerNorm statistics, within
    1e-4 of the fp32 reference's logits (measured 1.6e-5 at C2) -- so a caller that swaps the
    reference's import for this one gets the reference's fp32 numbers.  'bfloat16' is the
    throughput mode (~1e-2 from fp32, ~3x the images/s), 'float32' the exact-fp32 MFMA mode,
    'float8' the encoder Dense layers in MX-fp8 on the block-scaled fp8 MFMA (everything else
    bfloat16)."""
    if dropout is not None:
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout rate must be in [0, 1), got {dropout}")
        if training is True and float(dropout) > 0.0:
            raise ValueError("training=True applies dropout in every call (vtd.py:369, 405, "
                             "486); this forward path is inference-only")
    if input_shape is None:                                       # vtd.py:550-551
        input_shape = (*Constants.MODEL_IMAGE_SIZE.value, 3)
    kw = dict(input_shape=tuple(int(v) for v in input_shape), patch_size=int(patch_size),
              embedding_dim=int(embedding_dim), encoder_num_heads=int(encoder_num_heads),
              encoder_key_dim=int(encoder_key_dim), dropout=dropout,
              encoder_mlp_quantities=int(encoder_mlp_quantities),
              encoder_repeat_times=int(encoder_repeat_times),
              mlp_head_last_units=int(mlp_head_last_units),
              mlp_head_dense_layers_quantity=int(mlp_head_dense_layers_quantity),
              mlp_head_dense_mish_block_repeats=int(mlp_head_dense_mish_block_repeats),
              use_mish=bool(use_mish), max_weight=max_weight, clip_weight=clip_weight,
              training=training)
    return Model(kw, dtype=dtype, device=device, seed=seed)


def _to_device(inputs, what):
    """Stage a numpy array / CPU tensor / HIP tensor of shape (..., 6) on the HIP device.
    Returns (fp32 contiguous device tensor, back) where back(t) hands a result back in the
    caller's type: numpy in -> numpy out, CPU tensor in -> CPU tensor out.  There is no CPU
    decode path: without a HIP device this raises."""
    if torch.is_tensor(inputs):
        t, back = inputs, ((lambda r: r) if inputs.device.type == "cuda"
                           else (lambda r: r.cpu()))
    else:
        t, back = torch.as_tensor(np.asarray(inputs)), (lambda r: r.cpu().numpy())
    if t.shape[-1:] != (6,):
        raise ValueError(f"{what}: expected a (..., 6) input, got {tuple(t.shape)}")
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} runs on the HIP device and none is available")
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.to(torch.float32).contiguous(), back


class _Decode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src):
        src = src.detach()
        out = torch.empty_like(src)
        if src.numel():
            with torch.cuda.device(src.device):
                L.check(L.lib.vtd_decode(src.data_ptr(), src.numel() // 6, out.data_ptr(),
                                         L.stream_ptr()), "vtd_decode")
        ctx.save_for_backward(src)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        src, = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grad = torch.empty_like(src)
        with torch.cuda.device(src.device):
            L.check(L.lib.vtd_decode_grad(src.data_ptr(), g.data_ptr(), src.numel() // 6,
                                          grad.data_ptr(), L.stream_ptr()), "vtd_decode_grad")
        return grad


def transform_predictions(inputs):
    """vtd.py:586-647 on a (…, 6) tensor/array: sigmoid; clip the last 4 to [0, 1];
    [objectness, class * (CLASSES - 1), cx * W, cy * H, h * H, w * W] with (H, W) the
    constant MODEL_IMAGE_SIZE = (608, 608).  Decodes on the GPU (vtd_decode).  The
    reference's callers pass whatever `predict` returned (vtd.py:1164, 1341, 2447), so
    numpy / CPU inputs are staged to the device and the result comes back in the same
    type (numpy in, numpy out).  A tensor that requires grad gets a differentiable result
    (vtd_decode_grad: scale * s (1 - s) of the decode's own sigmoid)."""
    src, back = _to_device(inputs, "transform_predictions")
    if src.requires_grad and torch.is_grad_enabled():
        return back(_Decode.apply(src))
    out = torch.empty_like(src)
    n = src.numel() // 6
    if n:
        with torch.cuda.device(src.device):
            L.check(L.lib.vtd_decode(src.data_ptr(), n, out.data_ptr(), L.stream_ptr()),
                    "vtd_decode")
    return back(out)


def decode_detections(logits, objectness_threshold: float = 0.5,
                      classification_threshold: float = 0.5):
    """Device-side transform_predictions + thresholded detection test (vtd.py:586-647,
    1359-1384): category = round-half-even(class), confidence = (0.5 - |class -
    category|) / 0.5, valid = objectness > thr and confidence > thr.
    Returns (dets (..., 6) fp32, category (...) int32, valid (...) bool) in the caller's
    type (device tensors for a device input, numpy for numpy, CPU tensors for CPU)."""
    src, back = _to_device(logits, "decode_detections")
    n = src.numel() // 6
    dets = torch.empty_like(src)
    cat = torch.empty(src.shape[:-1], dtype=torch.int32, device=src.device)
    valid = torch.empty(src.shape[:-1], dtype=torch.uint8, device=src.device)
    if n:
        with torch.cuda.device(src.device):
            L.check(L.lib.vtd_decode_detections(src.data_ptr(), n, dets.data_ptr(),
                                                cat.data_ptr(), valid.data_ptr(),
                                                float(objectness_threshold),
                                                float(classification_threshold),
                                                L.stream_ptr()), "vtd_decode_detections")
    return back(dets), back(cat), back(valid.bool())


def detection_list(dets, category, valid):
    """Host-side list per image of the valid detections:
    [{"category": int, "objectness": float, "box_xywh": (cx, cy, w, h)}, ...]
    (box fields in MODEL_IMAGE_SIZE pixels, as transform_predictions returns them:
    [2] = cx, [3] = cy, [4] = height, [5] = width)."""
    d, c, v = dets.cpu().numpy(), category.cpu().numpy(), valid.cpu().numpy()
    out = []
    for b in range(d.shape[0]):
        items = []
        for k in np.nonzero(v[b])[0]:
            items.append({"slot": int(k), "category": int(c[b, k]),
                          "objectness": float(d[b, k, 0]),
                          "box_xywh": (float(d[b, k, 2]), float(d[b, k, 3]),
                                       float(d[b, k, 5]), float(d[b, k, 4]))})
        out.append(items)
    return out
