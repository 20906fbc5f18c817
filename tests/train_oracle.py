"""The yardsticks of vtd_train_step and vtd_fold_layernorm_batch (not a test), in numpy:

sparse32 / sparse64: Adam in the operation order of Keras's sparse path, which an Embedding's
gradient takes (the position embedding; every index occurs once, so it is a dense update) --
restated from Keras 2.9's optimizer_v2/adam.py `_resource_apply_sparse` from memory, TensorFlow
being unavailable here:
    m = m beta1 + g (1 - beta1);  v = v beta2 + (g g)(1 - beta2);  w = w - (alpha m) / (sqrt(v) + eps)
with g clipped by `clipvalue` first and the dense rule's alpha (tests/adam_oracle.py alpha64).
sparse32 rounds once per operation in float32, in the kernel's order (the kernel must match it
bit for bit); sparse64 is the same in float64.  No constraint unless asked: the reference leaves
the position embedding without ClipWeight.

packed_rows / grouped_pack: vtd_pack_dense's map and the bytes of a grouped destination in each
format.  grouped_vector: vtd_pack_vector's.  fold: vtd_fold_layernorm's outputs.
"""
import numpy as np

from tests import adam_oracle as A


def _sparse(dtype, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight, constrain):
    if t < 1:
        raise ValueError("t starts at 1")
    w, m, v, g = (np.asarray(a, dtype) for a in (w, m, v, g))
    one = dtype(1.0)
    b1, b2, eps = dtype(np.float32(beta_1)), dtype(np.float32(beta_2)), dtype(np.float32(epsilon))
    alpha = dtype(A.alpha64(t, lr, beta_1, beta_2))
    with np.errstate(all="ignore"):
        if clipvalue is not None and clipvalue > 0:
            g = A._clip(g, np.float32(clipvalue))
        m = m * b1 + g * (one - b1)
        v = v * b2 + (g * g) * (one - b2)
        w = w - (alpha * m) / (np.sqrt(v) + eps)
        if constrain:
            w = A._clip(np.where(np.isnan(w), one, w), np.float32(max_weight))
    assert w.dtype == m.dtype == v.dtype == dtype
    return w, m, v


def sparse32(w, m, v, g, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipvalue=None,
             max_weight=10.0, constrain=False):
    return _sparse(np.float32, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight,
                   constrain)


def sparse64(w, m, v, g, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipvalue=None,
             max_weight=10.0, constrain=False):
    return _sparse(np.float64, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight,
                   constrain)


POS = "position_encoding/position_embedding/embeddings"


def host_step(name, w, m, v, g, t, lr, f32=True, clipvalue=10.0, max_weight=10.0, constrain=True):
    """One tensor's step as Model.train_on_batch takes it: the sparse-order rule without the
    constraint for the position embedding, tests/adam_oracle.py's dense rule with ClipWeight for
    everything else."""
    if name == POS:
        rule, constrain = (sparse32 if f32 else sparse64), False
    else:
        rule = A.step32 if f32 else A.step64
    return rule(w, m, v, g, t, lr, clipvalue=clipvalue, max_weight=max_weight, constrain=constrain)


def model_trajectory(kw, weights, images, y_true, steps, lr, f32=False):
    """The losses of `steps` whole-model Adam steps on one batch, before each update: the torch
    model of tests/model_grad_oracle.py with autograd, the loss of tests/loss_grad_oracle.py at
    its logits, host_step per tensor.  f32=False: everything in float64 (the yardstick).
    f32=True: float32 weights, float32 autograd and step32 -- an fp32 CPU port, to show what
    deviation from the float64 trajectory fp32 arithmetic alone brings."""
    from collections import OrderedDict

    import torch

    from oracle import vtd_numpy as V
    from tests import loss_grad_oracle as G
    from tests import model_grad_oracle as M
    tdt, ndt = (torch.float32, np.float32) if f32 else (torch.float64, np.float64)
    stem, blocks, head = M.split_names(kw)
    names = stem + sum(blocks, []) + head
    patches = torch.tensor(M.patches_of(images, V.resolve_kwargs(**kw)["patch_size"])).to(tdt)
    cur = {n: np.asarray(weights[n], ndt) for n in names}
    m = {n: np.zeros_like(cur[n]) for n in names}
    v = {n: np.zeros_like(cur[n]) for n in names}
    losses = []
    for t in range(1, steps + 1):
        wt = OrderedDict((n, torch.tensor(cur[n], dtype=tdt, requires_grad=True)) for n in names)
        logits = M.model_forward(kw, wt, patches)
        values, dlogits = G.loss_and_grad(y_true, logits.detach().double().numpy())
        losses.append(values[3])
        (logits * torch.tensor(dlogits, dtype=tdt)).sum().backward()
        for n in names:
            cur[n], m[n], v[n] = host_step(n, cur[n], m[n], v[n], wt[n].grad.numpy(), t, lr,
                                           f32=f32)
    return losses


# ------------------------------------------------------------------ grouped destinations
def grouped_index(i, group, group_p):
    """vtd_pack_dense's / vtd_pack_vector's map of one axis: (i / group) group_p + i % group."""
    i = np.asarray(i)
    return (i // group) * group_p + i % group


def grouped_pack(w, fmt, rows, k_p, k_group=None, k_group_p=None, n_group=None, n_group_p=None,
                 row_offset=0, fill=None):
    """The destination of a matrix w [K][N] after the step: an array of `rows` packed rows in
    format `fmt` -- 'f32' float32 [rows][k_p], 'bf16' uint16 [rows][k_p], 'bf16x3' uint16
    [rows][3 k_p] = [hi | hi | lo].  The row of every real n holds the whole piece(s): the real
    k at their packed columns, zeros elsewhere; every other row keeps `fill` (an array of the
    destination's shape and dtype: what was there before; None = zeros)."""
    w = np.asarray(w, np.float32)
    K, N = w.shape
    kg, ng = k_group or K, n_group or N
    kgp, ngp = k_group_p or k_p, n_group_p or N
    assert K % kg == 0 and N % ng == 0
    cols = grouped_index(np.arange(K), kg, kgp)
    prow = row_offset + grouped_index(np.arange(N), ng, ngp)
    assert cols.max() < k_p and prow.max() < rows
    piece = np.zeros((N, k_p), np.float32)
    piece[:, cols] = w.T
    if fmt == "f32":
        out = np.zeros((rows, k_p), np.float32) if fill is None else np.array(fill, np.float32)
        out[prow] = piece
        return out
    hi, lo = A.split(piece)
    pieces = {"bf16": [hi], "bf16x3": [hi, hi, lo]}[fmt]
    out = (np.zeros((rows, len(pieces) * k_p), np.uint16) if fill is None
           else np.array(fill, np.uint16))
    out[prow] = np.concatenate(pieces, axis=1)
    return out


def grouped_vector(w, size, n_group=None, n_group_p=None, offset=0, fill=None):
    """The fp32 destination of a vector w [N]: element n at offset + (n / n_group) n_group_p +
    n % n_group; everything else keeps `fill` (None = zeros)."""
    w = np.asarray(w, np.float32).reshape(-1)
    N = w.size
    ng, ngp = n_group or N, n_group_p or N
    out = np.zeros(size, np.float32) if fill is None else np.array(fill, np.float32)
    at = offset + grouped_index(np.arange(N), ng, ngp)
    assert at.max() < size
    out[at] = w
    return out


# ------------------------------------------------------------------ the LayerNorm fold
def fold(w32, gamma, beta, bias_in, fmt="bf16"):
    """vtd_fold_layernorm on a packed fp32 operand w32 [N_p][K_p] (K = ldw = ldo = K_p):
    (W' = round(W * gamma) as uint16 bf16 bits ('bf16') or float32 ('f32'), bias' = float32(bias
    + sum_k W beta) and colsum = float32(sum_k W') with the sums in float64 (W' the rounded
    stored value)).  The float64 sums run here in numpy's order; the kernel's is lane-strided
    with a butterfly, so the two agree bit for bit where the sums are exact in float64 -- the
    designed tests use such values -- and to an ulp of float32 otherwise."""
    w32 = np.asarray(w32, np.float32)
    gamma, beta = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    prod = w32 * gamma[None, :]
    assert prod.dtype == np.float32
    if fmt == "bf16":
        wo = A.bf16_bits(prod)
        stored = A.bf16_value(wo)
    else:
        wo = stored = prod
    bias = np.zeros(w32.shape[0], np.float32) if bias_in is None else np.asarray(bias_in, np.float32)
    sb = (w32.astype(np.float64) * beta.astype(np.float64)[None, :]).sum(axis=1)
    bias_out = (bias.astype(np.float64) + sb).astype(np.float32)
    colsum = stored.astype(np.float64).sum(axis=1).astype(np.float32)
    return wo, bias_out, colsum
