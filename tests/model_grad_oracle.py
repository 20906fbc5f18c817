"""The yardstick of Model.gradients and vtd_stem_backward: the whole model in torch float64 with
autograd from Keras-name keyed weights -- a float64 stem on the numpy oracle's patches,
block_grad_oracle.block_forward per encoder block, head_grad_oracle.head_forward -- and the CPU
emulation of the device's chain of roundings composed from what exists: head_grad_oracle.mm for
the stem's two products in the mode's operands, emulated_block_backward per block,
emulated_head_backward for the head.

The stem (vtd.py:271-307): x0[b, n, :] = patches[b, n, :] @ W + bias + pos[n, 0].

Bars of the end-to-end comparison (tests/test_gpu_model_gradients.py), per tensor, of max |g64|
(key/bias: of block_grad_oracle._denominators' magnitude).  The project's are BARS: 2e-4 bf16x3,
5e-2 bfloat16, with the rule that the emulation stays under half a bar.  Over a whole chain the
emulation of some tensors passes half of that -- the roundings of every later stage reach them
-- and each of those has a bar of its own, twice the emulation's worst over the four cases
(tests/test_model_grad_kat.py measures it and holds the table to it).  They are listed in
OWN_BARS by mode and Keras name, fixed before any GPU run.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import vtd_numpy as V
from tests import block_grad_oracle as K
from tests import head_grad_oracle as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BARS = H.BARS
CASES = [("tiny_mish", 3), ("tiny_gelu", 2), ("tiny_seq400", 2), ("multi_tile", 16)]
POS, WP, BP = ("position_encoding/position_embedding/embeddings", "linear_projection/kernel",
               "linear_projection/bias")

# mode -> Keras name -> bar: the tensors whose emulated whole-chain error passes half the
# project's bar in some case; the value is twice the emulation's worst over CASES, rounded up
# to two digits.  bf16x3: none -- the emulation's worst is 4.1e-5 (multi_head_attention/value/
# kernel at tiny_gelu).  bfloat16, both at tiny_gelu (the deepest head, 10 Dense layers, above
# two blocks): the first block's LayerNorm beta 3.46e-2 and query bias 2.50e-2 (a hair over
# half of 5e-2).
OWN_BARS = {
    "bf16x3": {},
    "bfloat16": {"layer_normalization/beta": 7.0e-2,
                 "multi_head_attention/query/bias": 5.1e-2},
}


def bar(mode, name):
    return OWN_BARS[mode].get(name, BARS[mode])


def load_case(name, batch):
    """(kwargs, weights, images (B, H, W, C) float32, dlogits (B, 17, 6) float32): the
    configurations of tests/test_gpu_head_backward.py, a seeded stand-in for the loss gradient."""
    if name == "multi_tile":
        kw = dict(H.MULTI_TILE)
        w = V.init_weights(seed=11, **kw)
        x = V.synthetic_images(batch, kw["input_shape"], seed=12)
    else:
        z = np.load(os.path.join(GOLD, f"{name}.npz"))
        kw = json.loads(str(z["kwargs"]))
        kw["input_shape"] = tuple(kw["input_shape"])
        w = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        x = V.synthetic_images(batch, kw["input_shape"], seed=21)
    rng = np.random.default_rng(len(name) + batch)
    dlogits = (rng.normal(0.0, 1.0, (batch, 17, 6)) / (batch * 17)).astype(np.float32)
    return kw, w, np.asarray(x, np.float32), dlogits


def split_names(kw):
    """(stem names, [block names], head names) in Keras creation order."""
    k = V.resolve_kwargs(**kw)
    names = list(V.weight_shapes(**kw))
    per = 12 + 2 * k["encoder_mlp_quantities"]
    reps = k["encoder_repeat_times"]
    return (names[:3], [names[3 + i * per: 3 + (i + 1) * per] for i in range(reps)],
            names[3 + reps * per:])


def patches_of(images, p):
    """(B, N, p p C) float64: tf.image.extract_patches(SAME) + Reshape, the numpy oracle's."""
    return V.extract_patches_same(np.asarray(images, np.float64), p)


# ------------------------------------------------------------------ float64
def stem_forward(sw, patches):
    """x0 (B, N, d) from the patches and [pos (N, 1), W, b] (torch tensors of one dtype)."""
    pos, w, b = sw
    return patches @ w + b + pos                                           # vtd.py:297-307


def stem_grads(sw, images, p, dx0):
    """(x0, [dpos, dW, db]) in float64 by autograd, dx0 = d loss / d x0."""
    t = [torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in sw]
    x0 = stem_forward(t, torch.tensor(patches_of(images, p)))
    (x0 * torch.tensor(np.asarray(dx0), dtype=torch.float64)).sum().backward()
    return x0.detach().numpy(), [a.grad.numpy() for a in t]


def model_forward(kw, wt, patches, taps=None, inputs=None):
    """logits (B, 17, 6) of the whole model; wt: name -> torch tensor.  taps: every block's key
    tensor is appended (block_forward); inputs: every block input x_0 .. x_L is appended with
    its gradient retained."""
    k = V.resolve_kwargs(**kw)
    stem, blocks, head = split_names(kw)
    x = stem_forward([wt[n] for n in stem], patches)
    for names in blocks:
        if inputs is not None:
            x.retain_grad()
            inputs.append(x)
        x = K.block_forward([wt[n] for n in names], x, k["use_mish"], taps)
    if inputs is not None:
        x.retain_grad()
        inputs.append(x)
    return H.head_forward(OrderedDict((n, wt[n]) for n in head), x, k["use_mish"])


def model_grads(kw, weights, images, dlogits):
    """(logits, grads, dxs, den) in float64 by autograd from d loss / d logits: grads an
    OrderedDict name -> gradient in Keras creation order, dxs the gradients of the block inputs
    x_0 .. x_L, den name -> the denominator of the error measure (max |g64|; key/bias: the
    magnitude block_grad_oracle._denominators explains)."""
    k = V.resolve_kwargs(**kw)
    stem, blocks, head = split_names(kw)
    wt = OrderedDict((n, torch.tensor(np.asarray(weights[n]), dtype=torch.float64,
                                      requires_grad=True)) for n in stem + sum(blocks, []) + head)
    taps, inputs = [], []
    logits = model_forward(kw, wt, torch.tensor(patches_of(images, k["patch_size"])), taps, inputs)
    (logits * torch.tensor(np.asarray(dlogits), dtype=torch.float64)).sum().backward()
    grads = OrderedDict((n, t.grad.numpy()) for n, t in wt.items())
    den = OrderedDict((n, float(np.abs(g).max())) for n, g in grads.items())
    for names, key in zip(blocks, taps):
        den[names[K.KEY_BIAS]] = float(np.abs(key.grad.numpy()).sum(axis=(0, 1)).max())
    return logits.detach().numpy(), grads, [t.grad.numpy() for t in inputs], den


# ------------------------------------------------------------------ emulation
def _t32(a):
    return torch.tensor(np.asarray(a, np.float32))


def emulated_stem_forward(sw, images, p, mode):
    """x0 float32 (B, N, d): the GEMM on the mode's operands, then + bias, then + pos, each one
    float32 add (the epilogue's order)."""
    pos, w, b = (_t32(a) for a in sw)
    pt = _t32(patches_of(images, p))
    B, N, P = pt.shape
    x0 = (H.mm(pt.reshape(B * N, P), w, mode) + b).reshape(B, N, -1) + pos
    return x0.numpy()


def emulated_stem_backward(images, p, dx0, mode):
    """[dpos, dW, db] float32: dW on the mode's operands, db the sum of the stored operand, dpos
    the float32 sum of dx0 over the row, then over the batch."""
    pt = _t32(patches_of(images, p))
    B, N, P = pt.shape
    g = _t32(dx0).reshape(B * N, -1)
    dw = H.mm(pt.reshape(B * N, P).T, g, mode).numpy()
    db = H.stored(g, mode).sum(0).float().numpy()
    dpos = np.asarray(dx0, np.float32).sum(axis=2, dtype=np.float32).sum(axis=0, dtype=np.float32)
    return [dpos.reshape(N, 1), dw, db]


def emulated_model_backward(kw, weights, images, dlogits, mode):
    """The device's whole chain on the CPU, stage by stage as Model.gradients runs it: returns
    (logits, grads) float32 as model_grads does."""
    k = V.resolve_kwargs(**kw)
    stem, blocks, head = split_names(kw)
    heads, dk, use_mish = k["encoder_num_heads"], k["encoder_key_dim"], k["use_mish"]
    sw = [weights[n] for n in stem]
    xs = [emulated_stem_forward(sw, images, k["patch_size"], mode)]
    for names in blocks:
        bw = [weights[n] for n in names]
        y, _, _ = K.emulated_block_backward(bw, xs[-1], np.zeros_like(xs[-1]), heads, dk,
                                            use_mish, mode)
        xs.append(y)
    logits, hg = H.emulated_head_backward(weights, xs[-1], dlogits, use_mish, mode)
    grads = {n: hg[n] for n in head}
    dy = hg["encoded_images"]
    for i in range(len(blocks) - 1, -1, -1):
        bw = [weights[n] for n in blocks[i]]
        _, g, dy = K.emulated_block_backward(bw, xs[i], dy, heads, dk, use_mish, mode)
        grads.update(zip(blocks[i], g))
    grads.update(zip(stem, emulated_stem_backward(images, k["patch_size"], dy, mode)))
    return logits, OrderedDict((n, grads[n]) for n in stem + sum(blocks, []) + head)


def rel_errors(grads, grads64, den):
    """{name: max |g - g64| / den[name]}."""
    return {n: float(np.abs(np.asarray(grads[n], np.float64) - grads64[n]).max() / den[n])
            for n in grads64}


# ------------------------------------------------------------------ the stem alone
# (B, H, W, p, d) of tests/test_gpu_stem_backward.py, C = 3
STEM_CASES = [(3, 40, 36, 8, 24), (2, 33, 50, 7, 20), (2, 80, 80, 4, 32), (16, 64, 64, 4, 64),
              (2, 48, 32, 16, 768), (3, 20, 12, 4, 6)]


def stem_case_id(c):
    return "B{}_{}x{}_p{}_d{}".format(*c)


def seeded_stem(case, seed=0):
    """(images, [pos, W, b], dx0) float32: images U(0, 1), the Keras initialisers' scales with a
    non-zero bias, dx0 ~ N(0, 1)."""
    B, Hh, Ww, p, d = case
    rng = np.random.default_rng([B, Hh, Ww, p, d, seed])
    gh, gw = V.token_grid(Hh, Ww, p)
    N, P = gh * gw, p * p * 3
    images = rng.uniform(0.0, 1.0, (B, Hh, Ww, 3)).astype(np.float32)
    lim = np.sqrt(6.0 / (P + d))
    sw = [rng.uniform(-0.05, 0.05, (N, 1)).astype(np.float32),
          rng.uniform(-lim, lim, (P, d)).astype(np.float32),
          (0.05 * rng.standard_normal(d)).astype(np.float32)]
    dx0 = rng.standard_normal((B, N, d)).astype(np.float32)
    return images, sw, dx0


def dpos_roundings(B, d):
    """c of the dpos bound c 2^-24 sum_b sum_j |dx0| (DESIGN.md "Whole-model gradients"): the
    adds a value passes through in the kernels as written -- 8 ceil(d_p / 512) in its lane
    (d_p = d rounded up to 64), 6 wave steps, B batch adds."""
    dp = -(-d // 64) * 64
    return 8 * -(-dp // 512) + 6 + B
