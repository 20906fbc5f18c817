"""The yardstick of vtd_encoder_block_backward: one encoder block (vtd.py:350-412 with
dropout=None) in torch float64 with autograd from Keras-layout weights, and a CPU emulation of
the device's roundings composed from what exists -- head_grad_oracle.mm / stored for the Dense
products, attention_grad_oracle.emulate for the attention core, ln_grad_oracle.emulate for the
LayerNorm gradients, float32 elsewhere.

The block: h1 = LN(x); q, k, v = h1 Wq + bq, ... per head; O = softmax(q k^T / sqrt(key_dim)) v;
x1 = x + O Wo + bo; h2 = LN(x1); a_j = act(a_{j-1} W_j + b_j), a_{-1} = h2; y = x1 + a_{q-1}.
LayerNormalization epsilon 1e-3 (vtd.py:352).  A block's weights are a list in Keras creation
order: ln1 gamma, beta; query, key, value kernel (d, H, dk) and bias (H, dk); attention_output
kernel (H, dk, d) and bias (d,); ln2 gamma, beta; the MLP kernel / bias pairs.
"""
import math

import numpy as np
import torch

from tests import attention_grad_oracle as A
from tests import head_grad_oracle as H
from tests import ln_grad_oracle as LN

EPS = 1e-3
BARS = H.BARS
ATT_MODE = {"bf16x3": "x3", "bfloat16": "bf16"}

# (B, N, d, heads, key_dim, q, use_mish): the smallest shapes at which each branch of the chain
# can still go wrong (tests/test_gpu_encoder_block.py says which)
CASES = [(1, 3, 8, 1, 4, 1, True), (3, 25, 24, 3, 10, 3, True), (2, 40, 20, 2, 12, 2, False),
         (2, 400, 32, 3, 16, 2, True), (16, 256, 64, 2, 32, 2, True),
         (2, 77, 768, 12, 64, 3, False)]
TINY_MISH, TINY_GELU = CASES[1], CASES[2]


def case_id(c):
    return "B{}_N{}_d{}_h{}x{}_q{}_{}".format(*c[:6], "mish" if c[6] else "gelu")


def names(q):
    out = ["ln1/gamma", "ln1/beta"]
    for part in ("query", "key", "value", "attention_output"):
        out += [f"{part}/kernel", f"{part}/bias"]
    out += ["ln2/gamma", "ln2/beta"]
    for j in range(q):
        out += [f"mlp_{j + 1}/kernel", f"mlp_{j + 1}/bias"]
    return out


def shapes(d, heads, dk, q):
    out = [(d,), (d,)] + [(d, heads, dk), (heads, dk)] * 3 + [(heads, dk, d), (d,), (d,), (d,)]
    k = d
    for j in range(q):
        n = d << (q - 1 - j)
        out += [(k, n), (n,)]
        k = n
    return out


def seeded_weights(case, seed=0):
    """float32 arrays in creation order: glorot-uniform kernels (Keras's fans: the receptive
    field times the last two axes), biases 0.05 N(0, 1), gamma 1 + 0.1 N(0, 1), beta 0.1 N(0, 1)."""
    B, N, d, heads, dk, q, _ = case
    rng = np.random.default_rng([d, heads, dk, q, seed])
    out = []
    for name, shape in zip(names(q), shapes(d, heads, dk, q)):
        if name.endswith("/kernel"):
            rf = int(np.prod(shape[:-2]))
            lim = math.sqrt(6.0 / ((shape[-2] + shape[-1]) * rf))
            t = rng.uniform(-lim, lim, shape)
        elif name.endswith("/gamma"):
            t = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/beta"):
            t = 0.1 * rng.standard_normal(shape)
        else:
            t = 0.05 * rng.standard_normal(shape)
        out.append(t.astype(np.float32))
    return out


def seeded_inputs(case, seed=0):
    """x, dy ~ N(0, 1), float32 (B, N, d)."""
    B, N, d = case[:3]
    rng = np.random.default_rng([B, N, d, 99, seed])
    return (rng.standard_normal((B, N, d)).astype(np.float32),
            rng.standard_normal((B, N, d)).astype(np.float32))


# ------------------------------------------------------------------ float64
def _ln64(x, gamma, beta):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * gamma + beta


def block_forward(w, x, use_mish, taps=None):
    """y (B, N, d) from x and the block's weights (torch tensors of one dtype).  taps (a list):
    the key tensor (B, N, H, dk) is appended, with its gradient retained."""
    g1, b1, wq, bq, wk, bk, wv, bv, wo, bo, g2, b2 = w[:12]
    act = H.mish if use_mish else H.gelu_tanh
    dk = wq.shape[-1]
    h1 = _ln64(x, g1, b1)                                                  # vtd.py:352
    q = torch.einsum("bnd,dhk->bnhk", h1, wq) + bq                         # vtd.py:356-362
    k = torch.einsum("bnd,dhk->bnhk", h1, wk) + bk
    v = torch.einsum("bnd,dhk->bnhk", h1, wv) + bv
    if taps is not None:
        k.retain_grad()
        taps.append(k)
    p = torch.softmax(torch.einsum("bqhk,bjhk->bhqj", q, k) / math.sqrt(dk), dim=-1)
    o = torch.einsum("bhqj,bjhk->bqhk", p, v)
    x1 = x + torch.einsum("bnhk,hkd->bnd", o, wo) + bo                     # vtd.py:366
    a = _ln64(x1, g2, b2)                                                  # vtd.py:369
    for j in range((len(w) - 12) // 2):                                    # vtd.py:385-403
        a = act(a @ w[12 + 2 * j] + w[13 + 2 * j])
    return x1 + a                                                          # vtd.py:408


KEY_BIAS = 5          # index of key/bias in a block's weight list


def _denominators(grads, dx, k):
    """max |g64| per tensor and for x -- except key/bias.  Adding one vector to every key shifts
    all scores of a query by the same amount, which softmax ignores: d loss / d key bias is zero
    for every input, a complete cancellation of sum_rows dK, and max |g64| is rounding noise
    (1e-16).  As for the single-key case of tests/attention_grad_oracle.tensor_errors, the error
    is taken there against the largest magnitude of the cancelling terms, max sum_rows |dK64|:
    what a rounding of them can leave behind."""
    den = [float(np.abs(g).max()) for g in grads] + [float(np.abs(dx).max())]
    dk = k.grad.numpy()
    den[KEY_BIAS] = float(np.abs(dk).sum(axis=(0, 1)).max())
    return den


def block_grads(weights, x, dy, use_mish):
    """(y, grads, dx, den) in float64 by autograd; grads a list in the weights' order, den the
    measure's denominators (_denominators) for grads + [dx]."""
    w = [torch.tensor(np.asarray(t), dtype=torch.float64, requires_grad=True) for t in weights]
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    taps = []
    y = block_forward(w, xt, use_mish, taps)
    (y * torch.tensor(np.asarray(dy), dtype=torch.float64)).sum().backward()
    grads, dx = [t.grad.numpy() for t in w], xt.grad.numpy()
    return y.detach().numpy(), grads, dx, _denominators(grads, dx, taps[0])


def chain_grads(blocks, x, dy, use_mish):
    """Several blocks one after another: (y, [grads per block], dx, [den per block]) in float64
    (each den as block_grads gives it; its last entry is for the chain's dx)."""
    ws = [[torch.tensor(np.asarray(t), dtype=torch.float64, requires_grad=True) for t in w]
          for w in blocks]
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    y, taps = xt, []
    for w in ws:
        y = block_forward(w, y, use_mish, taps)
    (y * torch.tensor(np.asarray(dy), dtype=torch.float64)).sum().backward()
    grads, dx = [[t.grad.numpy() for t in w] for w in ws], xt.grad.numpy()
    return (y.detach().numpy(), grads, dx,
            [_denominators(g, dx, k) for g, k in zip(grads, taps)])


# ------------------------------------------------------------------ emulation
def _t32(a):
    return torch.tensor(np.asarray(a, np.float32))


def _ln32(x, stat, gamma, beta):
    """LayerNorm forward in float32 from the (mean, rstd) pairs."""
    f = np.float32
    xh = ((x - stat[:, :1]).astype(f) * stat[:, 1:2]).astype(f)
    return ((xh * gamma[None, :]).astype(f) + beta[None, :]).astype(f)


def emulated_block_backward(weights, x, dy, heads, dk, use_mish, mode):
    """The device's algorithm on the CPU, step by step as vtd_encoder_block_backward runs it:
    returns (y, grads, dx) float32 as block_grads does."""
    amode = ATT_MODE[mode]
    g1, b1, wq, bq, wk, bk, wv, bv, wo, bo, g2, b2 = [np.asarray(t, np.float32)
                                                      for t in weights[:12]]
    mlp = [np.asarray(t, np.float32) for t in weights[12:]]
    q_layers = len(mlp) // 2
    act = H.mish if use_mish else H.gelu_tanh
    x = np.asarray(x, np.float32)
    B, N, d = x.shape
    R, inner = B * N, heads * dk
    x2, dy2 = x.reshape(R, d), np.asarray(dy, np.float32).reshape(R, d)
    path = LN.route(d, lds=(d,))
    scale = 1.0 / math.sqrt(dk)

    # ---- training forward
    stat1 = LN.stats_fp32(x2)
    h1 = _t32(_ln32(x2, stat1, g1, b1))
    wqkv = _t32(np.concatenate([t.reshape(d, inner) for t in (wq, wk, wv)], axis=1))
    bqkv = _t32(np.concatenate([t.reshape(inner) for t in (bq, bk, bv)]))
    qkv = H.mm(h1, wqkv, mode) + bqkv
    if mode == "bfloat16":
        qkv = H.bf16(qkv)                                   # what the bf16 attention reads
    qn, kn, vn = (qkv[:, i * inner:(i + 1) * inner].reshape(B, N, heads, dk).double().numpy()
                  for i in range(3))
    fwd = A.emulate(qn, kn, vn, np.zeros_like(qn), scale, amode)
    o2 = _t32(fwd["o"].reshape(R, inner))
    wo2 = _t32(wo.reshape(inner, d))
    x1 = (_t32(x2) + (H.mm(o2, wo2, mode) + _t32(bo))).numpy()
    stat2 = LN.stats_fp32(x1)
    a = [_t32(_ln32(x1, stat2, g2, b2))]
    zs = []
    for j in range(q_layers):
        z = H.mm(a[-1], _t32(mlp[2 * j]), mode) + _t32(mlp[2 * j + 1])
        zs.append(z)
        a.append(act(z.double()).float())
    y = (_t32(x1) + a[-1]).numpy().reshape(B, N, d)

    # ---- backward
    grads = [None] * len(weights)
    g = _t32(dy2)
    for j in range(q_layers - 1, -1, -1):
        gz = g * H.act_grad64(zs[j], use_mish).float()
        grads[12 + 2 * j] = H.mm(a[j].T, gz, mode).numpy()
        grads[13 + 2 * j] = H.stored(gz, mode).sum(0).float().numpy()
        g = H.mm(gz, _t32(mlp[2 * j]).T, mode)
    dx1, grads[10], grads[11] = LN.emulate(x1, stat2, g2, g.numpy(), add=dy2, path=path)
    G = _t32(dx1)
    grads[8] = H.mm(o2.T, G, mode).numpy().reshape(heads, dk, d)
    grads[9] = H.stored(G, mode).sum(0).float().numpy()
    dO = H.mm(G, wo2.T, mode)
    if mode == "bfloat16":
        dO = H.bf16(dO)
    bwd = A.emulate(qn, kn, vn, dO.reshape(B, N, heads, dk).double().numpy(), scale, amode)
    dqkv = _t32(np.concatenate([bwd[n].reshape(R, inner) for n in ("dq", "dk", "dv")], axis=1))
    dw = H.mm(h1.T, dqkv, mode).numpy()
    db = H.stored(dqkv, mode).sum(0).float().numpy()
    for i in range(3):
        grads[2 + 2 * i] = dw[:, i * inner:(i + 1) * inner].reshape(d, heads, dk)
        grads[3 + 2 * i] = db[i * inner:(i + 1) * inner].reshape(heads, dk)
    dh1 = H.mm(dqkv, wqkv.T, mode).numpy()
    dx, grads[0], grads[1] = LN.emulate(x2, stat1, g1, dh1, add=dx1, path=path)
    return y, grads, dx.reshape(B, N, d)


def rel_errors(grads, dx, grads64, dx64, den, q):
    """{name: max |g - g64| / den} for every weight gradient and "x": den = max |g64|, for
    key/bias the magnitude _denominators explains."""
    out = {}
    for n, g, r, d in zip(names(q) + ["x"], list(grads) + [dx], list(grads64) + [dx64], den):
        out[n] = float(np.abs(np.asarray(g, np.float64) - r).max() / d)
    return out
