"""The yardstick of the dropout kernels, no GPU: a numpy restatement of the mask (Philox4x32-10,
the subkey, the 2 x 4 patch and the 16-bit keep decision of csrc/vtd_philox.h, DESIGN.md
"Dropout") and the float64 masked attention forward / backward.

  philox4x32_10            vectorised over arrays of counters
  mask_rows / mask_attention   bool [rows][N] / [B][H][N][N], True = kept
  forward64 / backward64   O = ((P o M) c) V and the gradients of sum(O * dO), c = inv_keep
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
DROP_TAG = 0x44524F50
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two python ints.  Returns four uint32 arrays."""
    c = [np.asarray(x, np.uint64) & U32 for x in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(rate):
    return min(int(float(rate) * 65536.0 + 0.5), 65535)


def inv_keep(rate):
    """fp32 of 1 / (1 - realised rate), computed in double."""
    return np.float32(1.0 / (1.0 - threshold(rate) / 65536.0))


def subkey(seed, step, site):
    w = philox4x32_10([np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32), np.uint32(site),
                       np.uint32(DROP_TAG)], (seed & 0xFFFFFFFF, seed >> 32))
    return int(w[0]), int(w[1])


def _lanes(words, di, dj):
    """The 16-bit lane of element (di, dj) of each 2 x 4 patch: word 2 di + (dj >> 1), low half
    for even dj."""
    w = np.stack(words, axis=0).astype(np.uint32)
    sel = np.take_along_axis(w, (2 * di + (dj >> 1))[None].astype(np.int64), axis=0)[0]
    return (sel >> (16 * (dj & 1)).astype(np.uint32)) & np.uint32(0xFFFF)


def mask_rows(rows, N, rate, seed, step=0, site=0, row0=0):
    """Elementwise site: bool [rows][N] of rows row0 .. row0 + rows - 1."""
    key = subkey(seed, step, site)
    m = (np.arange(rows, dtype=np.int64) + row0)[:, None]
    c = np.arange(N, dtype=np.int64)[None, :]
    pr = (m >> 1).astype(np.uint64)
    words = philox4x32_10([c >> 2, pr & U32, pr >> np.uint64(32), np.zeros_like(c)], key)
    di, dj = np.broadcast_arrays(m & 1, c & 3)
    return _lanes(words, di, dj) >= threshold(rate)


def mask_attention(B, H, N, rate, seed, step=0, site=0):
    """Attention site: bool [B][H][N][N] (image, head, query, key)."""
    key = subkey(seed, step, site)
    b = np.arange(B, dtype=np.int64)[:, None, None, None]
    h = np.arange(H, dtype=np.int64)[None, :, None, None]
    i = np.arange(N, dtype=np.int64)[None, None, :, None]
    j = np.arange(N, dtype=np.int64)[None, None, None, :]
    words = philox4x32_10([j >> 2, i >> 1, h, b], key)
    di, dj = np.broadcast_arrays(i & 1, j & 3)
    di, dj = np.broadcast_to(di, words[0].shape), np.broadcast_to(dj, words[0].shape)
    return _lanes(words, di, dj) >= threshold(rate)


# ------------------------------------------------------------------------------- float64
def forward64(q, k, v, scale, mask, c):
    """q, k, v [B][N][H][dk]; mask bool [B][H][N][N]; (O, lse, P): lse and P undropped."""
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * float(scale)
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    return np.einsum("bhqk,bkhd->bqhd", p * mask * float(c), v), (m + np.log(l))[..., 0], p


def backward64(q, k, v, do, scale, mask, c):
    """(dQ, dK, dV) of sum(O * dO) with dropout on the probabilities."""
    o, _, p = forward64(q, k, v, scale, mask, c)
    mc = mask * float(c)
    delta = np.einsum("bqhd,bqhd->bhq", do, o)
    dp = np.einsum("bqhd,bkhd->bhqk", do, v) * mc
    ds = p * (dp - delta[..., None]) * float(scale)
    return (np.einsum("bhqk,bkhd->bqhd", ds, k), np.einsum("bhqk,bqhd->bkhd", ds, q),
            np.einsum("bhqk,bqhd->bkhd", p * mc, do))


def magnitudes(q, k, v, do, scale, mask, c):
    """attention_grad_oracle.magnitudes with the mask: the single-key shape's denominators."""
    o, _, p = forward64(q, k, v, scale, mask, c)
    mc = mask * float(c)
    a = p * (np.einsum("bqhd,bkhd->bhqk", np.abs(do), np.abs(v)) * mc +
             np.einsum("bqhd,bqhd->bhq", np.abs(do), np.abs(o))[..., None]) * float(scale)
    return (np.einsum("bhqk,bkhd->bqhd", a, np.abs(k)), np.einsum("bhqk,bqhd->bkhd", a, np.abs(q)),
            np.einsum("bhqk,bqhd->bkhd", p * mc, np.abs(do)))


# ------------------------------------------------------------------------------- the block
def block_masks(case, rate, seed, step=0, site_base=0):
    """(attention mask [B][H][N][N], [mask [B][N][n_j] of MLP layer j]) of one encoder block:
    site_base the attention probabilities, site_base + 1 + j MLP layer j; an MLP activation is
    the [B N][n_j] matrix, row b N + t."""
    B, N, d, heads, dk, q, _ = case
    att = mask_attention(B, heads, N, rate, seed, step, site_base)
    mlp = [mask_rows(B * N, d << (q - 1 - j), rate, seed, step, site_base + 1 + j)
           .reshape(B, N, d << (q - 1 - j)) for j in range(q)]
    return att, mlp


def block_forward(w, x, use_mish, masks, c, taps=None):
    """tests/block_grad_oracle.block_forward with the reference's dropout (vtd.py:359-369,
    404-405): on the attention probabilities and after every MLP activation, the last one too."""
    import math

    import torch

    from tests import block_grad_oracle as K
    from tests import head_grad_oracle as H
    att, mlp = masks
    g1, b1, wq, bq, wk, bk, wv, bv, wo, bo, g2, b2 = w[:12]
    act = H.mish if use_mish else H.gelu_tanh
    dk = wq.shape[-1]
    h1 = K._ln64(x, g1, b1)
    q = torch.einsum("bnd,dhk->bnhk", h1, wq) + bq
    k = torch.einsum("bnd,dhk->bnhk", h1, wk) + bk
    v = torch.einsum("bnd,dhk->bnhk", h1, wv) + bv
    if taps is not None:
        k.retain_grad()
        taps.append(k)
    p = torch.softmax(torch.einsum("bqhk,bjhk->bhqj", q, k) / math.sqrt(dk), dim=-1)
    p = p * torch.tensor(att, dtype=x.dtype) * float(c)
    o = torch.einsum("bhqj,bjhk->bqhk", p, v)
    x1 = x + torch.einsum("bnhk,hkd->bnd", o, wo) + bo
    a = K._ln64(x1, g2, b2)
    for j in range((len(w) - 12) // 2):
        a = act(a @ w[12 + 2 * j] + w[13 + 2 * j]) * torch.tensor(mlp[j], dtype=x.dtype) * float(c)
    return x1 + a


def chain_grads(blocks, x, dy, use_mish, masks, c):
    """Blocks one after another with their masks: (y, [grads per block], dx, [den per block]) in
    float64, the denominators as tests/block_grad_oracle._denominators gives them."""
    import torch

    from tests import block_grad_oracle as K
    ws = [[torch.tensor(np.asarray(t), dtype=torch.float64, requires_grad=True) for t in w]
          for w in blocks]
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    y, taps = xt, []
    for w, m in zip(ws, masks):
        y = block_forward(w, y, use_mish, m, c, taps)
    (y * torch.tensor(np.asarray(dy), dtype=torch.float64)).sum().backward()
    grads, dx = [[t.grad.numpy() for t in w] for w in ws], xt.grad.numpy()
    return (y.detach().numpy(), grads, dx,
            [K._denominators(g, dx, k) for g, k in zip(grads, taps)])
