"""The yardstick of dropout at model level, no GPU: the masks of a whole model's dropout sites
(tests/dropout_oracle.py's mask_rows / block_masks at the site numbering of DESIGN.md "Dropout",
"Head and Model"), the float64 detection head with a Dropout after every Dense + activation
(mlp_head, vtd.py:468-486), and the float64 whole model built from model_grad_oracle.stem_forward,
dropout_oracle.block_forward and that head.

Sites, q = encoder_mlp_quantities, L = encoder_repeat_times: block i takes site_base i (1 + q)
(its attention probabilities, then its q MLP layers); head layer j, 0-based over all n_head
Dense + activation layers, takes L (1 + q) + j.  A head mask is the elementwise site over the
unpadded [B 17][units_j] activation, row b 17 + r.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import vtd_numpy as V
from tests import dropout_oracle as D
from tests import head_grad_oracle as H
from tests import loss_oracle as O
from tests import model_grad_oracle as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_DETECT = H.MAX_DETECT
# (name, batch): three of the existing cases and ragged_head, whose head units 24 / 12 / 6 are
# not all multiples of the mask's 4-column patch and whose 51 rows are odd against its 2 rows
CASES = [("tiny_mish", 3), ("tiny_gelu", 2), ("multi_tile", 16), ("ragged_head", 3)]
RATES = (0.5, 0.1)
SEED = 1234                       # the seed the GPU tests compile; OTHER_SEED where two are needed
OTHER_SEED = 0xFEEDFACE12345678
STEPS = (0, 1, 2)                 # the steps the GPU tests take


def load_case(name, batch):
    """(kwargs, weights, images, y_true) as tests/test_gpu_head_backward.load_case returns them;
    ragged_head: tiny_mish's kwargs with mlp_head_last_units=6, seeded weights."""
    if name == "multi_tile":
        kw = dict(H.MULTI_TILE)
        w = V.init_weights(seed=11, **kw)
        x = V.synthetic_images(batch, kw["input_shape"], seed=12)
    else:
        z = np.load(os.path.join(GOLD, f"{'tiny_mish' if name == 'ragged_head' else name}.npz"))
        kw = json.loads(str(z["kwargs"]))
        kw["input_shape"] = tuple(kw["input_shape"])
        if name == "ragged_head":
            kw["mlp_head_last_units"] = 6
            w = V.init_weights(seed=31, **kw)
        else:
            w = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        x = V.synthetic_images(batch, kw["input_shape"], seed=21)
    rng = np.random.default_rng(batch)
    y, _ = O.random_loss_batch(rng, batch, 17)
    return kw, w, np.asarray(x, np.float32), np.asarray(y, np.float32)


def shape_of(kw):
    """(tokens N, d, heads, key_dim, q, L, use_mish, [head units])."""
    k = V.resolve_kwargs(**kw)
    shapes = V.weight_shapes(**kw)
    units, j = [], 1
    while f"dense_{j}/bias" in shapes:
        units.append(int(shapes[f"dense_{j}/bias"][0]))
        j += 1
    return (int(shapes[M.POS][0]), k["embedding_dim"], k["encoder_num_heads"],
            k["encoder_key_dim"], k["encoder_mlp_quantities"], k["encoder_repeat_times"],
            bool(k["use_mish"]), units)


def head_site_base(kw):
    _, _, _, _, q, L, _, _ = shape_of(kw)
    return L * (1 + q)


def head_masks(kw, B, rate, seed, step, site_base=None):
    """[bool (B, 17, units_j)] per head layer j: mask_rows over [B 17][units_j] at site
    site_base + j (default site_base: L (1 + q))."""
    units = shape_of(kw)[7]
    base = head_site_base(kw) if site_base is None else site_base
    return [D.mask_rows(B * MAX_DETECT, u, rate, seed, step, base + j).reshape(B, MAX_DETECT, u)
            for j, u in enumerate(units)]


def model_masks(kw, B, rate, seed, step):
    """([block_masks of block i at site_base i (1 + q)], head_masks)."""
    N, d, heads, dk, q, L, use_mish, _ = shape_of(kw)
    case = (B, N, d, heads, dk, q, use_mish)
    return ([D.block_masks(case, rate, seed, step, i * (1 + q)) for i in range(L)],
            head_masks(kw, B, rate, seed, step))


def ones_like_masks(masks):
    blocks, head = masks
    return ([(np.ones_like(a), [np.ones_like(m) for m in mlp]) for a, mlp in blocks],
            [np.ones_like(m) for m in head])


def sites(kw):
    """Every dropout site of a model in call order."""
    _, _, _, _, q, L, _, units = shape_of(kw)
    out = []
    for i in range(L):
        out += [i * (1 + q) + t for t in range(1 + q)]
    return out + [L * (1 + q) + j for j in range(len(units))]


# ------------------------------------------------------------------ float64
def head_forward(hw, encoded, use_mish, masks, c):
    """head_grad_oracle.head_forward with act(...) * mask * inv_keep after every hidden layer."""
    act = H.mish if use_mish else H.gelu_tanh
    names = [n[:-len("/kernel")] for n in hw if n.endswith("/kernel")]
    x = encoded @ hw["dense/kernel"] + hw["dense/bias"]
    x = x.reshape(x.shape[0], MAX_DETECT, -1)
    assert len(masks) == len(names) - 2
    for n, m in zip(names[1:-1], masks):
        x = act(x @ hw[f"{n}/kernel"] + hw[f"{n}/bias"]) * torch.tensor(m, dtype=x.dtype) * float(c)
    return x @ hw["MLP_Head_no_Sigmoid/kernel"] + hw["MLP_Head_no_Sigmoid/bias"]


def head_grads(weights, encoded, dlogits, use_mish, masks, c):
    """(logits, grads) in float64 by autograd, as head_grad_oracle.head_grads."""
    hw = H.head_weights(weights)
    for t in hw.values():
        t.requires_grad_(True)
    enc = torch.tensor(np.asarray(encoded), dtype=torch.float64, requires_grad=True)
    logits = head_forward(hw, enc, use_mish, masks, c)
    (logits * torch.tensor(np.asarray(dlogits), dtype=torch.float64)).sum().backward()
    grads = OrderedDict((n, t.grad.numpy()) for n, t in hw.items())
    grads["encoded_images"] = enc.grad.numpy()
    return logits.detach().numpy(), grads


def model_forward(kw, wt, patches, masks, c, taps=None, inputs=None):
    """model_grad_oracle.model_forward with every dropout site."""
    k = V.resolve_kwargs(**kw)
    stem, blocks, head = M.split_names(kw)
    bmasks, hmasks = masks
    x = M.stem_forward([wt[n] for n in stem], patches)
    for names, bm in zip(blocks, bmasks):
        if inputs is not None:
            x.retain_grad()
            inputs.append(x)
        x = D.block_forward([wt[n] for n in names], x, k["use_mish"], bm, c, taps)
    if inputs is not None:
        x.retain_grad()
        inputs.append(x)
    return head_forward(OrderedDict((n, wt[n]) for n in head), x, k["use_mish"], hmasks, c)


def model_grads(kw, weights, images, dlogits, masks, c):
    """(logits, grads, dxs, den) as model_grad_oracle.model_grads returns them."""
    from tests import block_grad_oracle as K
    k = V.resolve_kwargs(**kw)
    stem, blocks, head = M.split_names(kw)
    wt = OrderedDict((n, torch.tensor(np.asarray(weights[n]), dtype=torch.float64,
                                      requires_grad=True)) for n in stem + sum(blocks, []) + head)
    taps, inputs = [], []
    logits = model_forward(kw, wt, torch.tensor(M.patches_of(images, k["patch_size"])), masks, c,
                           taps, inputs)
    (logits * torch.tensor(np.asarray(dlogits), dtype=torch.float64)).sum().backward()
    grads = OrderedDict((n, t.grad.numpy()) for n, t in wt.items())
    den = OrderedDict((n, float(np.abs(g).max())) for n, g in grads.items())
    for names, key in zip(blocks, taps):
        den[names[K.KEY_BIAS]] = float(np.abs(key.grad.numpy()).sum(axis=(0, 1)).max())
    return logits.detach().numpy(), grads, [t.grad.numpy() for t in inputs], den
