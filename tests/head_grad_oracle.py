"""The yardstick of the head backward: mlp_head (vtd.py:454-493) from `encoded_images` to the
logits in torch float64 with autograd, and a CPU emulation of what the device computes -- the
same chain of products on split-bf16 / plain-bf16 operands with fp32 accumulation.

The head: Dense(17) on (B, N, d); Reshape((17, -1)) -- a plain reinterpretation of each
image's N * 17 values; `n_head` blocks of Dense + Mish (or tanh GELU); Dense(6).
"""
import math
from collections import OrderedDict

import numpy as np
import torch

MAX_DETECT = 17


def head_names(weights):
    names, j = ["dense"], 1
    while f"dense_{j}/kernel" in weights:
        names.append(f"dense_{j}")
        j += 1
    return names + ["MLP_Head_no_Sigmoid"]


def head_weights(weights, dtype=torch.float64):
    """The head's tensors of a Keras-name keyed weight dict, in creation order."""
    out = OrderedDict()
    for n in head_names(weights):
        for part in ("kernel", "bias"):
            out[f"{n}/{part}"] = torch.tensor(np.asarray(weights[f"{n}/{part}"]), dtype=dtype)
    return out


def mish(x):
    return x * torch.tanh(torch.nn.functional.softplus(x, threshold=1e9))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def head_forward(hw, encoded, use_mish):
    """logits (B, 17, 6) from encoded (B, N, d); hw: head_weights()."""
    act = mish if use_mish else gelu_tanh
    names = [n[:-len("/kernel")] for n in hw if n.endswith("/kernel")]
    x = encoded @ hw["dense/kernel"] + hw["dense/bias"]                    # vtd.py:454-458
    x = x.reshape(x.shape[0], MAX_DETECT, -1)                              # vtd.py:461-463
    for n in names[1:-1]:                                                  # vtd.py:468-486
        x = act(x @ hw[f"{n}/kernel"] + hw[f"{n}/bias"])
    return x @ hw["MLP_Head_no_Sigmoid/kernel"] + hw["MLP_Head_no_Sigmoid/bias"]


def head_grads(weights, encoded, dlogits, use_mish):
    """(logits, grads) in float64 by autograd: grads keyed as the weights, plus
    "encoded_images"; dlogits is d loss / d logits."""
    hw = head_weights(weights)
    for t in hw.values():
        t.requires_grad_(True)
    enc = torch.tensor(np.asarray(encoded), dtype=torch.float64, requires_grad=True)
    logits = head_forward(hw, enc, use_mish)
    (logits * torch.tensor(np.asarray(dlogits), dtype=torch.float64)).sum().backward()
    grads = OrderedDict((n, t.grad.numpy()) for n, t in hw.items())
    grads["encoded_images"] = enc.grad.numpy()
    return logits.detach().numpy(), grads


# ------------------------------------------------------------------ operand emulation
def bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split(x):
    """(hi, lo) of a float32 tensor: hi = bf16(x), lo = bf16(x - hi), both as float32."""
    hi = bf16(x)
    return hi, bf16(x - hi)


def mm(a, b, mode):
    """a @ b as the device forms it: 'bf16x3' hi hi + lo hi + hi lo, 'bfloat16' bf16(a) bf16(b);
    products of bf16 values are exact in float32 and the sums run in float32."""
    a, b = a.float(), b.float()
    if mode == "bfloat16":
        return bf16(a) @ bf16(b)
    (ah, al), (bh, bl) = split(a), split(b)
    return ah @ bh + al @ bh + ah @ bl


def stored(x, mode):
    """float64 value of what the device stores for a float32 operand."""
    x = torch.as_tensor(x).float()
    if mode == "bfloat16":
        return bf16(x).double()
    hi, lo = split(x)
    return hi.double() + lo.double()


def act_grad64(z, use_mish):
    z = torch.tensor(np.asarray(z), dtype=torch.float64, requires_grad=True)
    (mish(z) if use_mish else gelu_tanh(z)).sum().backward()
    return z.grad


def emulated_head_backward(weights, encoded, dlogits, use_mish, mode):
    """The device's algorithm on the CPU: float32 pre-activations and activation values, every
    product through mm(); returns (logits, grads) as head_grads does, float32."""
    hw = head_weights(weights, torch.float32)
    names = [n[:-len("/kernel")] for n in hw if n.endswith("/kernel")]
    act = mish if use_mish else gelu_tanh
    enc = torch.tensor(np.asarray(encoded), dtype=torch.float32)
    B, N, d = enc.shape
    enc2 = enc.reshape(B * N, d)
    t = mm(enc2, hw["dense/kernel"], mode) + hw["dense/bias"]
    a = [t.reshape(B * MAX_DETECT, N)]
    zs = []
    for n in names[1:-1]:
        z = mm(a[-1], hw[f"{n}/kernel"], mode) + hw[f"{n}/bias"]
        zs.append(z)
        a.append(act(z.double()).float())
    logits = mm(a[-1], hw["MLP_Head_no_Sigmoid/kernel"], mode) + hw["MLP_Head_no_Sigmoid/bias"]
    grads = OrderedDict()
    g = torch.tensor(np.asarray(dlogits), dtype=torch.float32).reshape(B * MAX_DETECT, 6)
    grads["MLP_Head_no_Sigmoid/kernel"] = mm(a[-1].T, g, mode)
    grads["MLP_Head_no_Sigmoid/bias"] = stored(g, mode).sum(0).float()
    da = mm(g, hw["MLP_Head_no_Sigmoid/kernel"].T, mode)
    for i in range(len(zs) - 1, -1, -1):
        n = names[1 + i]
        gz = da * act_grad64(zs[i], use_mish).float()
        grads[f"{n}/kernel"] = mm(a[i].T, gz, mode)
        grads[f"{n}/bias"] = stored(gz, mode).sum(0).float()
        da = mm(gz, hw[f"{n}/kernel"].T, mode)
    dt = da.reshape(B * N, MAX_DETECT)
    grads["dense/kernel"] = mm(enc2.T, dt, mode)
    grads["dense/bias"] = stored(dt, mode).sum(0).float()
    grads["encoded_images"] = mm(dt, hw["dense/kernel"].T, mode).reshape(B, N, d)
    order = [f"{n}/{p}" for n in names for p in ("kernel", "bias")] + ["encoded_images"]
    return logits.reshape(B, MAX_DETECT, 6).numpy(), OrderedDict(
        (k, grads[k].numpy()) for k in order)


def rel_err(got, ref):
    """max |g - g64| / max |g64| of one tensor."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------ configurations
MULTI_TILE = dict(input_shape=(64, 64, 3), patch_size=4, embedding_dim=64, encoder_num_heads=2,
                  encoder_key_dim=32, encoder_mlp_quantities=2, encoder_repeat_times=1,
                  mlp_head_last_units=136, mlp_head_dense_layers_quantity=2,
                  mlp_head_dense_mish_block_repeats=1, use_mish=True)
BARS = {"bf16x3": 2e-4, "bfloat16": 5e-2}
