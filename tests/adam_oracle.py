"""The yardstick of vtd_adam_step (not a test): keras.optimizers.Adam in TF's ApplyAdam
functor order with `clipvalue`, followed by the ClipWeight constraint (vtd.py:209-236), restated
in numpy -- step32 in float32 with one rounding per operation, in the kernel's order (the
kernel must match it bit for bit), step64 the same in float64 -- and pack_ref, the bytes of the
forward's packed operand of a weight matrix.

The scalars are the fp32 values the C-ABI receives (beta_1, beta_2, epsilon, clipvalue,
max_weight); alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) is formed in double from them and,
in step32, rounded to float32 once.
"""
import math

import numpy as np

DEFAULTS = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7)


def _f32(x):
    return float(np.float32(x))


def alpha64(t, lr, beta_1, beta_2):
    b1, b2 = _f32(beta_1), _f32(beta_2)
    return float(lr) * math.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))


def _clip(x, bound):
    """x < lo ? lo : (x > hi ? hi : x): a NaN passes through (tf.clip_by_value)."""
    lo, hi = x.dtype.type(-bound), x.dtype.type(bound)
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _step(dtype, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight, constrain):
    if t < 1:
        raise ValueError("t starts at 1")
    w, m, v, g = (np.asarray(a, dtype) for a in (w, m, v, g))
    one = dtype(1.0)
    b1, b2, eps = dtype(np.float32(beta_1)), dtype(np.float32(beta_2)), dtype(np.float32(epsilon))
    alpha = dtype(alpha64(t, lr, beta_1, beta_2))
    with np.errstate(all="ignore"):
        if clipvalue is not None and clipvalue > 0:
            g = _clip(g, np.float32(clipvalue))
        m = m + (g - m) * (one - b1)
        v = v + (g * g - v) * (one - b2)
        w = w - (m * alpha) / (np.sqrt(v) + eps)
        if constrain:
            w = _clip(np.where(np.isnan(w), one, w), np.float32(max_weight))
    assert w.dtype == m.dtype == v.dtype == dtype
    return w, m, v


def step32(w, m, v, g, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipvalue=None,
           max_weight=10.0, constrain=True):
    """(w, m, v) after step t, float32, the kernel's operations in the kernel's order."""
    return _step(np.float32, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight,
                 constrain)


def step64(w, m, v, g, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipvalue=None,
           max_weight=10.0, constrain=True):
    return _step(np.float64, w, m, v, g, t, lr, beta_1, beta_2, epsilon, clipvalue, max_weight,
                 constrain)


# ------------------------------------------------------------------ packed operands
def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16))
    r = np.where(np.isnan(x), (u >> np.uint32(16)) | np.uint32(0x40), r)
    return r.astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_isnan(bits):
    bits = np.asarray(bits, np.uint16)
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def split(x):
    """(hi, lo) bf16 bits: hi = bf16(x), lo = bf16(x - hi) with x - hi in float32."""
    x = np.asarray(x, np.float32)
    hi = bf16_bits(x)
    with np.errstate(all="ignore"):
        lo = bf16_bits(x - bf16_value(hi))
    return hi, lo


def pack_ref(w, K_p, N_p, mode):
    """The forward's packed operand of a weight matrix w [K][N] as uint16 bf16 bits: W^T
    [N_p][K_p] ('bf16'), or the split-bf16 B operand [N_p][3 K_p] = [hi | hi | lo] ('bf16x3');
    zeros outside [N][K].  For a bias w [N]: the float32 padded vector [N_p] (K_p unused)."""
    w = np.asarray(w, np.float32)
    if w.ndim == 1:
        out = np.zeros(N_p, np.float32)
        out[:w.size] = w
        return out
    K, N = w.shape
    assert K_p >= K and N_p >= N
    hi, lo = split(w.T)
    if mode == "bf16":
        out = np.zeros((N_p, K_p), np.uint16)
        out[:N, :K] = hi
        return out
    assert mode == "bf16x3"
    out = np.zeros((N_p, 3 * K_p), np.uint16)
    out[:N, :K] = hi
    out[:N, K_p:K_p + K] = hi
    out[:N, 2 * K_p:2 * K_p + K] = lo
    return out
