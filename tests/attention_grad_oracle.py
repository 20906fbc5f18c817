"""The yardstick of vtd_attention_train / vtd_attention_backward, no GPU.

  forward64 / backward64   the attention core and its gradients in float64
  emulate                  a numpy emulation of each operand mode's ROUNDINGS (operands rounded
                           to bf16, or split hi / lo with the lo.lo term dropped; P, dS and O
                           rounded where the kernels round them; every sum exact, in float64)
  magnitudes               float64 componentwise magnitudes for the designed inputs, whose
                           gradients nearly cancel
  random_case              the seeded inputs the host and the GPU tests share

All arrays are [B][N][H][dk] (q, k, v, dO, O and the gradients) or [B][H][N] (lse).
"""
import math

import numpy as np

LOG2E_F32 = np.float32(1.4426950408889634)
LN2 = 0.6931471805599453

# per tensor max |g - g64| / max |g64| (the project's head-backward bars) and the componentwise
# factor of the designed cases (the vtd_gemm_wgrad bars); lse against max(1, max |lse64|)
BARS = {"x3": 2e-4, "bf16": 5e-2}
C_DESIGNED = {"x3": 2.0 ** -15, "bf16": 2.0 ** -7}
LSE_TOL = {"x3": 2e-5, "bf16": 2e-2}

# (B, heads, N, key_dim): a single row, a ragged 32-block, a full block + 1, ragged blocks, the
# C2 length, one 256-key block and + 1, several blocks, each dkp
SHAPES = [(1, 1, 1, 24), (2, 2, 31, 24), (2, 3, 33, 24), (2, 2, 77, 24), (2, 2, 196, 40),
          (1, 2, 256, 64), (1, 2, 257, 64), (1, 2, 290, 128), (1, 2, 400, 64), (1, 1, 577, 64)]
# the standard deviation of q, k, v, dO per shape: 1.5, or 1.0 where the issue's table says so
# (N 196 / dk 40 and N 290 / dk 128)
SIGMA = {s: (1.0 if s[3] in (40, 128) else 1.5) for s in SHAPES}
DESIGNED_PATTERNS = ("spike", "tie", "staircase", "offset")
DESIGNED_SHAPES = [(77, 24), (196, 40), (290, 64)]        # (N, key_dim); B = H = 2


def dkp_of(dk):
    return 32 if dk <= 32 else (64 if dk <= 64 else 128)


def bf16(x):
    """The nearest bf16 value (ties to even) of float32(x), as float64."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return r.astype(np.float64)


def split(x):
    """float32(x) -> (hi, lo) = (bf16(x), bf16(x - hi)), float64."""
    x32 = np.asarray(x, np.float32).astype(np.float64)
    hi = bf16(x32)
    return hi, bf16(x32 - hi)


def random_case(shape, mode, sigma=None):
    """q, k, v, dO ~ N(0, sigma) float64 holding float32 values (x3) or bf16 values (bf16), and
    scale = 1 / sqrt(key_dim).  Seeded by the shape alone: both modes draw the same numbers."""
    B, H, N, dk = shape
    sigma = SIGMA[shape] if sigma is None else sigma
    rng = np.random.default_rng([B, H, N, dk])
    t = [rng.normal(0.0, sigma, size=(B, N, H, dk)).astype(np.float32) for _ in range(4)]
    if mode == "bf16":
        return [bf16(a) for a in t], 1.0 / math.sqrt(dk)
    return [a.astype(np.float64) for a in t], 1.0 / math.sqrt(dk)


def designed_do(pattern, N, dk, B=2, H=2):
    """bf16-representable N(0, 1) dO for a designed case."""
    rng = np.random.default_rng([DESIGNED_PATTERNS.index(pattern), N, dk, 7])
    return bf16(rng.normal(0.0, 1.0, size=(B, N, H, dk)).astype(np.float32))


def unpack_qkv(qkv, B, N, H, dk):
    """The packed [B*N][ld] matrix of tests/test_gpu_attention_patterns.pack_qkv -> q, k, v."""
    dkp = dkp_of(dk)
    out = []
    for part in range(3):
        m = np.zeros((B, N, H, dk), np.float64)
        for h in range(H):
            c0 = part * H * dkp + h * dkp
            m[:, :, h, :] = qkv[:, c0:c0 + dk].reshape(B, N, dk)
        out.append(m)
    return out


# ------------------------------------------------------------------------------- float64
def _scores(q, k):
    return np.einsum("bqhd,bkhd->bhqk", q, k)


def forward64(q, k, v, scale):
    """(O [B][N][H][dk], lse [B][H][N] natural units, P [B][H][N][N])."""
    s = _scores(q, k) * float(scale)
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    return np.einsum("bhqk,bkhd->bqhd", p, v), (m + np.log(l))[..., 0], p


def backward64(q, k, v, do, scale):
    """(dQ, dK, dV) of sum(O * dO)."""
    o, _, p = forward64(q, k, v, scale)
    delta = np.einsum("bqhd,bqhd->bhq", do, o)
    dp = np.einsum("bqhd,bkhd->bhqk", do, v)
    ds = p * (dp - delta[..., None]) * float(scale)
    return (np.einsum("bhqk,bkhd->bqhd", ds, k), np.einsum("bhqk,bqhd->bkhd", ds, q),
            np.einsum("bhqk,bqhd->bkhd", p, do))


def magnitudes(q, k, v, do, scale):
    """den_dQ = A |K|, den_dK = A^T |Q|, den_dV = P^T |dO| with
    A = P o (|dO| |V|^T + sum_d |dO O|) scale: what each gradient component's terms add up to
    in magnitude before they cancel."""
    o, _, p = forward64(q, k, v, scale)
    a = p * (np.einsum("bqhd,bkhd->bhqk", np.abs(do), np.abs(v)) +
             np.einsum("bqhd,bqhd->bhq", np.abs(do), np.abs(o))[..., None]) * float(scale)
    return (np.einsum("bhqk,bkhd->bqhd", a, np.abs(k)), np.einsum("bhqk,bqhd->bkhd", a, np.abs(q)),
            np.einsum("bhqk,bqhd->bkhd", p, np.abs(do)))


def rel_err(g, g64):
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def tensor_errors(got, q, k, v, do, scale):
    """max |g - g64| / max |g64| for (dQ, dK, dV).  With a single key P is 1 and dS = dP - delta
    is 0 for every input: dQ and dK are zero, a complete cancellation, and the measure has no
    denominator; there (N = 1 only) the error is taken against the largest magnitude of the
    cancelling terms (`magnitudes`), which is what a rounding of them can leave behind."""
    g64 = backward64(q, k, v, do, scale)
    if q.shape[1] > 1:
        return [rel_err(g, r) for g, r in zip(got, g64)]
    den = magnitudes(q, k, v, do, scale)
    return [float(np.abs(g - r).max() / d.max()) for g, r, d in zip(got, g64, den)]


# ------------------------------------------------------------------------------- emulation
def _prod(eq, a, b, mode):
    """One product of the device: bf16 x bf16 (operands already bf16 values), or the three
    products hi.hi + lo.hi + hi.lo of the split operands; exact sums."""
    if mode == "bf16":
        return np.einsum(eq, a, b)
    ah, al = split(a)
    bh, bl = split(b)
    return np.einsum(eq, ah, bh) + np.einsum(eq, al, bh) + np.einsum(eq, ah, bl)


def _rnd(x, mode):
    """What the device stores or feeds to the next product: a bf16 value, or hi + lo."""
    if mode == "bf16":
        return bf16(x)
    hi, lo = split(x)
    return hi + lo


def emulate(q, k, v, do, scale, mode):
    """dict(o, lse, dq, dk, dv): the training forward and the backward with each mode's
    roundings.  bf16: the query pre-scaled by float32(scale log2 e) and rounded to bf16 again
    (forward and backward alike), P rounded to bf16 for P V and P^T dO, dS rounded to bf16, O and
    the gradients stored as bf16.  x3: every operand split, P and dS split, O and the gradients
    stored as hi + lo, and the backward's P divided by its own row sums.  Statistics (max, sum,
    lse, delta) in fp32 values, sums exact."""
    c = np.float32(np.float32(scale) * LOG2E_F32)
    if mode == "bf16":
        qs = bf16(q.astype(np.float32) * c)                        # log2 units
        s2 = np.einsum("bqhd,bkhd->bhqk", qs, k)
    else:
        s2 = (_prod("bqhd,bkhd->bhqk", q, k, mode).astype(np.float32) * c).astype(np.float64)
    m = s2.max(axis=-1, keepdims=True)
    p = np.exp2(s2 - m).astype(np.float32).astype(np.float64)
    l = p.sum(axis=-1, keepdims=True)
    pv = _prod("bhqk,bkhd->bqhd", _rnd(p, mode), v, mode)
    o = _rnd(pv / np.moveaxis(l, 1, 2), mode)
    lse = ((m + np.log2(l)) * LN2).astype(np.float32).astype(np.float64)[..., 0]
    # backward
    delta = np.einsum("bqhd,bqhd->bhq", do, o).astype(np.float32).astype(np.float64)
    nl = (lse.astype(np.float32) * LOG2E_F32).astype(np.float64)
    pb = np.exp2(s2 - nl[..., None]).astype(np.float32).astype(np.float64)
    if mode == "x3":
        # the split mode divides by the row sums of what it recomputed: lse's own rounding (one
        # fp32 number per row, a common factor of the row) cancels
        rinv = (1.0 / pb.sum(axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)
        pb = (pb * rinv).astype(np.float32).astype(np.float64)
    dp = _prod("bqhd,bkhd->bhqk", do, v, mode) - delta[..., None]
    ds = _rnd(pb * dp, mode)
    sc = float(np.float32(scale))
    return dict(o=o, lse=lse,
                dq=_rnd(_prod("bhqk,bkhd->bqhd", ds, k, mode) * sc, mode),
                dk=_rnd(_prod("bhqk,bqhd->bkhd", ds, q, mode) * sc, mode),
                dv=_rnd(_prod("bhqk,bqhd->bkhd", _rnd(pb, mode), do, mode), mode))
