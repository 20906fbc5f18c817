"""The yardstick of vtd_layernorm_backward (csrc/vtd_layernorm_bwd.hip): a float64 numpy
LayerNorm backward, an fp32 numpy restatement of the kernels' own operation order, the measures,
the derived bars and the cases.  tests/test_ln_grad_kat.py checks all of it on the CPU;
tests/test_gpu_layernorm_backward.py holds the device to it.

The reference takes what the kernel takes: x, the fp32 (mean, rstd) per row, gamma, dy, add.  So
the statistics' own rounding is outside the measure, and

  xhat = (x - mean) rstd, gy = dy gamma
  dx = rstd (gy - mean_D(gy) - xhat mean_D(gy xhat)) + add
  dgamma = sum_rows dy xhat, dbeta = sum_rows dy.

Measures (componentwise; u = 2^-24):
  |dx - dx64| <= c den_x, den_x = rstd (|gy| + mean|gy| + |xhat| mean|gy xhat|) + |add|
  |dgamma - dgamma64| <= c_g sum_rows |dy xhat|, |dbeta - dbeta64| <= c_g sum_rows |dy|
with c = k_dx u and c_g = k_param u, the first-order counts of roundings on the longest path of
the kernels as written (every operation rounds once: the file is built without FMA contraction).

k_dx.  T = additions terms per lane in a row sum: 4 NV = 4 ceil(D / 256) on the vector path
(lane l holds columns (i 64 + l) 4 .. + 3 of chunk i), ceil(D / 64) on the generic path.
  xhat: the subtraction and the product, 2.  gy: 1.
  s1 = sum gy: a term meets at most T - 1 lane additions and the 6 of the wave butterfly; with
    gy's own rounding and the division by D: T + 7, relative to mean|gy|.
  s2 = sum gy xhat: the term carries gy (1), xhat (2) and the product (1): T + 10, relative to
    mean|gy xhat|.
  dx = ((gy - m1) - xhat m2) rstd + add: the first difference rounds once (relative to |gy| +
    mean|gy|), the product xhat m2 adds xhat's 2 and its own 1, the second difference, the
    product with rstd and the sum with add round once each, relative to everything before them.
  Per component of den_x: |gy|: 1 + 1 + 1 + 1 + 1 = 5; mean|gy|: (T + 7) + 4 = T + 11;
  |xhat| mean|gy xhat|: (T + 10) + 3 + 3 = T + 16; |add|: 1.  So k_dx = T + 16.

k_param.  A term dy xhat carries 3 roundings (dbeta's terms carry none; the one c_g covers both).
A wave adds the rows r0 + w, r0 + w + 4, ... of its range into a zero register: nw - 1
roundings, nw = range_rows / 4.  The four waves combine in order: 3.  The plane sum runs over 16
segments of seglen = ceil(ranges / 16) planes, each from zero: seglen - 1, then the segments in
order: 15.  k_param = 3 + (nw - 1) + 3 + (seglen - 1) + 15 = nw + seglen + 19.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24
EPS = 1e-3
MAX_RANGES, SEGS = 1024, 16


# ------------------------------------------------------------------ the launch geometry, restated
def range_rows(rows):
    q = -(-rows // (4 * MAX_RANGES))
    return 4 * max(q, 2)


def ranges(rows):
    return -(-rows // range_rows(rows))


def route(D, lds=(), misaligned=False):
    """"vec" or "generic": what layernorm_backward_launch takes for these leading dimensions."""
    vec = D % 4 == 0 and D <= 4096 and all(ld % 4 == 0 for ld in lds) and not misaligned
    return "vec" if vec else "generic"


def lane_terms(D, path):
    return 4 * -(-D // 256) if path == "vec" else -(-D // 64)


def k_dx(D, path):
    return lane_terms(D, path) + 16


def k_param(rows):
    return range_rows(rows) // 4 + -(-ranges(rows) // SEGS) + 19


# ------------------------------------------------------------------ float64
def stats32(x, eps=EPS):
    """fp32 (mean, rstd) [rows][2] of fp32 rows: any fp32 pair serves as the kernel's input."""
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=1).astype(f32)
    var = ((x64 - mean.astype(np.float64)[:, None]) ** 2).mean(axis=1)
    return np.stack([mean, (1.0 / np.sqrt(var + eps)).astype(f32)], axis=1)


def backward64(x, stat, gamma, dy, add=None):
    """dict(dx, dgamma, dbeta, den_x, den_g, den_b) in float64 from the kernel's fp32 inputs."""
    x, stat, gamma, dy = (np.asarray(a, np.float64) for a in (x, stat, gamma, dy))
    mean, rstd = stat[:, :1], stat[:, 1:2]
    xhat = (x - mean) * rstd
    gy = dy * gamma[None, :]
    m1 = gy.mean(axis=1, keepdims=True)
    m2 = (gy * xhat).mean(axis=1, keepdims=True)
    dx = rstd * (gy - m1 - xhat * m2)
    den = rstd * (np.abs(gy) + np.abs(gy).mean(axis=1, keepdims=True)
                  + np.abs(xhat) * np.abs(gy * xhat).mean(axis=1, keepdims=True))
    if add is not None:
        a = np.asarray(add, np.float64)
        dx = dx + a
        den = den + np.abs(a)
    return dict(dx=dx, dgamma=(dy * xhat).sum(axis=0), dbeta=dy.sum(axis=0), den_x=den,
                den_g=np.abs(dy * xhat).sum(axis=0), den_b=np.abs(dy).sum(axis=0))


def stats_fp32(x, eps=EPS):
    """(mean, rstd) as an fp32 two-pass evaluation gives them (numpy's pairwise sums): stands in
    for vtd_layernorm_stats where the op's statistics, roundings included, are part of what is
    measured."""
    x = np.asarray(x, f32)
    D = f32(x.shape[1])
    mean = (x.sum(axis=1, dtype=f32) / D).astype(f32)
    d = (x - mean[:, None]).astype(f32)
    var = ((d * d).astype(f32).sum(axis=1, dtype=f32) / D).astype(f32)
    return np.stack([mean, (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)], axis=1)


def stats64(x, eps=EPS):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1)
    return np.stack([mean, 1.0 / np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1) + eps)], axis=1)


OP_SHAPES = ((2, 31, 64), (1, 77, 768))


def op_case(shape):
    """N(0, 1) rows for the layer_norm op, which is measured against float64 with float64
    statistics: the fp32 statistics' own rounding then counts as error.  On N(0, 1) rows it is a
    few u of |x| ~ 1 and the derived bars hold it (test_ln_grad_kat.py, under half); on a row
    with mean 1e3 it would be 1e3 u, which is the statistics' error, not this kernel's."""
    return Case(shape[-1], shape[0] * shape[1], seed=7, designs=False)


def forward64(x, gamma, beta, eps=EPS):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * gamma + beta


# ------------------------------------------------------------------ the kernels' order in fp32
def _butterfly(s):
    """wave_sum (tests/ln_designs.py): s += s[l ^ o], o = 32 .. 1, over the last axis."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[..., lanes ^ o]).astype(f32)
    return s[..., 0]


def _row_sum(t, path):
    """sum over the columns of t [rows][D] as the kernel's lanes and wave add them."""
    rows, D = t.shape
    W = 4 if path == "vec" else 1
    n = -(-D // (64 * W))
    p = np.zeros((rows, n * 64 * W), f32)
    p[:, :D] = t
    p = p.reshape(rows, n, 64, W)
    s = np.zeros((rows, 64), f32)
    for i in range(n):
        for j in range(W):
            s = (s + p[:, i, :, j]).astype(f32)
    return _butterfly(s)


def emulate(x, stat, gamma, dy, add=None, path="vec", params=True):
    """(dx, dgamma, dbeta) in fp32, operation by operation as ln_bwd_kernel (path "vec") or
    ln_bwd_generic_kernel + ln_bwd_colsum_kernel ("generic"), then ln_bwd_reduce_kernel."""
    x, stat, gamma, dy = (np.asarray(a, f32) for a in (x, stat, gamma, dy))
    rows, D = x.shape
    mean, rstd = stat[:, :1], stat[:, 1:2]
    xh = ((x - mean).astype(f32) * rstd).astype(f32)
    gy = (dy * gamma[None, :]).astype(f32)
    Df = f32(D)
    m1 = (_row_sum(gy, path) / Df).astype(f32)[:, None]
    m2 = (_row_sum((gy * xh).astype(f32), path) / Df).astype(f32)[:, None]
    dx = (rstd * ((gy - m1).astype(f32) - (xh * m2).astype(f32)).astype(f32)).astype(f32)
    if add is not None:
        dx = (dx + np.asarray(add, f32)).astype(f32)
    if not params:
        return dx, None, None
    rpr, R = range_rows(rows), ranges(rows)
    term = np.zeros((2, R * rpr, D), f32)                  # rows past `rows` add exact zeros
    term[0, :rows] = (dy * xh).astype(f32)
    term[1, :rows] = dy
    term = term.reshape(2, R, rpr // 4, 4, D)              # [plane][range][step][wave][column]
    acc = np.zeros((2, R, 4, D), f32)
    for k in range(rpr // 4):
        acc = (acc + term[:, :, k]).astype(f32)
    plane = acc[:, :, 0]
    for w in (1, 2, 3):
        plane = (plane + acc[:, :, w]).astype(f32)         # [plane][range][column]
    seglen = -(-R // SEGS)
    pad = np.zeros((2, SEGS * seglen, D), f32)
    pad[:, :R] = plane
    pad = pad.reshape(2, SEGS, seglen, D)
    seg = np.zeros((2, SEGS, D), f32)
    for r in range(seglen):
        seg = (seg + pad[:, :, r]).astype(f32)
    tot = seg[:, 0]
    for s in range(1, SEGS):
        tot = (tot + seg[:, s]).astype(f32)
    return dx, tot[0], tot[1]


# ------------------------------------------------------------------ the measure
def ratio(got, want, den, c):
    """max |got - want| / (c den); where den == 0 the value must equal the reference."""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(err).all(), "non-finite value"
    zero = den == 0
    assert (err[zero] == 0).all(), "error where the measure's denominator is zero"
    return float((err[~zero] / (c * den[~zero])).max()) if (~zero).any() else 0.0


def ratios(got, ref, D, rows, path):
    """(dx, dgamma, dbeta) errors as fractions of their bars; dgamma / dbeta None when absent."""
    dx, dg, db = got
    c, cg = k_dx(D, path) * U, k_param(rows) * U
    out = [ratio(dx, ref["dx"], ref["den_x"], c)]
    out.append(None if dg is None else ratio(dg, ref["dgamma"], ref["den_g"], cg))
    out.append(None if db is None else ratio(db, ref["dbeta"], ref["den_b"], cg))
    return out


# ------------------------------------------------------------------ cases
WIDTHS_VEC = (4, 64, 252, 768, 1024, 4096)
WIDTHS_GENERIC = (7, 4100)
DESIGNS = ("constant_row", "offset_1e3", "constant_dy", "single_column_dy", "random")


def multi_range_rows():
    """The smallest row count with at least two ranges and a ragged last one."""
    rows = 1
    while not (ranges(rows) >= 2 and rows % range_rows(rows) != 0):
        rows += 1
    return rows


def row_counts():
    return (1, 5, multi_range_rows())


class Case:
    """x, gamma, dy, add [rows][D] fp32.  Row r follows DESIGNS[r % 5] when rows >= 5 (a lone
    row is random) unless designs is False: N(0, 1) rows then; gamma_mode "random" (1 + 0.1
    N(0, 1)), "const" (1.5) or "zero"."""

    def __init__(self, D, rows, gamma_mode="random", seed=0, designs=True):
        rng = np.random.default_rng(1000 * D + 10 * rows + seed)
        self.D, self.rows, self.gamma_mode = D, rows, gamma_mode
        x = rng.standard_normal((rows, D)).astype(f32)
        dy = rng.standard_normal((rows, D)).astype(f32)
        if rows >= 5 and designs:
            for r in range(rows):
                kind = DESIGNS[r % 5]
                if kind == "constant_row":
                    x[r] = f32(2.5)
                elif kind == "offset_1e3":
                    x[r] = (x[r] + f32(1e3)).astype(f32)
                elif kind == "constant_dy":
                    dy[r] = f32(0.75)
                elif kind == "single_column_dy":
                    dy[r] = 0
                    dy[r, (3 * r + 1) % D] = f32(-1.25)
        self.x, self.dy = x, dy
        self.add = rng.standard_normal((rows, D)).astype(f32)
        self.gamma = {"random": (1 + 0.1 * rng.standard_normal(D)).astype(f32),
                      "const": np.full(D, 1.5, f32), "zero": np.zeros(D, f32)}[gamma_mode]
        self.beta = (0.1 * rng.standard_normal(D)).astype(f32)

    def __repr__(self):
        return f"D{self.D}_rows{self.rows}_{self.gamma_mode}"


def shape_cases():
    return [Case(D, rows) for D in WIDTHS_VEC + WIDTHS_GENERIC for rows in row_counts()]


def reduce_cases():
    """More than 16 ranges (segments of several planes) and ranges of more than 8 rows."""
    return [Case(64, 323), Case(64, 8200)]


def design_cases():
    return [Case(D, 5, mode, seed=1) for D in (64, 768, 7) for mode in ("const", "zero", "random")]
