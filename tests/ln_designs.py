"""Designed rows for the LayerNorm family (csrc/vtd_elementwise.hip): generator, float64
references, bounds, a restatement of the dispatch and a numpy emulation of the kernels'
arithmetic.  Pure numpy, importable without a GPU; tests/test_ln_designs_host.py checks this
module on the CPU, tests/test_gpu_layernorm_designed.py runs the same cases on the device.

Order-free rows: x[c] = m + h k[c], h a power of two, k[c] integers with 1 <= |k| <= 64 (fewer
for D > 4096) and sum(k) == 0.  In units of h every x is an integer and every partial sum of x
stays below 2^24 units (`check_order_free` asserts D (|m / h| + max |k|) < 2^24, and
D max(k^2) <= 2^24 for the squares): every partial sum in any order is an fp32 number.  So
mean == m exactly, every d = x - mean = h k exactly, q = sum(d^2) = h^2 sum(k^2) exactly,
whatever the lane layout (4, 8, 16 columns per lane, the 64-stride generic loop) and with or
without FMA contraction.  What remains is q / D, + eps, sqrt, 1 / x: four correctly rounded
fp32 operations, at most (1/2 + 1/2 + 1 + 1) 2^-24 = 0.75 x 2^-22 relative on rstd.
(D = 1 admits no non-zero k with sum zero: its row is x = m, k = 0.)

Constant rows: x = c0 (an integer), d == 0, so y == beta (f32 output) or bf16(beta) in every
column, byte for byte; rstd = 1 / sqrt(eps).

General rows: seeded N(1, 3), and one row per case with a high offset (1e3 for f32 input, 200
for bf16 input), rounded to the input dtype before any reference runs.  Their sums are not
exact, so they are held to a measured bound (below).

gamma = 1 + j / 16, beta = j / 8, j in [-8, 8], differing from column to column.

Bounds.  Designed (order-free and constant) rows, derived:
  stats   mean bit-exact; |rstd - rstd64| <= 2^-22 rstd64;
  f32 y   |y - y64| <= 4 x 2^-23 (|p| + |beta|), p = (x - mean64) rstd64 gamma: d is exact, the
          device spends at most 6 x 2^-24 |p| (rstd, two products) + 2^-24 (|p| + |beta|);
  bf16 y  bf16(y64 - b) <= y <= bf16(y64 + b) with b the f32 bound (rounding is monotonic);
  constant rows: equality.
General rows, measured: per row |device - float64| <= 8 x the worst error in that row of an
fp32 numpy evaluation of the same two-pass formula + 4 fp32 ulp of the row's largest |float64
value| -- the rule and the margin of tests/test_gpu_loss_grad.py.  The yardstick never involves
the device output.  It is the larger of two evaluations: numpy's pairwise sums, and the same
formula summed in the routed kernel's lane order (`emulate`).  One evaluation alone does not
serve: in a high-offset row the error of every y is the rounding of the mean, anywhere in
[0, ulp(mean) / 2] by the luck of the summation order, so a correct kernel exceeds 8 x a lucky
pairwise evaluation about once in sixteen rows (the lane-order emulation itself did, D = 63,
offset 1e3: 2.83e-5 against 8 x 2.9e-6).  `Report.pairwise` keeps the ratio against the pairwise
evaluation alone.
"""
import math

import numpy as np

from oracle import mx8 as MX
from tests import gemm_designs as G

f32 = np.float32
EPS = float(np.float32(1e-3))                   # the value the C-ABI receives
LIMIT = 2 ** 24
U23, U22 = 2.0 ** -23, 2.0 ** -22
bf16_bits, bf16_value = G.bf16_bits, G.bf16_value

ORDER_FREE = {"f32": ((0.0, 0.125), (16.0, 0.125), (-100.0, 0.125), (256.0, 0.125)),
              "bf16": ((0.0, 0.125), (16.0, 0.125), (256.0, 2.0))}
CONSTANTS = (3.0, -7.0, 100.0)
HIGH_OFFSET = {"f32": 1e3, "bf16": 200.0}


# ------------------------------------------------------------------ the dispatch restated
def _bucket(n, sizes):
    return next((s for s in sizes if n <= s), None)


def ln16_ok(xdt, D, ldx, x_mis=0, g_mis=0, b_mis=0):
    """ln16_ok: *_mis are the byte addresses modulo 16 (0 = 16-byte aligned)."""
    return (D % 16 == 0 and D <= 4096 and ldx % (8 if xdt == "bf16" else 4) == 0
            and x_mis % 16 == 0 and g_mis % 16 == 0 and b_mis % 16 == 0)


def route(entry, xdt=None, D=0, ldx=0, P=0, out="f32", Kq=0, x_mis=0, y_mis=0, g_mis=0, b_mis=0,
          slots=0):
    """(kernel, NV or NC or S) that ln_dispatch / layernorm_mx8_launch / ln_stats_dispatch /
    ln_stats_finalize_launch choose.  P: the output piece width (ldy, or ldy / 2 for a split
    output); *_mis: byte address modulo 16."""
    isz = 2 if xdt == "bf16" else 4
    if entry == "layernorm":
        osz = 4 if out == "f32" else 2
        vec = (D % 4 == 0 and ldx % 4 == 0 and P % 4 == 0 and x_mis % (4 * isz) == 0
               and y_mis % (4 * osz) == 0 and g_mis % 16 == 0 and b_mis % 16 == 0)
        if vec and xdt == "bf16" and ln16_ok(xdt, D, ldx, x_mis, g_mis, b_mis):
            return "layernorm16_kernel", _bucket(-(-D // 1024), (1, 2, 4))
        nv = _bucket(-(-D // 256), (1, 2, 3, 4, 8, 16))
        if vec and nv:
            return "layernorm_kernel", nv
        return "layernorm_generic_kernel", 0
    if entry == "layernorm_mx8":
        ok = (D % 4 == 0 and ldx % 4 == 0 and g_mis % 16 == 0 and b_mis % 16 == 0
              and x_mis % (8 if xdt == "bf16" else 16) == 0 and Kq % 128 == 0 and D <= Kq <= 4096)
        if not ok:
            return "invalid", 0
        if ln16_ok(xdt, D, ldx, x_mis, g_mis, b_mis):
            return "layernorm16_mx8_kernel", _bucket(-(-Kq // 1024), (1, 2, 4))
        return "layernorm_mx8_kernel", _bucket(-(-Kq // 256), (2, 4, 8, 16))
    if entry == "layernorm_stats":
        nv = _bucket(-(-D // 512), (1, 2, 4))
        if D % 8 == 0 and ldx % 8 == 0 and x_mis % 16 == 0 and nv:
            return "ln_stats_kernel", nv
        return "ln_stats_generic_kernel", 0
    if entry == "layernorm_stats_finalize":
        return ("ln_stats_finalize_s_kernel", slots) if slots in (12, 16) \
            else ("ln_stats_finalize_kernel", 0)
    raise ValueError(entry)


# every kernel and NV / NC / S the family instantiates
INSTANTIATIONS = (
    [("layernorm_kernel", n) for n in (1, 2, 3, 4, 8, 16)]
    + [("layernorm16_kernel", n) for n in (1, 2, 4)] + [("layernorm_generic_kernel", 0)]
    + [("layernorm16_mx8_kernel", n) for n in (1, 2, 4)]
    + [("layernorm_mx8_kernel", n) for n in (2, 4, 8, 16)]
    + [("ln_stats_kernel", n) for n in (1, 2, 4)] + [("ln_stats_generic_kernel", 0)]
    + [("ln_stats_finalize_s_kernel", 12), ("ln_stats_finalize_s_kernel", 16),
       ("ln_stats_finalize_kernel", 0)])


# ------------------------------------------------------------------ rows
def k_cap(D):
    return min(64, math.isqrt(LIMIT // D))


def order_free_k(D, rng):
    """Integers, 1 <= |k| <= k_cap(D), sum(k) == 0 (D = 1: k = 0, the only choice)."""
    if D == 1:
        return np.zeros(1, np.int64)
    cap = k_cap(D)
    k = rng.integers(1, cap + 1, D) * rng.choice((-1, 1), D)
    s = int(k.sum())
    while s:
        i = int(rng.integers(D))
        new = int(np.clip(k[i] - s, -cap, cap))
        if new == 0:                                # one past zero: the next step mends it
            new = -1 if s > 0 else 1
        s += new - int(k[i])
        k[i] = new
    return k


def check_order_free(k, m, h, bf16=False):
    """The exactness rule of the module docstring, asserted per row."""
    D = len(k)
    assert math.frexp(h)[0] == 0.5, "h must be a power of two"
    assert int(k.sum()) == 0, "sum(k) != 0"
    assert D == 1 or (np.abs(k) >= 1).all(), "a zero k moves neither sum"
    assert D * int((k * k).max()) <= LIMIT, "D max(k^2) > 2^24: q is not order-free"
    assert abs(D * m / h) < LIMIT, "|D m / h| >= 2^24: the sum is not order-free"
    assert (m / h) == int(m / h) and D * (abs(m / h) + int(np.abs(k).max())) < LIMIT, \
        "a partial sum of x can leave the fp32 integers"
    x = m + h * k.astype(np.float64)
    x32 = G.to_f32_exact(x)
    if bf16:
        assert np.array_equal(bf16_value(bf16_bits(x32)), x32), "a value is not a bf16 number"
    return x32


class Case:
    """One x buffer: rows of differing kinds, gamma, beta, and where they sit in memory.
    x_off / g_off: elements by which x / gamma start past a 256-byte boundary."""

    def __init__(self, xdt, rows, D, ldx=None, x_off=0, g_off=0, seed=0, kinds=None):
        self.xdt, self.rows, self.D, self.x_off, self.g_off = xdt, rows, D, x_off, g_off
        self.ldx = ldx if ldx is not None else D + (8 if D % 4 == 0 else 5)
        self.isz = 2 if xdt == "bf16" else 4
        rng = np.random.default_rng([seed, rows, D, self.isz, x_off, g_off])
        of = ORDER_FREE[xdt]
        if kinds is None:
            cycle = [("of", i) for i in range(len(of))] + [("const", 0), ("gen", 0), ("hi", 0)]
            start = 1 if rows == 1 else 0           # a single row: a non-zero mean
            kinds = [cycle[(start + r) % len(cycle)] for r in range(rows)]
            kinds = [(k, (r // len(cycle)) % 3 if k == "const" else v)
                     for r, (k, v) in enumerate(kinds)]
        self.kinds = kinds
        self.x = np.zeros((rows, D), f32)
        self.k = [None] * rows
        self.designed = np.zeros(rows, bool)
        self.exact_mean = np.zeros(rows, f32)
        for r, (kind, v) in enumerate(kinds):
            if kind == "of":
                m, h = of[v]
                self.k[r] = order_free_k(D, rng)
                self.x[r] = check_order_free(self.k[r], m, h, xdt == "bf16")
                self.designed[r], self.exact_mean[r] = True, m
            elif kind == "const":
                c0 = CONSTANTS[v]
                assert abs(D * c0) < LIMIT
                self.x[r] = c0
                self.designed[r], self.exact_mean[r] = True, c0
            else:
                row = rng.normal(1.0, 3.0, D) + (HIGH_OFFSET[xdt] if kind == "hi" else 0.0)
                self.x[r] = row.astype(f32)
        if xdt == "bf16":
            self.x = bf16_value(bf16_bits(self.x))
        self.gamma = (1 + rng.integers(-8, 9, D) / 16).astype(f32)
        self.beta = (rng.integers(-8, 9, D) / 8).astype(f32)
        self.constant = np.array([k == "const" for k, _ in kinds])

    def __repr__(self):
        return (f"{self.xdt} rows {self.rows} D {self.D} ldx {self.ldx} x_off {self.x_off} "
                f"g_off {self.g_off}")

    # ---- memory images
    def x_body(self):
        """[rows + 1][ldx] of the input dtype: the rows start x_off elements in; pad columns,
        the lead-in and the tail are NaN."""
        bits = self.xdt == "bf16"
        body = np.full((self.rows + 1) * self.ldx, 0x7FC0 if bits else np.nan,
                       np.uint16 if bits else f32)
        assert self.x_off <= self.ldx
        for r in range(self.rows):
            o = self.x_off + r * self.ldx
            body[o:o + self.D] = bf16_bits(self.x[r]) if bits else self.x[r]
        return body.reshape(self.rows + 1, self.ldx)

    def x_rows(self):
        """[rows][ldx] float64 view of what a kernel sees from its x pointer (NaN pads)."""
        b = self.x_body().ravel()[self.x_off:self.x_off + self.rows * self.ldx]
        v = bf16_value(b) if self.xdt == "bf16" else b
        return v.astype(np.float64).reshape(self.rows, self.ldx)

    def vec_body(self, v):
        """gamma / beta: g_off NaN elements, then exactly D values (guards follow)."""
        return np.concatenate([np.full(self.g_off, np.nan, f32), np.asarray(v, f32)])

    def mis(self):
        return dict(x_mis=self.x_off * self.isz % 16, g_mis=self.g_off * 4 % 16,
                    b_mis=self.g_off * 4 % 16)

    def route(self, entry, **kw):
        return route(entry, self.xdt, self.D, self.ldx, **self.mis(), **kw)

    # ---- references
    def ref64(self, gamma=None, beta=None):
        x = self.x.astype(np.float64)
        mean = x.mean(axis=1)
        d = x - mean[:, None]
        rstd = 1.0 / np.sqrt((d * d).mean(axis=1) + EPS)
        g = (self.gamma if gamma is None else gamma).astype(np.float64)
        b = (self.beta if beta is None else beta).astype(np.float64)
        p = d * rstd[:, None] * g
        return mean, rstd, p, p + b

    def np32(self, gamma=None, beta=None):
        """The yardstick of the measured bound: the two-pass formula in fp32 numpy."""
        x = self.x
        D = f32(self.D)
        mean = (x.sum(axis=1, dtype=f32) / D).astype(f32)
        d = x - mean[:, None]
        rstd = (f32(1) / np.sqrt((d * d).sum(axis=1, dtype=f32) / D + f32(EPS))).astype(f32)
        g = self.gamma if gamma is None else gamma
        b = self.beta if beta is None else beta
        return mean, rstd, (d * rstd[:, None] * g + b).astype(f32)

    def yardstick(self, kernel=None):
        """Per row, the error against float64 of fp32 numpy evaluations of the two-pass formula:
        (mean, rstd, worst y) errors, each as (used, pairwise).  `pairwise` is np32 alone; `used`
        is the larger of np32's and, when `kernel` = (name, n) is given, that of the same formula
        summed in that kernel's lane order (emulate).  Neither involves the device."""
        key = ("yardstick", kernel)
        if key not in self.__dict__:
            mean64, rstd64, _, y64 = self.ref64()
            evals = [self.np32()]
            if kernel is not None:
                evals.append(emulate(self, *kernel))
            errs = [(np.abs(m - mean64), np.abs(r - rstd64), np.abs(y - y64).max(axis=1))
                    for m, r, y in evals]
            self.__dict__[key] = tuple((np.maximum.reduce([e[i] for e in errs]), errs[0][i])
                                       for i in range(3))
        return self.__dict__[key]


def bf16_rne64(v):
    """float64 -> the nearest bf16 number (ties to even), one rounding, as float64.  Normal
    range only: 8 significant bits, quantum 2^(e - 7)."""
    v = np.asarray(v, np.float64)
    _, ex = np.frexp(v)                                  # |v| in [2^(ex - 1), 2^ex)
    quantum = np.exp2(ex.astype(np.float64) - 8)
    return np.rint(v / quantum) * quantum


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(f32)).astype(np.float64)


# ------------------------------------------------------------------ checks (device and emulation)
class Report:
    """Worst ratios of one entry point (or of one case), printed and quoted in the docstrings."""

    def __init__(self):
        self.designed, self.general, self.pairwise = 0.0, 0.0, 0.0
        self.gen_err = self.gen_emu = 0.0               # the row behind `general`
        self.rstd_equal, self.rstd_total = 0, 0

    def note_general(self, err, used, pair, floor):
        """One general row: device error, the yardstick's error (used; pairwise alone)."""
        if err / max(used, floor) > self.general:
            self.general, self.gen_err, self.gen_emu = err / max(used, floor), err, used
        self.pairwise = max(self.pairwise, err / max(pair, floor))

    def merge(self, o):
        if o.general > self.general:
            self.general, self.gen_err, self.gen_emu = o.general, o.gen_err, o.gen_emu
        self.designed, self.pairwise = max(self.designed, o.designed), max(self.pairwise, o.pairwise)
        self.rstd_equal, self.rstd_total = self.rstd_equal + o.rstd_equal, self.rstd_total + o.rstd_total

    def __str__(self):
        return (f"designed rows worst error / bound {self.designed:.3f}; general rows worst "
                f"device error / fp32-numpy error {self.general:.3f} (device {self.gen_err:.3g}, "
                f"numpy {self.gen_emu:.3g}; against the pairwise evaluation alone "
                f"{self.pairwise:.3f}); rstd bit-equal to fp32 numpy "
                f"{self.rstd_equal} of {self.rstd_total}")


def check_stats(case, got, rep=None, what="stats", kernel=None):
    """got [rows][2] f32 = (mean, rstd); kernel: the call's route, for the yardstick."""
    got = np.asarray(got, f32)
    mean64, rstd64, _, _ = case.ref64()
    _, rstd32, _ = case.np32()
    ymean, yrstd, _ = case.yardstick(kernel)
    assert np.isfinite(got).all(), f"{what}: not finite"
    rep = rep or Report()
    for r in range(case.rows):
        gm, gr = float(got[r, 0]), float(got[r, 1])
        if case.designed[r]:
            assert got[r, 0] == case.exact_mean[r], \
                f"{what}: row {r} mean {gm!r} != {float(case.exact_mean[r])!r} (must be exact)"
            ratio = abs(gr - rstd64[r]) / (U22 * rstd64[r])
            assert ratio <= 1, f"{what}: row {r} rstd {gr!r} vs {rstd64[r]!r}: {ratio:.3f} of 2^-22"
            rep.designed = max(rep.designed, ratio)
        else:
            for name, g, (used, pair), ref in (("mean", gm, ymean, mean64[r]),
                                               ("rstd", gr, yrstd, rstd64[r])):
                tol = 8 * float(used[r]) + 4 * float(ulp32(ref))
                err = abs(g - ref)
                assert err <= tol, (f"{what}: row {r} {name} {g!r} vs {ref!r}: error {err:.3g}, "
                                    f"fp32 numpy {used[r]:.3g}, allowed {tol:.3g}")
                rep.note_general(err, float(used[r]), float(pair[r]), float(ulp32(ref)) / 2)
        rep.rstd_total += 1
        rep.rstd_equal += int(got[r, 1] == rstd32[r])
    return rep


def y_bounds(case, kernel=None):
    """(y64, tol [rows][D], yardstick errors): the derived bound on designed rows, the measured
    one on general rows."""
    _, _, p, y64 = case.ref64()
    tol = 4 * U23 * (np.abs(p) + np.abs(case.beta.astype(np.float64))[None, :])
    used, pair = case.yardstick(kernel)[2]
    m = 8 * used + 4 * ulp32(np.abs(y64).max(axis=1))
    for r in range(case.rows):
        if not case.designed[r]:
            tol[r] = m[r]
        if case.constant[r]:
            tol[r] = 0.0
    return y64, tol, used, pair


def check_y(case, out, got, rep=None, what="y", kernel=None):
    """got [rows][D]: f32 values (out "f32") or bf16 bits (out "bf16"); kernel: the route."""
    y64, tol, emu, pair = y_bounds(case, kernel)
    rep = rep or Report()
    if out == "f32":
        got = np.asarray(got, f32)
        assert not np.isnan(got).any(), f"{what}: NaN in the output"
        err = np.abs(got.astype(np.float64) - y64)
        bad = err > tol
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: {bad.sum()} of {bad.size} outside the bound, first at "
                                 f"row {r} ({case.kinds[r][0]}) column {c}: got {got[r, c]!r}, "
                                 f"float64 {y64[r, c]!r}, error {err[r, c]:.3g} > {tol[r, c]:.3g}")
        for r in range(case.rows):
            if case.constant[r]:
                continue
            if case.designed[r]:
                ok = tol[r] > 0
                if ok.any():
                    rep.designed = max(rep.designed, float((err[r][ok] / tol[r][ok]).max()))
            else:
                floor = float(ulp32(np.abs(y64[r]).max())) / 2
                rep.note_general(float(err[r].max()), float(emu[r]), float(pair[r]), floor)
        return rep
    got = bf16_value(np.asarray(got, np.uint16))
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    lo, hi = bf16_rne64(y64 - tol), bf16_rne64(y64 + tol)
    bad = (got < lo) | (got > hi)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} bf16 outputs outside "
                             f"[bf16(y64 - b), bf16(y64 + b)], first at row {r} "
                             f"({case.kinds[r][0]}) column {c}: got {got[r, c]!r}, float64 "
                             f"{y64[r, c]!r}, allowed [{lo[r, c]!r}, {hi[r, c]!r}]")
    return rep


def split_expected(y_f32, P):
    """[hi | lo] bf16 bits of the f32 output, each piece P wide with zero pad columns."""
    rows, D = y_f32.shape
    yp = np.zeros((rows, P), f32)
    yp[:, :D] = y_f32
    hi, lo = G.split_bits(yp)
    return np.concatenate([hi, lo], axis=1)


# ------------------------------------------------------------------ MX-fp8
encode_e4m3 = MX.encode_e4m3       # e4m3 values -> bytes; the sign bit of -0 is kept


def mx_expected(vals, Kq):
    """f32 values [rows][D] (already bf16 numbers) -> (bytes [rows][Kq], scale bytes
    [rows][Kq / 32]) by oracle/mx8.py; columns [D, Kq) are zero."""
    v, E = MX.quantize(np.asarray(vals, np.float64), Kq)
    return encode_e4m3(v), (E + 127).astype(np.uint8)


def scale_body(scales, s_rows, fill):
    """[rows][Kq / 32] -> the device layout [Kq / 128][s_rows][4] as [Kq / 128][4 s_rows], rows
    past `rows` holding `fill`; also the mask of what the contract writes."""
    rows, nb = scales.shape
    body = np.full((nb // 4, s_rows, 4), fill, np.uint8)
    body[:, :rows] = scales.reshape(rows, nb // 4, 4).transpose(1, 0, 2)
    mask = np.zeros((nb // 4, s_rows, 4), bool)
    mask[:, :rows] = True
    return body.reshape(nb // 4, 4 * s_rows), mask.reshape(nb // 4, 4 * s_rows)


def mx_beta(D, rng):
    """beta for the constant-row check of the fused quantizer: per 32-column block j the maximum
    sits at column 32 j + (j mod 32) (every lane position of the amax exchange carries it once);
    the block kinds cycle through amax = 448 x 2^E exactly (the m > 0.875 boundary from below,
    7.0 among them), 7.03125 x 2^e (from above), all zero (scale byte 1), values that are
    subnormal in e4m3 after scaling (ties included), and a plain dyadic block.  Every value is a
    bf16 number."""
    beta = np.zeros(-(-D // 32) * 32, np.float64)
    for j in range(len(beta) // 32):
        kind, e = j % 5, (j // 5) % 7 - 3
        blk = np.zeros(32)
        if kind == 0:
            amax = 7.0 * 2.0 ** e                       # = 448 x 2^(e - 6)
        elif kind == 1:
            amax = 7.03125 * 2.0 ** e
        elif kind == 2:
            amax = 0.0
        elif kind == 3:
            amax = 256.0                                # E = 0: the rest are e4m3 subnormals
            blk[:] = np.resize([1, 2, 3, 5, 7, 0.5, 1.5, 2.5, 6.5, 0.25, 0.75], 32) * 2.0 ** -9
        else:
            amax = float(rng.integers(9, 16)) / 8 * 2.0 ** e
        if kind in (0, 1, 4):
            top = 2.0 ** math.floor(math.log2(amax))
            blk[:] = rng.integers(1, 8, 32) / 8 * top * rng.choice((-1, 1), 32)
            assert (np.abs(blk) < amax).all()
        pos = j % 32
        if 32 * j + pos >= D:
            pos = D - 1 - 32 * j
        blk[pos] = amax if j % 2 == 0 or amax == 0 else -amax       # never -0: y = +0 + beta
        beta[32 * j:32 * j + 32] = blk
    beta = beta[:D].astype(f32)
    assert np.array_equal(bf16_value(bf16_bits(beta)), beta)
    return beta


# ------------------------------------------------------------------ finalize partials
class Partials:
    """vtd_layernorm_stats_finalize on hand-made partials, slot-major part[b rows + r] =
    (block mean, block M2).  Designed rows: block means m + j_b / 8 with sum(j_b) == 0 and M2
    small integers, so every step of the merge but the last division is exact: mean == m,
    rstd within 2^-22.  general=True: block means N(200, 2), M2 around 64 x 4."""

    def __init__(self, rows, slots, general=False, seed=0):
        self.rows, self.slots, self.D, self.general = rows, slots, 64 * slots, general
        rng = np.random.default_rng([seed, rows, slots, int(general)])
        if general:
            self.bm = rng.normal(200.0, 2.0, (slots, rows)).astype(f32)
            self.m2 = (64 * (4 + np.abs(rng.normal(0, 1, (slots, rows))))).astype(f32)
        else:
            m = np.resize(np.array([0.0, 16.0, -100.0, 256.0, 1000.5, -3.25]), rows)
            m = np.roll(m, seed)
            j = rng.integers(-16, 17, (slots, rows))
            j[-1] -= j.sum(axis=0)                      # sum(j_b) == 0, |j| <= 16 (slots - 1)
            assert (j.sum(axis=0) == 0).all() and np.abs(j).max() <= 16 * max(slots - 1, 1)
            self.exact_mean = m.astype(f32)
            self.bm = G.to_f32_exact(m[None, :] + j / 8)
            self.m2 = rng.integers(0, 200, (slots, rows)).astype(f32)
            assert 64 * (j * j).sum(axis=0).max() + self.m2.sum(axis=0).max() < LIMIT
        self.part = np.stack([self.bm, self.m2], axis=2).reshape(slots * rows, 2)

    def ref64(self):
        bm, m2 = self.bm.astype(np.float64), self.m2.astype(np.float64)
        mean = bm.mean(axis=0)
        var = (m2.sum(axis=0) + 64 * ((bm - mean) ** 2).sum(axis=0)) / self.D
        return mean, 1 / np.sqrt(var + EPS)

    def np32(self, part=None):
        """ln_merge_partials restated in fp32 numpy (sequential over the slots)."""
        p = (self.part if part is None else part).reshape(self.slots, self.rows, 2).astype(f32)
        m0 = p[0, :, 0]
        ds, q = np.zeros(self.rows, f32), np.zeros(self.rows, f32)
        for b in range(self.slots):
            ds = ds + (p[b, :, 0] - m0)
            q = q + p[b, :, 1]
        dmean = ds / f32(self.slots)
        between = np.zeros(self.rows, f32)
        for b in range(self.slots):
            dv = (p[b, :, 0] - m0) - dmean
            between = between + dv * dv
        var = (q + f32(64) * between) / f32(self.D)
        return np.stack([m0 + dmean, f32(1) / np.sqrt(var + f32(EPS))], axis=1).astype(f32)

    def check(self, got, rep=None, what="finalize"):
        got = np.asarray(got, f32)
        mean64, rstd64 = self.ref64()
        rep = rep or Report()
        assert np.isfinite(got).all(), f"{what}: not finite"
        emu = self.np32()
        if not self.general:
            bad = got[:, 0] != self.exact_mean
            assert not bad.any(), f"{what}: mean not exact at rows {np.argwhere(bad)[:6].ravel()}"
            ratio = np.abs(got[:, 1] - rstd64) / (U22 * rstd64)
            assert ratio.max() <= 1, f"{what}: rstd {ratio.max():.3f} of 2^-22 at {ratio.argmax()}"
            rep.designed = max(rep.designed, float(ratio.max()))
        else:
            for c, ref in ((0, mean64), (1, rstd64)):
                e = np.abs(emu[:, c] - ref)
                tol = 8 * e + 4 * ulp32(ref)
                err = np.abs(got[:, c] - ref)
                assert (err <= tol).all(), \
                    f"{what}: column {c} row {np.argmax(err - tol)} error {err.max():.3g}"
                for r in range(self.rows):              # one evaluation here: the kernel's order
                    rep.note_general(float(err[r]), float(e[r]), float(e[r]), float(ulp32(ref[r])) / 2)
        rep.rstd_total += self.rows
        rep.rstd_equal += int((got[:, 1] == emu[:, 1]).sum())
        return rep


# ------------------------------------------------------------------ fold
class Fold:
    """vtd_fold_layernorm on dyadic operands: w = i / 4 (|i| <= 8), gamma = 1 + j / 16,
    beta = j / 8, bias_in = i / 8.  w gamma = i (16 + j) / 64 with |i (16 + j)| <= 192 < 2^8 is a
    bf16 number, and the float64 sums are exact and fp32 numbers: equality throughout."""

    def __init__(self, N, K, ldw, ldo, seed=0):
        self.N, self.K, self.ldw, self.ldo = N, K, ldw, ldo
        rng = np.random.default_rng([seed, N, K])
        self.w = (rng.integers(-8, 9, (N, K)) / 4).astype(f32)
        self.gamma = (1 + rng.integers(-8, 9, K) / 16).astype(f32)
        self.beta = (rng.integers(-8, 9, K) / 8).astype(f32)
        self.bias_in = (rng.integers(-40, 41, N) / 8).astype(f32)

    def expected(self, with_bias, bf16):
        w64 = self.w.astype(np.float64)
        wo = G.to_f32_exact(w64 * self.gamma.astype(np.float64))
        if bf16:
            assert np.array_equal(bf16_value(bf16_bits(wo)), wo)
        w_out = np.zeros((self.N, self.ldo), f32)
        w_out[:, :self.K] = wo
        bias = w64 @ self.beta.astype(np.float64) + (self.bias_in if with_bias else 0.0)
        return w_out, G.to_f32_exact(bias), G.to_f32_exact(wo.astype(np.float64).sum(axis=1))


# ------------------------------------------------------------------ the tables of cases
LN_D = {
    "f32": dict(
        vec=(4, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048, 2052, 4096),
        generic=(1, 30, 63, 65, 4100),
        more=(8, 104, 128, 520, 776, 1032, 2056, 3072, 3968, 4088)),   # stats and MX widths
    "bf16": dict(
        vec=(8, 264, 520, 776, 1032, 2056),                            # D % 16 != 0
        ln16=(16, 1024, 1040, 2048, 2064, 3072, 4096),
        generic=(1, 30, 63, 65, 4100),
        more=(104, 128, 512, 3968, 4088)),
}
# (xdt, D, ldx or None, x_off, g_off)
LN_MISALIGNED = [
    ("f32", 256, None, 2, 0),       # x 8-byte aligned: generic (stats and MX refuse / go generic)
    ("f32", 256, None, 0, 1),       # gamma and beta 4-byte aligned: generic
    ("bf16", 1024, None, 4, 0),     # x 8- but not 16-byte aligned: layernorm_kernel NV 4
    ("bf16", 4096, None, 4, 0),     # ... NV 16
    ("bf16", 768, None, 4, 0),      # ... NV 3
    ("bf16", 512, 524, 0, 0),       # ldx % 8 != 0: NV 2
    ("bf16", 256, None, 1, 0),      # x 2-byte aligned: generic
    ("bf16", 256, None, 0, 1),
]


def ln_cases(xdt, rows):
    ds = sorted({d for group in LN_D[xdt].values() for d in group})
    cases = [Case(xdt, rows, D) for D in ds]
    cases += [Case(t, rows, D, ldx, xo, go) for t, D, ldx, xo, go in LN_MISALIGNED if t == xdt]
    return cases


Y_PADS = (0, 4, 100)


def y_pad(case, i):
    """ldy - D of the i-th output of a case: 0, 4, 100 in turn."""
    return Y_PADS[(i + case.D // 4 + case.rows) % 3]


def mx_kq(case, wide=False):
    kq = -(-case.D // 128) * 128
    return min(kq + 128, 4096) if wide else kq


# Kq > D: D = 104 in Kq = 128, and D = 3968 in Kq = 4096 (four whole blocks of padding)
MX_D = {"layernorm16_mx8_kernel": (128, 1024, 2048, 3072, 3968, 4096),
        "layernorm_mx8_kernel": (104, 776, 1032, 2056, 4088)}

MX_WIDE = (104, 1024, 3968)                     # also run with Kq one K-step wider


def calls(case):
    """Every library call the GPU module makes on one case, with its route."""
    out = []
    for i, o in enumerate(("f32", "bf16", "split")):
        P = case.D + y_pad(case, i)
        out.append(dict(entry="layernorm", out=o, P=P,
                        route=case.route("layernorm", P=P, out=o)))
    out.append(dict(entry="layernorm_stats", route=case.route("layernorm_stats")))
    for wide in (False, True):
        Kq = mx_kq(case, wide)
        r = case.route("layernorm_mx8", Kq=Kq)
        if r[0] != "invalid" and (not wide or case.D in MX_WIDE) and Kq >= case.D:
            out.append(dict(entry="layernorm_mx8", Kq=Kq, route=r))
    return out


def mx_const_cases():
    """Constant rows with the designed beta of mx_beta, on every branch of both fused kernels."""
    cases = []
    for xdt in ("f32", "bf16"):
        for rows in (1, 11):
            for D in sorted(MX_D["layernorm16_mx8_kernel"] + MX_D["layernorm_mx8_kernel"]):
                cases.append((xdt, rows, D, 0))
            cases.append(("bf16", rows, 1024, 4))       # misaligned: the 4-column kernel, NV 4
    out = []
    for xdt, rows, D, x_off in dict.fromkeys(cases):
        c = Case(xdt, rows, D, x_off=x_off, kinds=[("const", r % 3) for r in range(rows)])
        c.beta = mx_beta(D, np.random.default_rng([D, rows]))
        out.append(c)
    return out


FIN_UNROLLED = [(s, r, knob) for s in (12, 16) for r in (1, 300, 2500) for knob in (-1, 1, 3)]
FIN_GENERIC = [(s, r) for s in (1, 2, 8, 13, 64) for r in (1, 257)]
FOLD_SHAPES = ((5, 1, 1, 8), (200, 96, 96, 128), (7, 63, 70, 64), (9, 130, 130, 256))


# ------------------------------------------------------------------ the kernels' arithmetic
def _butterfly(s):
    """wave_sum: s += s[l ^ o], o = 32, 16, 8, 4, 2, 1 over the last axis (64 lanes)."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[..., lanes ^ o]).astype(f32)
    return s[..., 0]


def emulate(case, kernel, n, gamma=None, beta=None, fault=None):
    """(mean, rstd, y) [rows], [rows], [rows][D] in fp32 as kernel (with NV / NC n) computes
    them from the memory image -- NaN pads included, so a column read past D shows.  W columns per
    lane and chunk: 4 (layernorm_kernel, layernorm_mx8_kernel), 8 (ln_stats_kernel), 16 (the
    layernorm16 pair), 1 with n = ceil(D / 64) (the generic loops).  fault: a seeded defect."""
    D, rows = case.D, case.rows
    W = {"layernorm_kernel": 4, "layernorm_mx8_kernel": 4, "ln_stats_kernel": 8,
         "layernorm16_kernel": 16, "layernorm16_mx8_kernel": 16}.get(kernel, 1)
    if W == 1:
        n = -(-D // 64)
    xr = case.x_rows()
    span = n * 64 * W
    col = np.arange(span)
    start = col - col % W                                # first column of the lane's vector
    limit = D
    if fault == "mask_one_vector_short":
        limit = D - W
    if fault == "pad_column_read":
        limit = D + W
    live = start < limit
    assert span >= D, "the instantiation does not cover the row"
    xs = np.zeros((rows, span), np.float64)
    src = np.minimum(col, case.ldx - 1)
    xs[:, live] = xr[:, src[live]]
    xs = xs.astype(f32)
    if fault == "column_dropped":
        xs_sum = xs.copy()
        xs_sum[:, D // 2] = 0
    else:
        xs_sum = xs
    # lane l of chunk i owns columns W (64 i + l) .. + W - 1
    v = xs_sum.reshape(rows, n, 64, W)
    s = np.zeros((rows, 64), f32)
    for i in range(n):
        for g in range(0, W, 4):
            w = v[:, i, :, g:g + 4]
            if W == 1:
                s = (s + v[:, i, :, 0]).astype(f32)
            else:
                s = (s + (((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3])).astype(f32)
    cnt = f32(case.ldx if fault == "divide_by_ld" else D)
    with np.errstate(invalid="ignore"):
        mean = (_butterfly(s) / cnt).astype(f32)
        v = xs.reshape(rows, n, 64, W)
        lv = live.reshape(n, 64, W)
        q = np.zeros((rows, 64), f32)
        for i in range(n):
            for j in range(W):
                if fault == "one_pass_variance":
                    t = v[:, i, :, j] * v[:, i, :, j]
                else:
                    d = v[:, i, :, j] - mean[:, None]
                    t = d * d
                q = np.where(lv[i, :, j][None, :], (q + t).astype(f32), q)
        q = _butterfly(q)
        if fault == "one_pass_variance":
            var = (q / cnt - mean * mean).astype(f32)
        else:
            var = (q / cnt).astype(f32)
        if fault == "eps_outside_sqrt":
            rstd = (f32(1) / (np.sqrt(var) + f32(EPS))).astype(f32)
        else:
            rstd = (f32(1) / np.sqrt(var + f32(EPS))).astype(f32)
        g = (case.gamma if gamma is None else gamma).astype(f32)
        b = (case.beta if beta is None else beta).astype(f32)
        if fault == "gamma_shifted":
            g = np.roll(g, 1)
        y = ((xs[:, :D] - mean[:, None]) * rstd[:, None] * g[None, :] + b[None, :]).astype(f32)
    if fault == "rows_swapped" and rows > 1:
        mean, rstd, y = mean.copy(), rstd.copy(), y.copy()
        mean[[0, 1]], rstd[[0, 1]], y[[0, 1]] = mean[[1, 0]], rstd[[1, 0]], y[[1, 0]]
    return mean, rstd, y


def emulate_mx(y, Kq, fault=None):
    """The fused quantizer's tail: bf16-round, block amax, E8M0 exponent, e4m3 bytes."""
    rows, D = y.shape
    o = np.zeros((rows, Kq), f32)
    o[:, :D] = bf16_value(bf16_bits(y))
    blocks = o.astype(np.float64).reshape(rows, Kq // 32, 32)
    seen = blocks[..., :16] if fault == "amax_over_16" else blocks
    E = MX.block_exponent(np.abs(seen).max(axis=2))
    scaled = blocks * np.exp2(-E.astype(np.float64))[..., None]
    vals = MX.round_e4m3(np.clip(scaled, -448, 448))     # the conversion saturates
    return encode_e4m3(vals.reshape(rows, Kq)), (E + 127).astype(np.uint8)


FAULTS = ("column_dropped", "divide_by_ld", "one_pass_variance", "pad_column_read",
          "mask_one_vector_short", "gamma_shifted", "amax_over_16", "eps_outside_sqrt",
          "rows_swapped")
