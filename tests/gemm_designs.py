"""Designed GEMM operands whose product is exact in fp32 whatever the accumulation order.

A plain helper (no GPU, no torch) for tests/test_gemm_designs_host.py and
tests/test_gpu_gemm_designed.py.  C = A Bt^T with A [M][K], Bt [N][K]:

  base values
    "bf16" / "f32"  small signed integers (|a| <= 7, fewer for long K);
    "bf16x3"        a = h + l / 256 with h in +-{5, 6, 7}, l in {-3..3} (K <= 1280) or h = +-3,
                    l in {-1, 0, 1} (K <= 3072): bf16(a) == h and bf16(a - h) == l / 256 exactly
                    (h stays clear of powers of two, where a negative l would drop a into the
                    lower binade).  The operands are the split pieces, built with the numpy
                    restatement of the split below: A as [hi | lo], Bt as [hi | hi | lo].
  power-of-two dressing (exact)
    row m of A times 2^r[m], row n of Bt times 2^c[n] (r, c not monotone, spanning +-12 when
    nothing is added in the epilogue), and 64-wide K-block j of A times 2^t[j], of Bt times
    2^-t[j] (neighbouring blocks always differ).  Every output is then checked at its own
    scale, and a mix-up of rows, columns or K-blocks is off by a power of two.
  epilogue data, exact with act = NONE
    integer bias, rowadd (period, rowadd_ncols < N), residual, the LayerNorm fold with integer
    mean, power-of-two rstd varying with m and integer colsum -- each at the scale of the
    outputs it meets.

Expected output.  In bf16x3 the device sums THREE products, hi.hi + lo.hi + hi.lo; the lo.lo
term is dropped -- that is the mode's documented semantics (include/vtd.h "Split-bf16
operands"), so the expectation is  sum_k h_a h_b + (l_a h_b + h_a l_b) / 256  and NOT the
product of the f32 values.  It is computed in float64 from integers (exact: every sum is far
below 2^53) and cast to the output type.

The rule that makes the comparison exact: for every output, sum_k |term| plus the epilogue
addends stays below 2^24 units of the smallest term (`Design.check_rule`).  Every partial sum,
in any order and with or without fused multiply-adds, is then a multiple of that unit below
2^24 units: representable in fp32.  The value ranges are derived from K so that this holds and
make_design refuses a K where it cannot.
"""
import numpy as np

KBLOCK = 64
LIMIT = float(2 ** 24)
EPI_FIELDS = ("bias", "rowadd", "resid", "lnfold")


# ------------------------------------------------------------------ number formats
def bf16_bits(x):
    """f32 -> bf16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_bits(x32):
    """The split of include/vtd.h restated: hi = bf16(v), lo = bf16(v - hi), as bf16 bits."""
    x32 = np.ascontiguousarray(x32, np.float32)
    hi = bf16_bits(x32)
    lo = bf16_bits(x32 - bf16_value(hi))
    return hi, lo


def to_f32_exact(v64):
    """float64 -> f32, asserting the value is representable."""
    f = np.asarray(v64, np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v64), "expected value is not an fp32 number"
    return f


# ------------------------------------------------------------------ dressing
def exponents(n, span, rng):
    """n exponents in [-span, span], both ends present from n = 2 on, not monotone."""
    e = rng.integers(-span, span + 1, size=n)
    if n >= 2:
        e[0], e[n - 1] = span, -span
    if n >= 4:
        e[1], e[2] = -span + 1, span - 1         # up, down, up: not monotone
    return e.astype(np.int64)


def kblock_exponents(nblocks):
    """t[j] = (3 j + 1) mod 7 - 3: in [-3, 3], neighbouring blocks always differ."""
    return ((3 * np.arange(nblocks) + 1) % 7 - 3).astype(np.int64)


def base_range(mode, K):
    """(hs, lmax): the |h| values and the largest |l| for this K, or ValueError."""
    if mode == "bf16x3":
        if K <= 1280:
            return (5, 6, 7), 3          # per term <= 7 7 256 + 2 3 7 = 12586 units of 1/256
        if K <= 3072:
            return (3,), 1               # <= 3 3 256 + 2 3 = 2310
        raise ValueError(f"bf16x3 design: no value range keeps K = {K} under 2^24 units")
    for amax in (7, 5, 3, 2, 1):
        if K * amax * amax * 4 <= LIMIT:   # a factor 4 of room for the epilogue addends
            return tuple(range(1, amax + 1)), 0
    raise ValueError(f"integer design: K = {K} is too long")


class Design:
    """One designed problem.  a_op / b_op are the operands as the device stores them (uint16
    bf16 bits, or float32 for mode "f32"); a_read / b_read the K' wide rows the K loop sees
    ([hi | lo | hi] against [hi | hi | lo] in bf16x3), as float32."""

    def check_rule(self):
        """sum |terms| + |addends| < 2^24 units, every addend a multiple of the unit."""
        u1 = self.unit
        b1 = self.absacc.copy()
        e = self.epi
        if "lnfold" in e:
            mc = np.abs(np.outer(e["mean"], e["colsum"]))
            assert np.array_equal(mc / u1, np.round(mc / u1))
            b1 = b1 + mc
        assert (b1 < LIMIT * u1).all(), "accumulator stage breaks the 2^24 rule"
        rstd = e["rstd"][:, None] if "lnfold" in e else 1.0
        u2, b2 = u1 * rstd, b1 * rstd
        for a in self.addends():
            assert np.array_equal(a / u2, np.round(a / u2)), "addend is not a multiple of the unit"
            b2 = b2 + np.abs(a)
        assert (b2 < LIMIT * u2).all(), "epilogue stage breaks the 2^24 rule"
        return float((b2 / u2).max())

    def addends(self):
        e, out = self.epi, []
        if "bias" in e:
            out.append(np.broadcast_to(e["bias"][None, :], (self.M, self.N)))
        if "rowadd" in e:
            ra = np.zeros((self.M, self.N))
            ra[:, :e["rowadd_ncols"]] = e["rowadd"][np.arange(self.M) % e["rowadd_period"], None]
            out.append(ra)
        if "resid" in e:
            out.append(e["resid"])
        return out

    def expected(self):
        """float64 [M][N]: act(acc [LN fold] + bias + rowadd) + resid with act = NONE."""
        v, e = self.acc, self.epi
        if "lnfold" in e:
            v = (v - np.outer(e["mean"], e["colsum"])) * e["rstd"][:, None]
        for a in self.addends():
            v = v + a
        return v

    def lnstat(self):
        return np.stack([self.epi["mean"], self.epi["rstd"]], axis=1).astype(np.float32)


def make_design(mode, M, N, K, seed=0, epi=(), span=None, kreal=None):
    """mode "bf16" | "f32" | "bf16x3"; K the logical contraction length (bf16x3: the piece width
    P, vtd_gemm's K is 3 P), K % 64 == 0.  epi: names from EPI_FIELDS.  kreal < K: the columns
    [kreal, K) of both operands (of every piece) are the zero K-pad the producers write."""
    assert mode in ("bf16", "f32", "bf16x3") and K % KBLOCK == 0 and M > 0 and N > 0
    assert set(epi) <= set(EPI_FIELDS)
    rng = np.random.default_rng([seed, M, N, K, ("bf16", "f32", "bf16x3").index(mode)])
    hs, lmax = base_range(mode, K)
    d = Design()
    d.mode, d.M, d.N, d.K = mode, M, N, K
    d.Kcall = 3 * K if mode == "bf16x3" else K
    # an epilogue addend has one scale per column (bias) or per row (rowadd): the row / column
    # exponents stay narrow there so that it fits the 24-bit window of every output it meets
    rs, cs = (1, 2) if epi else (12, 12)
    if span is not None:
        rs = cs = span
    d.r, d.c = exponents(M, rs, rng), exponents(N, cs, rng)
    d.t = kblock_exponents(K // KBLOCK)
    tk = np.repeat(d.t, KBLOCK)

    def base(rows):
        h = rng.choice(hs, size=(rows, K)) * rng.choice((-1, 1), size=(rows, K))
        if mode != "bf16x3":
            h = h * (rng.random((rows, K)) < 0.9)            # some zeros among the integers
        l = rng.integers(-lmax, lmax + 1, size=(rows, K)) if lmax else np.zeros((rows, K), int)
        if kreal is not None:
            h[:, kreal:], l[:, kreal:] = 0, 0
        return h.astype(np.float64), l.astype(np.float64)

    d.ha, d.la = base(M)
    d.hb, d.lb = base(N)
    sa = np.exp2((d.r[:, None] + tk[None, :]).astype(np.float64))
    sb = np.exp2((d.c[:, None] - tk[None, :]).astype(np.float64))
    a64, b64 = (d.ha + d.la / 256) * sa, (d.hb + d.lb / 256) * sb
    a32, b32 = to_f32_exact(a64), to_f32_exact(b64)
    if mode == "bf16x3":
        ahi, alo = split_bits(a32)
        bhi, blo = split_bits(b32)
        # pieces split as designed
        assert np.array_equal(bf16_value(ahi), d.ha * sa) and np.array_equal(bf16_value(alo), d.la / 256 * sa)
        assert np.array_equal(bf16_value(bhi), d.hb * sb) and np.array_equal(bf16_value(blo), d.lb / 256 * sb)
        d.a_op = np.concatenate([ahi, alo], axis=1)
        d.b_op = np.concatenate([bhi, bhi, blo], axis=1)
        d.a_read = bf16_value(np.concatenate([ahi, alo, ahi], axis=1))
        d.b_read = bf16_value(d.b_op)
        u0 = 1.0 / 256
        units = 256 * d.ha @ d.hb.T + d.la @ d.hb.T + d.ha @ d.lb.T
        absu = 256 * np.abs(d.ha) @ np.abs(d.hb).T + np.abs(d.la) @ np.abs(d.hb).T + \
            np.abs(d.ha) @ np.abs(d.lb).T
    else:
        if mode == "bf16":
            d.a_op, d.b_op = bf16_bits(a32), bf16_bits(b32)
            assert np.array_equal(bf16_value(d.a_op), a32) and np.array_equal(bf16_value(d.b_op), b32)
        else:
            d.a_op, d.b_op = a32, b32
        d.a_read, d.b_read = a32, b32
        u0 = 1.0
        units = d.ha @ d.hb.T
        absu = np.abs(d.ha) @ np.abs(d.hb).T
    d.unit = np.exp2((d.r[:, None] + d.c[None, :]).astype(np.float64)) * u0
    d.acc, d.absacc = units * d.unit, absu * d.unit

    # ---- epilogue data
    e = d.epi = {}
    smax = 0
    if "lnfold" in epi:
        s = np.arange(M) % 3                                  # rstd = 1, 2, 4 by row
        smax = int(s.max())
        e["lnfold"] = True
        e["rstd"] = np.exp2(s.astype(np.float64))
        e["mean"] = rng.integers(-4, 5, size=M) * np.exp2(d.r.astype(np.float64))
        e["colsum"] = rng.integers(-4, 5, size=N) * np.exp2(d.c.astype(np.float64))
    # an addend met by rows of every r[m] (and rstd): a multiple of the largest unit among them
    eadd = float(d.r.max() + smax)
    if "bias" in epi:
        e["bias"] = rng.integers(-8, 9, size=N) * np.exp2(d.c + eadd)
    if "rowadd" in epi:
        e["rowadd_period"] = max(1, min(M, 5))
        e["rowadd_ncols"] = max(1, N - 1 - N // 3)
        e["rowadd"] = rng.integers(-8, 9, size=e["rowadd_period"]) * np.exp2(d.c.max() + eadd)
    if "resid" in epi:
        rs_ = e["rstd"][:, None] if "lnfold" in e else 1.0
        e["resid"] = rng.integers(-9, 10, size=(M, N)) * np.exp2((d.r[:, None] + d.c[None, :]).astype(np.float64)) * rs_
    d.check_rule()
    return d


def make_wgrad_design(mode, M, K, N, seed=0):
    """vtd_gemm_wgrad: dW[k][n] = sum_m X[m][k] G[m][n], db[n] = sum_m G[m][n], the contraction
    over the ROW index m (any M <= 1280).  mode "bf16" | "bf16x3" (operands [hi | lo]; dW from
    the three products, db from hi + lo).  Column k of X carries 2^r[k], column n of G 2^c[n],
    and 32-row step j of X 2^t[j], of G 2^-t[j] with t = j mod 3 - 1 (db sums G alone, so its
    terms keep the step scales: +-1 keeps sum |g| under 2^24 units)."""
    assert mode in ("bf16", "bf16x3") and 0 < M <= 1280
    rng = np.random.default_rng([seed, M, K, N, 7 + (mode == "bf16x3")])
    hs, lmax = base_range(mode, 1280)
    d = Design()
    d.mode, d.M, d.K, d.N = mode, M, K, N
    d.r, d.c = exponents(K, 12, rng), exponents(N, 12, rng)
    tm = (np.arange(M) // 32) % 3 - 1

    def base(cols):
        h = rng.choice(hs, size=(M, cols)) * rng.choice((-1, 1), size=(M, cols))
        l = rng.integers(-lmax, lmax + 1, size=(M, cols)) if lmax else np.zeros((M, cols), int)
        return h.astype(np.float64), l.astype(np.float64)

    hx, lx = base(K)
    hg, lg = base(N)
    sx = np.exp2((tm[:, None] + d.r[None, :]).astype(np.float64))
    sg = np.exp2((-tm[:, None] + d.c[None, :]).astype(np.float64))
    x32, g32 = to_f32_exact((hx + lx / 256) * sx), to_f32_exact((hg + lg / 256) * sg)
    if mode == "bf16x3":
        xh, xl = split_bits(x32)
        gh, gl = split_bits(g32)
        assert np.array_equal(bf16_value(xl), lx / 256 * sx) and np.array_equal(bf16_value(gl), lg / 256 * sg)
        d.x_op, d.g_op = (xh, xl), (gh, gl)
        u0 = 1.0 / 256
        units = 256 * hx.T @ hg + lx.T @ hg + hx.T @ lg
        absu = 256 * np.abs(hx).T @ np.abs(hg) + np.abs(lx).T @ np.abs(hg) + np.abs(hx).T @ np.abs(lg)
    else:
        d.x_op, d.g_op = (bf16_bits(x32),), (bf16_bits(g32),)
        u0 = 1.0
        units, absu = hx.T @ hg, np.abs(hx).T @ np.abs(hg)
    unit = np.exp2((d.r[:, None] + d.c[None, :]).astype(np.float64)) * u0
    assert (absu < LIMIT).all(), "dW breaks the 2^24 rule"
    d.dW = units * unit
    g64 = g32.astype(np.float64)
    db_unit = np.exp2(d.c.astype(np.float64) - 1) * u0           # the smallest step scale
    assert (np.abs(g64).sum(0) < LIMIT * db_unit).all(), "db breaks the 2^24 rule"
    d.db = g64.sum(0)
    to_f32_exact(d.dW), to_f32_exact(d.db)
    return d


# ------------------------------------------------------------------ output casts
def cast_f32(v64):
    return to_f32_exact(v64)


def cast_bf16(v64):
    """bf16 bits of the exact fp32 value, round to nearest even."""
    return bf16_bits(to_f32_exact(v64))


def cast_split(v64):
    """(hi bits, lo bits) of the split-bf16 output [hi | lo]."""
    return split_bits(to_f32_exact(v64))


def scatter_expected(v64, tokens):
    """The head's Reshape epilogue (vtd.h scatter_tokens): [B T][17] -> [B 17][T]."""
    rows, n = v64.shape
    assert n == 17 and rows % tokens == 0
    return v64.reshape(rows // tokens, tokens * 17).reshape(rows // tokens * 17, tokens)


# ------------------------------------------------------------------ fp32 emulation
ORDERS = ("forward", "reverse", "four_lanes", "blocks_reverse")


def emulate(a_read, b_read, order="forward"):
    """A GEMM with fp32 products and fp32 accumulation over K' in the given order."""
    a = np.ascontiguousarray(a_read, np.float32)
    b = np.ascontiguousarray(b_read, np.float32)
    K = a.shape[1]

    def run(ks):
        acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
        for k in ks:
            acc = acc + a[:, k:k + 1] * b[:, k][None, :]
        return acc

    if order == "forward":
        return run(range(K))
    if order == "reverse":
        return run(range(K - 1, -1, -1))
    if order == "four_lanes":                 # four interleaved partial sums, as MFMA k-groups
        p = [run(range(i, K, 4)) for i in range(4)]
        return (p[0] + p[1]) + (p[2] + p[3])
    if order == "blocks_reverse":             # 64-wide steps last to first, each summed forward
        acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
        for k0 in range(K - 64, -1, -64):
            acc = acc + run(range(k0, k0 + 64))
        return acc
    raise ValueError(order)


# ------------------------------------------------------------------ seeded faults
def _first_nonzero_lo(d):
    m, k = np.argwhere(d.la != 0)[0]
    return int(m), int(k)


def fault_drop_one_lo(d):
    """One lo element of A read as zero."""
    a = d.a_read.copy()
    m, k = _first_nonzero_lo(d)
    a[m, d.K + k] = 0
    return emulate(a, d.b_read)


def fault_lo_chunk_from_next_block(d):
    """A 16-byte chunk (8 elements) of A's lo piece taken from the neighbouring K-block."""
    a = d.a_read.copy()
    a[:, d.K + 8:d.K + 16] = a[:, d.K + 64 + 8:d.K + 64 + 16]
    return emulate(a, d.b_read)


def fault_piece_swap_at_wrap(d):
    """The first K-step after the wrap reads A's lo piece where it should return to hi."""
    a = d.a_read.copy()
    a[:, 2 * d.K:2 * d.K + 64] = a[:, d.K:d.K + 64]
    return emulate(a, d.b_read)


def fault_last_row_twice(d):
    """Row M - 1 of A used for row M - 2 (a clamp off by one)."""
    a = d.a_read.copy()
    a[d.M - 2] = a[d.M - 1]
    return emulate(a, d.b_read)


def fault_kblock_scale_from_neighbour(d):
    """K-block 0 of A carries block 1's scale."""
    a = d.a_read.copy()
    f = np.float32(2.0 ** float(d.t[1] - d.t[0]))
    for piece in range(a.shape[1] // d.K):
        a[:, piece * d.K:piece * d.K + 64] *= f
    return emulate(a, d.b_read)


def fault_tile_twice(d, tile=8):
    """One output tile computed twice (stored over its neighbour), the neighbour never."""
    out = emulate(d.a_read, d.b_read)
    out[:tile, tile:2 * tile] = out[:tile, :tile]
    return out


FAULTS = (fault_drop_one_lo, fault_lo_chunk_from_next_block, fault_piece_swap_at_wrap,
          fault_last_row_twice, fault_kblock_scale_from_neighbour, fault_tile_twice)
