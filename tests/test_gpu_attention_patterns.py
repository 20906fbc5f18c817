"""vtd_attention against fp64 on DESIGNED score patterns, every kernel variant.

The other attention tests draw Q, K and V from N(0, 1.5): scores with a standard deviation
of about 2.25 (natural units), diffuse softmax rows.  Three things that decide whether a
streaming-softmax kernel is right never happen there on purpose: the deferred rescale
(fires rarely, once, barely over its threshold of 8 log2 units), the identity of single keys
(a dropped, double-counted or mis-indexed key moves a diffuse row by ~|V| / N, far inside the
bf16 bound) and scores of large magnitude (the 4-wave bf16 kernel keeps its running max in
bf16).  Here the scores are constructed:

  scale = float32(ln 2), so that the launchers' scale * log2(e) is exactly 1.0f: scores are
  q.k in log2 units, and the kernels that pre-scale Q in bf16 get Q back unchanged;
  every element of Q and K is bf16-representable and a multiple of 1/4, every row's
  sum |q_d k_d| is below 2^20: products are multiples of 1/16, every partial sum is exact in
  fp32 whatever the accumulation order, so the comparison with fp64 measures the softmax
  and the P.V product, not the score accumulation.

Patterns (the sub-cases cycle with the query index, so one wave of 32 queries mixes them):
  ramp       score a_i * j, slopes a_i in {0, 1/2, -1/2, 1/4}: the up-ramps rescale in every
             chunk by different amounts per lane, flat lanes ride along, the down-ramp's P
             underflows in later chunks
  staircase  per-32-key levels [0, 7.5, 15, 15, 40, 33, 48.5, ...] times {1, 0, 1/2, -1}:
             growth below the rescale threshold, cumulative drift, a jump, a fall, and a
             last step (the ragged tail) 9.5 over everything before it
  spike      one key 24 over flat noise, at {0, 31, 32, 63, 64, N-33, N-2, N-1}: O ~ V[p]
  tie        two keys equally 24 over the rest: 0|N-1, 31|32, 63|64; O ~ (V[p0] + V[p1]) / 2;
             a double-counted clamped key N - 1 would give weights 1/3 : 2/3
  offset     flat noise + a common offset C = A * Bc per row, |C| <= 2^15
  offset_big C = +-65790, +-65884, +-65852: more than 128 away from its bf16 rounding, so a
             running max rounded to bf16 is off by 2^128 or more in P (inf, or l = 0)
(ramp keeps j = 256 (j >> 8) + (j & 255) in two dimensions: integers over 256 are not all
bf16 values.  spike / tie select their keys by one-hot dimensions 2.., a rank-1 score cannot
place a different key per query.)

The generator and its own checks need no GPU (from the repository root; a subset runs in
tests/test_attention_patterns_host.py):
  python -c "from tests.test_gpu_attention_patterns import check_generator; check_generator()"
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


LN2_F32 = np.float32(math.log(2.0))
# the launchers compute scale * 1.4426950408889634f in fp32: exactly 1 for scale = LN2_F32
assert LN2_F32 * np.float32(1.4426950408889634) == np.float32(1.0)

PATTERNS = ("ramp", "staircase", "spike", "tie", "offset", "offset_big")
B, H = 2, 2
RAMP_SLOPES = (0.0, 0.5, -0.5, 0.25)
STAIR_LEVELS = (0.0, 7.5, 15.0, 15.0, 40.0, 33.0, 48.5, 48.5, 56.0, 62.5)
STAIR_FACTORS = (1.0, 0.0, 0.5, -1.0)
PEAK = 24.0                                        # spike / tie height, = 4 * 6
OFFSET_PAIRS = ((128.0, 129.0), (181.0, 182.0))    # (A, Bc): C = 16512, 32942
# C = 65790 (254 over its bf16 rounding 65536), -65884 (164 over -66048), 65852 (196 under
# 66048); the factor -1 below gives each with the other sign
OFFSET_BIG_PAIRS = ((258.0, 255.0), (364.0, -181.0), (202.0, 326.0))
OFFSET_FACTORS = (1.0, -1.0, 0.0, 0.5)
TOL = {"f32": 2e-5, "x3": 2e-5, "bf16": 2e-2}      # the project's bounds, times max(1, max|O|)


def dkp_of(dk):
    return 32 if dk <= 32 else (64 if dk <= 64 else 128)


def bf16_round_np(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def is_bf16(x):
    x = np.ascontiguousarray(x, np.float32)
    return bool(((x.view(np.uint32) & 0xFFFF) == 0).all())


def spike_positions(N):
    return [int(min(max(p, 0), N - 1)) for p in (0, 31, 32, 63, 64, N - 33, N - 2, N - 1)]


def tie_positions(N):
    return [(min(p0, N - 1), min(p1, N - 1)) for p0, p1 in ((0, N - 1), (31, 32), (63, 64))]


def stair_levels(N):
    """One level per 32-key step; the last step (the ragged tail when N % 32 != 0) lies 9.5
    over every earlier one: a rescale in the last chunk for 32- and 64-key chunks alike."""
    n = (N + 31) // 32
    lv = list(STAIR_LEVELS[:n])
    if n > 1:
        lv[-1] = max(lv[:-1]) + 9.5
    return lv


def attention_ref(q, k, v, scale):
    """softmax(scale * q.k) v in fp64; q, k, v [B][N][H][dk]."""
    s = np.einsum("bqhd,bkhd->bhqk", q.astype(np.float64), k.astype(np.float64)) * float(scale)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v.astype(np.float64))


def pack_qkv(q, k, v, dkp):
    """[B][N][H][dk] x 3 -> the qkv matrix [B*N][3 H dkp + 8] (columns dk..dkp of a head zero)."""
    Bn, N, Hn, dk = q.shape
    ld = 3 * Hn * dkp + 8
    qkv = np.zeros((Bn * N, ld), np.float32)
    for part, m in enumerate((q, k, v)):
        for h in range(Hn):
            c0 = part * Hn * dkp + h * dkp
            qkv[:, c0:c0 + dk] = m[:, :, h, :].reshape(Bn * N, dk)
    return qkv


@functools.lru_cache(maxsize=4)
def make_case(pattern, N, dk):
    """(qkv fp32 [B*N][ld], expected fp64 [B][N][H][dk], extra tolerance, scores fp64
    [B][H][N][N] in log2 units) of one pattern.  Asserts what the pattern relies on."""
    rng = np.random.default_rng([PATTERNS.index(pattern), N, dk])
    q = np.zeros((B, N, H, dk), np.float32)
    k = np.zeros((B, N, H, dk), np.float32)
    v = bf16_round_np(rng.normal(0, 1, size=(B, N, H, dk)).astype(np.float32))
    i = np.arange(N)
    cyc = i % 32                                   # position in the wave's 32 queries
    # first noise dimension (staircase: one dimension, noise of +-1/4 at most, so that its
    # growth of 7.5 stays under the rescale threshold of 8)
    nd0 = {"spike": 2 + 8, "tie": 2 + 3, "staircase": dk - 1}.get(pattern, 2)
    q[..., nd0:] = 0.5 * rng.integers(-1, 2, size=(B, N, H, dk - nd0))
    k[..., nd0:] = 0.5 * rng.integers(-1, 2, size=(B, N, H, dk - nd0))
    extra = 0.0
    if pattern == "ramp":
        a = np.asarray(RAMP_SLOPES, np.float32)[cyc % 4]
        q[..., 0] = a[None, :, None]
        q[..., 1] = a[None, :, None]
        k[..., 0] = (i & 255)[None, :, None]
        k[..., 1] = (256 * (i >> 8))[None, :, None]
    elif pattern == "staircase":
        q[..., 0] = np.asarray(STAIR_FACTORS, np.float32)[cyc % 4][None, :, None]
        k[..., 0] = np.asarray(stair_levels(N), np.float32)[i // 32][None, :, None]
    elif pattern == "spike":
        pos = spike_positions(N)
        q[:, i, :, 2 + cyc % 8] = 4.0
        for c, p in enumerate(pos):
            k[:, p, :, 2 + c] = 6.0
    elif pattern == "tie":
        sets = tie_positions(N)
        q[:, i, :, 2 + cyc % 3] = 4.0
        for c, (p0, p1) in enumerate(sets):
            for p in (p0, p1):
                k[:, p, :, 2 + c] = 6.0
                k[:, p, :, nd0:] = 0.0             # no noise on a tied key: the tie is exact
    else:
        pairs = OFFSET_PAIRS if pattern == "offset" else OFFSET_BIG_PAIRS
        f = np.asarray(OFFSET_FACTORS, np.float32)[cyc % 4]
        cmax = 0.0
        for b in range(B):
            for h in range(H):
                A, Bc = pairs[(b * H + h) % len(pairs)]
                q[b, :, h, 1] = A * f
                k[b, :, h, 1] = Bc
                cmax = max(cmax, abs(A * Bc))
        # A kernel that multiplies by scale_log2 AFTER the dot product (the f32, persistent,
        # LDS-DMA and split-bf16 kernels) rounds each score C + noise_j once more in fp32: up
        # to ulp(C) / 2 per key, so two keys' scores move apart by at most ulp(C) (log2
        # units), P_j / P_k by a factor within exp(ln2 * ulp(C)), every normalised weight by
        # at most ln2 * ulp(C) of itself, and O by at most ln2 * ulp_f32(|C|) * max |V|.
        # (With this test's scale the product is by 1.0f and exact; the term is the bound of
        # the operation, not of what the kernels happen to do.)
        extra = math.log(2.0) * float(np.spacing(np.float32(cmax))) * float(np.abs(v).max())

    # ---- what every pattern relies on: bf16 inputs, exact fp32 scores
    assert is_bf16(q) and is_bf16(k) and is_bf16(v)
    assert (q * 4 == np.round(q * 4)).all() and (k * 4 == np.round(k * 4)).all()
    mag = np.einsum("bqhd,bkhd->bhqk", np.abs(q).astype(np.float64), np.abs(k).astype(np.float64))
    assert mag.max() < 2.0 ** 20
    s = np.einsum("bqhd,bkhd->bhqk", q.astype(np.float64), k.astype(np.float64))
    assert (s * 16 == np.round(s * 16)).all()
    exp = attention_ref(q, k, v, LN2_F32)
    bound = TOL["bf16"] * max(1.0, np.abs(exp).max())          # the loosest bound in use

    if pattern == "spike":
        # the peak dominates: O is V[p] to well inside the f32 bound's order of magnitude
        for c, p in enumerate(spike_positions(N)):
            rows = i[cyc % 8 == c]
            assert np.abs(exp[:, rows] - v[:, p][:, None].astype(np.float64)).max() < 1e-2
    if pattern == "tie":
        for c, (p0, p1) in enumerate(tie_positions(N)):
            rows = i[cyc % 3 == c]
            mid = 0.5 * (v[:, p0].astype(np.float64) + v[:, p1].astype(np.float64))
            assert np.abs(exp[:, rows] - mid[:, None]).max() < 1e-2
            if p0 != p1:
                # weights 1/3 : 2/3 instead of 1/2 : 1/2 would move O by |V[p0] - V[p1]| / 6:
                # visible for the V drawn, in every (image, head)
                moved = np.abs(v[:, p0].astype(np.float64) - v[:, p1].astype(np.float64)) / 6
                assert (moved.max(axis=-1) > 2 * bound).all()
    if pattern == "offset_big":
        # the hazard is reached: the rows with factor +-1 have a max more than 128 log2 units
        # away from its bf16 rounding, on both sides
        rm = s.max(axis=-1)[:, :, np.isin(cyc % 4, (0, 1))].astype(np.float32)
        res = rm - bf16_round_np(rm)
        assert (np.abs(res) > 128).all() and res.max() > 128 and res.min() < -128
    return pack_qkv(q, k, v, dkp_of(dk)), exp, extra, s


def rescales(s_wave, kc):
    """The deferred-rescale rule (`ballot(mx > m_run + 8)`, all 32 lanes rescale when one
    asks) emulated over the scores [32 or fewer queries][N] of one wave: per chunk after the
    first, whether it fires, and the largest growth of a lane's chunk max over its running
    max."""
    n = s_wave.shape[1]
    m_run = s_wave[:, :kc].max(axis=1)
    fired, growth = [], []
    for c0 in range(kc, n, kc):
        mx = s_wave[:, c0:c0 + kc].max(axis=1)
        growth.append(float((mx - m_run).max()))
        fired.append(bool((mx > m_run + 8).any()))
        if fired[-1]:
            m_run = np.maximum(m_run, mx)
    return fired, growth


def check_generator(shapes=None):
    """Every (pattern, dk, N) the tests use (or the (dk, N) given): make_case's assertions
    (exact scores, the tie error visible, the bf16 hazard reached), and the rescale behaviour
    each pattern is for."""
    shapes = sorted(shapes or {(r[3], r[4]) for r in ROWS})
    for pattern in PATTERNS:
        for dk, N in shapes:
            qkv, exp, extra, s = make_case(pattern, N, dk)
            assert np.isfinite(exp).all()
            if N <= 64:
                continue
            for kc in (32, 64):
                fired, growth = rescales(s[0, 0, :32], kc)
                if pattern == "ramp":
                    # the 1/2 slope alone grows by 16 per 32 keys: every full chunk rescales
                    # (a short ragged tail may not), the wave's lanes by very different amounts
                    assert all(fired[:-1]) and len(fired) == (N + kc - 1) // kc - 1
                    if N == 300:
                        assert sum(fired) >= {32: 8, 64: 4}[kc]
                if pattern == "staircase":
                    assert fired[-1]                           # in the (ragged) last chunk
                    if kc == 64 and N > 128:
                        # 64-key chunks: 15 after 7.5, growth just under the threshold
                        assert not fired[0] and 7 <= growth[0] <= 8
                    if kc == 32 and N > 96:
                        # 32-key chunks: 7.5 (no rescale), then 15 over a max still at 0
                        assert not fired[0] and fired[1] and growth[1] >= 14.5
                if pattern == "spike":
                    assert any(fired)      # (a tie's second key never grows over its first)
    print(f"check_generator: {len(PATTERNS)} patterns x {len(shapes)} shapes ok")


# ---------------------------------------------------------------------------------------
# the kernels: (name, mode, knob, dk, N, diagnostic-build-only)
def _rows():
    rows = []
    for dk in (20, 64, 100):
        for N in (100, 300):
            rows.append(("f32", "f32", -1, dk, N, False))
    for N in (33, 100, 128):
        rows.append(("bf16-4wave", "bf16", -1, 64, N, False))
    for dk in (20, 100):
        for N in (33, 100, 128, 200):
            rows.append(("bf16-4wave", "bf16", -1, dk, N, False))
    rows += [("bf16-8wave", "bf16", -1, 64, 300, False), ("bf16-8wave", "bf16", 2, 64, 196, False),
             ("bf16-8wave", "bf16", 2, 64, 131, False), ("bf16-8wave", "bf16", 3, 64, 100, False),
             ("bf16-8wave", "bf16", 3, 20, 100, False)]
    for N in (131, 196, 203, 256):
        rows.append(("bf16-persistent", "bf16", -1, 64, N, False))
    for N in (196, 208):
        rows.append(("bf16-ps16", "bf16", 5, 64, N, True))
    for N in (100, 300):
        rows.append(("bf16-ldsdma", "bf16", 6, 64, N, False))
    for dk in (20, 64, 100):
        for N in (100, 300):
            rows.append(("bf16-generic", "bf16", 1, dk, N, False))
    for dk in (20, 64, 100):
        for N in (33, 100, 300):
            rows.append(("bf16x3", "x3", -1, dk, N, False))
    for N in (33, 100, 300):
        rows.append(("bf16x3-kc64", "x3", 10, 64, N, False))
    return rows


ROWS = _rows()
# one (pattern, shape) after another, so that make_case's small cache serves every kernel of it
CASES = sorted(((p,) + r for p in PATTERNS for r in ROWS),
               key=lambda c: (PATTERNS.index(c[0]), c[4], c[5]))


def run_attention(L, cuda, mode, knob, qkv, N, dk, scale):
    """vtd_attention on qkv [B*N][ld] -> O fp64 [B][N][H][dkp]; asserts that the columns past
    the heads (slack of ldo) keep their fill."""
    dkp = dkp_of(dk)
    inner = H * dkp
    ld = qkv.shape[1]
    if mode == "x3":
        P = inner + 64
        out = torch.full((B * N, 2 * P), -1, dtype=torch.int16, device=cuda)
        qkv_d = torch.from_numpy(qkv).to(cuda)
        code, ldo = L.BF16X3, 2 * P
    else:
        tdt = torch.float32 if mode == "f32" else torch.bfloat16
        qkv_t = torch.from_numpy(qkv).to(tdt)
        ldo = inner + 16
        out = torch.full((B * N, ldo), float("nan"), dtype=tdt, device=cuda)
        qkv_d = qkv_t.to(cuda)
        code = L.F32 if mode == "f32" else L.BF16
    with L.knob(L.KNOB_ATTN_VARIANT, knob):
        L.check(L.lib.vtd_attention(qkv_d.data_ptr(), B, N, H, dkp, ld, float(scale),
                                    out.data_ptr(), ldo, code, L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    if mode == "x3":
        got = out.cpu().view(torch.int16).numpy().view(np.uint16)
        assert (got[:, inner:P] == 0xFFFF).all() and (got[:, P + inner:] == 0xFFFF).all()
        hi = (got[:, :inner].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        lo = (got[:, P:P + inner].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        o = hi + lo
    else:
        o = out.cpu().double().numpy()
        assert np.isnan(o[:, inner:]).all()                    # nothing written past the heads
        o = o[:, :inner]
    return o.reshape(B, N, H, dkp)


@pytest.mark.parametrize("pattern,kernel,mode,knob,dk,N,diag", CASES)
def test_attention_pattern(L, cuda, pattern, kernel, mode, knob, dk, N, diag):
    """Every pattern on every kernel, against fp64 of the same (bf16-exact) inputs."""
    if diag and not hasattr(L.lib, "vtd_diag_build"):
        pytest.skip("the 16-query persistent kernel is in the diagnostic build only (make diag)")
    qkv, exp, extra, _ = make_case(pattern, N, dk)
    if mode == "bf16":
        assert (torch.from_numpy(qkv).to(torch.bfloat16).float().numpy() == qkv).all()
    got = run_attention(L, cuda, mode, knob, qkv, N, dk, LN2_F32)
    tol = TOL[mode] * max(1.0, np.abs(exp).max()) + extra
    finite = np.isfinite(got).all()
    err = np.abs(got[..., :dk] - exp).max() if finite else float("inf")
    print(f"{pattern} {kernel} knob {knob} dk {dk} N {N}: finite {finite}, "
          f"max err {err:.3e}, tol {tol:.3e}")
    assert finite
    assert err < tol
    assert (got[..., dk:] == 0).all()


BF16_SHAPES = sorted({(r[3], r[4]) for r in ROWS if r[1] == "bf16"})


@functools.lru_cache(maxsize=2)
def make_random(N, dk):
    """The other attention tests' data: Q, K, V ~ N(0, 1.5), rounded to bf16."""
    g = np.random.default_rng(N * 10 + dk)
    q, k, v = (bf16_round_np(g.normal(0, 1.5, size=(B, N, H, dk)).astype(np.float32))
               for _ in range(3))
    return pack_qkv(q, k, v, dkp_of(dk)), attention_ref(q, k, v, 1.0 / math.sqrt(dk))


@pytest.mark.parametrize("knob", [1, 2, 3])
@pytest.mark.parametrize("dk,N", BF16_SHAPES)
def test_attention_random_bf16_forced_kernels(L, cuda, dk, N, knob):
    """N(0, 1.5) data on the kernels no other test compares with fp64: the generic bf16 kernel
    (knob 1), the streaming kernel as knob 2 picks it (8 waves from N = 129) and the 8-wave
    kernel at any N (knob 3)."""
    qkv, exp = make_random(N, dk)
    got = run_attention(L, cuda, "bf16", knob, qkv, N, dk, 1.0 / math.sqrt(dk))
    assert np.isfinite(got).all()
    assert np.abs(got[..., :dk] - exp).max() < TOL["bf16"] * max(1.0, np.abs(exp).max())
    assert (got[..., dk:] == 0).all()
