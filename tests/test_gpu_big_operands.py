"""Every row-indexed kernel on operands whose last rows lie more than 2^31 and 2^32 bytes from
their base (tests/big_operands.py: the arena, the periodic row data, the comparisons).

Each case hands an entry point tall operands [rows][pitch] from the start of the arena's span --
262,477 rows of 16 KiB, or 524,621 rows of 8 KiB where the entry point writes its whole leading
dimension -- whose row m is row m mod 1021 of a designed table, and asserts
  (a) over ALL rows, on the device: the GEMM family equals the float64-derived expectation as
      numbers; the per-row and per-image kernels equal, bit for bit, a run of the same entry point
      on one period of rows (an invariance check, paired with (b));
  (b) on four 512-row windows (first, across byte 2^31, across byte 2^32, last), on the host: the
      existing float64 oracles with their existing bars;
  (c) no byte of the arena outside what the contract writes changed, no input element changed;
  (d) the route each case means to take.
A failure names the first bad (row, column), its byte offset and the alias row whose value was
found there (a row 2^31 / 2^32 bytes or elements before it, or the clamped last row).

An entry point that writes its whole leading dimension (vtd_split_bf16x3, vtd_act_forward,
vtd_act_grad, vtd_layernorm: pad columns up to ld are written as zero) cannot share rows with
its input, so it runs twice: tall input with a small side output, and tall output (8 KiB rows)
with a small side input.  The other entry points take input and output in one row at different
column offsets: both cross 2^31 and 2^32 bytes in one call.  vtd_gemm_wgrad has no tall output.

vtd_dropout_apply is not row-invariant by design (the Philox counter carries the row): over all
rows every output is 0 or x * 1 / (1 - rate) and the kept fraction is the rate's; the mask itself
is checked on the windows against tests/dropout_oracle.py.

The module allocates 8.125 GiB once; with less than that plus 2 GiB free it skips (the only skip).
Measured on an MI355X: 58 tests, none skipped, the module in 7.7 s (10.1 s with collection), the
longest test 0.7 s (the first, which warms the device up), every other under 0.5 s.  Worst
figures of the window checks, as the tests print them: MX-fp8 GEMM 1.1e-4 (bar 5e-4); activation
derivative 7.7e-6 (bar 1e-5); LayerNorm backward 0.106 / 0.002 / 0.001 of the dx / dgamma / dbeta
bars; attention forward at most 0.38 of its tolerance; attention gradients 0.0025 (bf16, bar
2^-7) and 4.0e-6 (bf16x3, bar 2^-15) of their magnitudes.  No kernel failed.
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import attention_grad_oracle as AG
from tests import big_operands as BO
from tests import dropout_oracle as DO
from tests import gemm_designs as G
from tests import head_grad_oracle as H
from tests import ln_designs as LD
from tests import ln_grad_oracle as LG
from tests.test_gpu_act_grad import grid_values
from tests.test_gpu_attention_patterns import LN2_F32, TOL as ATT_TOL, make_case
from tests.test_gpu_gemm_designed import knobs, route

pytestmark = pytest.mark.gpu
P, PITCH, TIED = BO.P, BO.PITCH, BO.PITCH_TIED
M16, M8 = BO.tall_rows(PITCH), BO.tall_rows(TIED)
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def arena(cuda):
    free, total = torch.cuda.mem_get_info()
    need = BO.ARENA_BYTES + BO.HEADROOM
    if free < need:
        pytest.skip(f"big operands need {need / 2**30:.1f} GiB free (arena "
                    f"{BO.ARENA_BYTES / 2**30:.2f} GiB + 2 GiB), the device has "
                    f"{free / 2**30:.1f} of {total / 2**30:.1f} GiB")
    a = BO.Arena(cuda)
    yield a
    a.free()
    print(f"big operands: module wall time {time.perf_counter() - T0:.1f} s")


# ------------------------------------------------------------------ small helpers
def bits(a, dev):
    """numpy array -> device tensor of its bits (int32 / int16 / uint8)."""
    a = np.ascontiguousarray(a)
    v = {4: np.int32, 2: np.int16, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(v).copy()).to(dev)


def f32_of(b16):
    return (np.asarray(b16).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def side(dev, rows, ld, dtype, fill=BO.FILL_OUT):
    """A small side buffer [rows][ld] with 64 KiB of fill before and behind: (tensor, view)."""
    esz = torch.empty((), dtype=dtype).element_size()
    g = 65536 // esz
    t = torch.empty(rows * ld + 2 * g, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(fill)
    return t, t[g:g + rows * ld].view(rows, ld)


def side_guards_ok(t, fill=BO.FILL_OUT):
    g = 65536
    raw = t.view(torch.uint8)
    return bool((raw[:g] == fill).all()) and bool((raw[-g:] == fill).all())


def gather_rows(table, index, chunk=1 << 16):
    """table[index] for a device table, written chunk by chunk into a new tensor."""
    out = torch.empty((len(index),) + tuple(table.shape[1:]), dtype=table.dtype, device=table.device)
    for a in range(0, len(index), chunk):
        out[a:a + chunk] = table[index[a:a + chunk]]
    return out


def equal_rows(got, table, index, what, M, pitch, esz, chunk=1 << 16):
    """got [M][w] (a side output) == table[index] bit for bit, all rows, on the device."""
    bad = torch.zeros((), dtype=torch.int64, device=got.device)
    for a in range(0, M, chunk):
        bad += (got[a:a + chunk] != table[index[a:a + chunk]]).sum()
    if int(bad.item()):
        g, w = got.cpu().numpy(), table.cpu().numpy()
        BO.check_rows(g, np.arange(M), M, pitch, esz, w, index.cpu().numpy(), what, numbers=False)


def read_windows(arena, field, piece=0):
    return np.concatenate([arena.window(field, a, b, piece) for _, a, b in
                           BO.windows(arena.M, arena.pitch)])


def index_dev(index, dev):
    return torch.from_numpy(np.asarray(index)).to(dev)


ROW_INDEX16, ROW_INDEX8 = BO.row_index(M16), BO.row_index(M8)


# ------------------------------------------------------------------ vtd_gemm and vtd_gemm_splitk
A_COL, OUT_COL, RES_COL = 0, 1024, 4096
# id: (mode, N, K, out, fast epilogue, residual, knobs, route, ksplit)
GEMM_CASES = {
    "skinny-bf16-f32": ("bf16", 17, 64, "f32", False, None, {}, "skinny", 0),
    "skinny-x3-split": ("bf16x3", 17, 64, "split", False, None, {}, "skinny", 0),
    "skinny-x3-bf16-resid": ("bf16x3", 17, 64, "bf16", False, "separate", {}, "skinny", 0),
    "tn128-bf16-bf16-inplace": ("bf16", 17, 64, "bf16", False, "alias", {"SKINNY": 0}, "tn128", 0),
    "tn128-x3-f32-resid": ("bf16x3", 33, 64, "f32", False, "separate", {"SKINNY": 0}, "tn128", 0),
    "tn128-f32": ("f32", 72, 64, "f32", False, "alias", {"F32_PP2": 0}, "tn128", 0),
    "pp2-generic-bf16-f32": ("bf16", 255, 64, "f32", False, None, {}, "pp2", 0),
    "pp2-generic-x3-split": ("bf16x3", 130, 64, "split", False, None, {}, "pp2", 0),
    "pp2-generic-bf16-bf16-inplace": ("bf16", 72, 64, "bf16", False, "alias", {"GEMM_TR": 0},
                                      "pp2", 0),
    "pp2-fast-bf16-bf16-inplace": ("bf16", 256, 64, "bf16", True, "alias", {}, "pp2", 0),
    "pp2-fast-bf16-f32-resid-tr1": ("bf16", 256, 64, "f32", True, "separate", {"GEMM_TR": 1},
                                    "pp2", 0),
    "pp2-fast-x3-f32-resid": ("bf16x3", 256, 64, "f32", True, "separate", {}, "pp2", 0),
    "pp2-fast-x3-split": ("bf16x3", 264, 64, "split", True, None, {}, "pp2", 0),
    "f32-pp2": ("f32", 72, 64, "f32", True, "separate", {}, "f32-pp2", 0),
    "splitk-bf16-f32": ("bf16", 72, 128, "f32", True, None, {}, "pp2", 2),
    "splitk-x3-bf16-inplace": ("bf16x3", 68, 64, "bf16", False, "alias", {}, "pp2", 2),
}


def gemm_tables(d, out):
    """The P-row expectation of design d in the output form: [(np bits [P][N], as float32)]."""
    want64 = d.expected()
    if out == "f32":
        return [G.cast_f32(want64)]
    if out == "bf16":
        return [G.cast_bf16(want64)]
    return list(G.cast_split(want64))


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm(L, cuda, arena, case):
    mode, N, K, out, fast, resid, kn, want_route, ksplit = GEMM_CASES[case]
    M = M16
    fields = (("bias",) if fast else ()) + (("resid",) if resid else ())
    d = G.make_design(mode, P, N, K, epi=fields)
    d.check_rule()
    assert route(mode, M, N, d.Kcall, kn.get("SKINNY", -1), kn.get("F32_PP2", -1)) == want_route
    in_dt = "f32" if mode == "f32" else "bf16"
    out_dt = "f32" if out == "f32" else "bf16"
    esz_in, esz_out = (4 if mode == "f32" else 2), (4 if out == "f32" else 2)
    A = BO.Field("A", "in", in_dt, [BO.Piece(A_COL, d.a_op.shape[1])], bits(d.a_op, cuda), band=512)
    BO.assert_distinct(d.a_op, ROW_INDEX16, M, PITCH, esz_in)
    tabs = gemm_tables(d, out)
    ldo = PITCH // esz_out
    pieces = [BO.Piece(OUT_COL, N)] + ([BO.Piece(OUT_COL + ldo, N)] if out == "split" else [])
    ep = L.VtdEpilogue()
    flds = [A]
    if resid:
        r = d.epi["resid"].astype(np.float32)
        r = r if out == "f32" else G.bf16_bits(r)
    if resid == "alias":
        O = BO.Field("out", "inout", out_dt, pieces, bits(r, cuda))
        ep.resid, ep.ldr = arena.ptr(OUT_COL), ldo
    else:
        O = BO.Field("out", "out", out_dt, pieces)
        if resid:
            R = BO.Field("resid", "in", out_dt, [BO.Piece(RES_COL, N)], bits(r, cuda),
                         band=-(-N * esz_out // 64) * 64 + 64)
            flds.append(R)
            ep.resid, ep.ldr = arena.ptr(RES_COL), ldo
    flds.append(O)
    arena.stage(PITCH, M, flds, ROW_INDEX16)
    bt = bits(d.b_op, cuda)
    keep = [bt]
    if fast:
        bias = torch.from_numpy(d.epi["bias"].astype(np.float32)).to(cuda)
        keep.append(bias)
        ep.bias = bias.data_ptr()
    ep.out, ep.ldo = arena.ptr(OUT_COL), ldo
    ep.out_dtype = {"f32": L.F32, "bf16": L.BF16, "split": L.BF16X3}[out]
    dtype = {"bf16": L.BF16, "f32": L.F32, "bf16x3": L.BF16X3}[mode]
    lda = PITCH // esz_in
    with knobs(L, **kn):
        if ksplit:
            pt, part = side(cuda, ksplit * M, N, torch.float32)
            L.check(L.lib.vtd_gemm_splitk(M, N, d.Kcall, arena.ptr(A_COL), lda, bt.data_ptr(),
                                          d.b_op.shape[1], dtype, ctypes.byref(ep), part.data_ptr(),
                                          ksplit * M * N * 4, ksplit, L.stream_ptr()), case)
        else:
            L.check(L.lib.vtd_gemm(M, N, d.Kcall, arena.ptr(A_COL), lda, bt.data_ptr(),
                                   d.b_op.shape[1], dtype, ctypes.byref(ep), L.stream_ptr()), case)
    torch.cuda.synchronize()
    # (a) all rows, as numbers; (b) the windows against the same float64-derived expectation
    rows = BO.window_rows(M, PITCH)
    for i, tab in enumerate(tabs):
        arena.compare(O, bits(tab, cuda), f"{case} piece {i}", numbers=True, piece=i)
        got = read_windows(arena, O, i)
        as_num = (lambda x: x.view(np.float32)) if out == "f32" else f32_of
        BO.check_rows(as_num(got), rows, M, PITCH, esz_out, as_num(tab), ROW_INDEX16,
                      f"{case} windows piece {i}", col_byte=pieces[i].col)
    arena.assert_guards(case)
    if ksplit:
        assert side_guards_ok(pt), "the split-K partials' guards were touched"
    last = (M - 1) * PITCH + pieces[-1].col + N * esz_out
    assert last > 1 << 32 and (M - 1) * PITCH + d.a_op.shape[1] * esz_in > 1 << 32
    if out == "split":
        assert M * ldo > 1 << 31, "the split output has more than 2^31 elements"


def test_gemm_mx8(L, cuda, arena):
    """vtd_gemm_mx8 with a tall e4m3 A (16 KiB rows of 1-byte elements, K = 128) and its scale
    rows [1][sa_rows][4].  The scaled MFMA's reduction is not known to be exact: all rows equal a
    run of the same entry point on the 1021 rows bit for bit, and the windows meet the dequantized
    float64 product within test_gpu_mx8.py's bound (5e-4 of max(1, |ref|), fp32 output)."""
    from oracle import mx8 as MX
    M, N, K = M16, 136, 128
    g = torch.Generator().manual_seed(5)
    a32 = torch.randn(P, K, generator=g).to(torch.bfloat16).float()
    w32 = torch.randn(N, K, generator=g) / K ** 0.5

    def quant(x, s_rows):
        rows = x.shape[0]
        q = torch.zeros((rows, K), dtype=torch.uint8, device=cuda)
        s = torch.full((s_rows, 4), 127, dtype=torch.uint8, device=cuda)
        xd = x.to(cuda)
        L.check(L.lib.vtd_quantize_mx8(xd.data_ptr(), L.F32, rows, K, K, K, q.data_ptr(), K,
                                       s.data_ptr(), s_rows, L.stream_ptr()), "quantize_mx8")
        torch.cuda.synchronize()
        return q, s

    sp_rows, sb_rows = -(-P // 4) * 4, -(-N // 4) * 4
    qa, sa = quant(a32, sp_rows)
    qb, sb = quant(w32, sb_rows)
    BO.assert_distinct(qa.cpu().numpy(), ROW_INDEX16, M, PITCH, 1)
    bias = torch.zeros(N, device=cuda)

    def run(Mr, a_ptr, lda, s_t, s_rows, o_ptr, ldo):
        ep = L.VtdEpilogue()
        ep.bias, ep.out, ep.ldo, ep.out_dtype = bias.data_ptr(), o_ptr, ldo, L.F32
        L.check(L.lib.vtd_gemm_mx8(Mr, N, K, a_ptr, lda, s_t.data_ptr(), s_rows, qb.data_ptr(), K,
                                   sb.data_ptr(), sb_rows, ctypes.byref(ep), L.stream_ptr()), "mx8")
        torch.cuda.synchronize()

    small = torch.zeros((P, N), device=cuda)
    run(P, qa.data_ptr(), K, sa, sp_rows, small.data_ptr(), N)
    A = BO.Field("A", "in", "u8", [BO.Piece(A_COL, K)], qa, band=512)
    O = BO.Field("out", "out", "f32", [BO.Piece(OUT_COL, N)])
    arena.stage(PITCH, M, [A, O], ROW_INDEX16)
    sa_rows = -(-M // 4) * 4
    st, s_tall = side(cuda, sa_rows, 4, torch.uint8, fill=127)
    s_tall[:M] = gather_rows(sa[:P], arena.index)
    run(M, arena.ptr(A_COL), PITCH, s_tall, sa_rows, arena.ptr(OUT_COL), PITCH // 4)
    arena.compare(O, small.view(torch.int32), "mx8 against the 1021-row run")
    ref = MX.dequantize(qa.cpu().numpy(), sa.cpu().numpy().reshape(1, sp_rows, 4), P, K) @ \
        MX.dequantize(qb.cpu().numpy(), sb.cpu().numpy().reshape(1, sb_rows, 4), N, K).T
    rows = BO.window_rows(M, PITCH)
    got = read_windows(arena, O).view(np.float32).astype(np.float64)
    want = ref[ROW_INDEX16[rows]]
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    print(f"mx8 windows: worst {err.max():.3g}")
    assert err.max() < 5e-4, (err.max(), rows[np.argwhere(err >= 5e-4)[:3, 0]])
    arena.assert_guards("mx8")
    assert side_guards_ok(st, 127)


# ------------------------------------------------------------------ vtd_gemm_wgrad
WG_KR, WG_N, WG_W, WG_DENSE = 128, 17, 128, 9


def wgrad_problem(mode, M, pitch):
    """X one-hot in k by region (rows before byte 2^31, up to 2^32, past it; 128 values of k each,
    so K = 384: three whole k-tiles), G small values: tables [3 P][384] / [3 P][128] of pieces
    (G's pad columns zero up to the 128-wide tile the kernel reads), the region index, and dW / db
    in float64 from the table rows times their multiplicities.  bf16x3: X = h + l / 256 in every
    row; G's columns [0, 9) are integers in every row and its columns [9, 17) carry a lo piece in
    1 table row of 32 (db sums |g| over all M rows of a column: a lo piece makes 1 / 256 the unit
    and the 2^24 rule then allows about 9000 such rows)."""
    rng = np.random.default_rng([7, mode == "bf16x3"])
    x3 = mode == "bf16x3"
    r31, r32 = (1 << 31) // pitch, (1 << 32) // pitch
    m = np.arange(M, dtype=np.int64)
    region = (m >= r31).astype(np.int64) + (m >= r32)
    index = region * P + m % P
    K = 3 * WG_KR
    hs = np.array([5, 6, 7])
    hx = rng.choice(hs, size=3 * P) * rng.choice((-1, 1), size=3 * P)
    lx = rng.integers(-3, 4, size=3 * P) if x3 else np.zeros(3 * P, np.int64)
    hg = rng.choice(hs, size=(P, WG_N)) * rng.choice((-1, 1), size=(P, WG_N))
    lg = rng.integers(-3, 4, size=(P, WG_N)) if x3 else np.zeros((P, WG_N), np.int64)
    if x3:
        keepg = (np.arange(P)[:, None] + 7 * np.arange(WG_N)[None, :]) % 32 == 0
        keepg[:, :WG_DENSE] = True
        hg, lg = hg * keepg, lg * keepg
        lg[:, :WG_DENSE] = 0
    j = np.arange(3 * P) % P
    kcol = (np.arange(3 * P) // P) * WG_KR + j % WG_KR
    Xh, Xl = np.zeros((3 * P, K)), np.zeros((3 * P, K))
    Xh[np.arange(3 * P), kcol], Xl[np.arange(3 * P), kcol] = hx, lx
    Gh, Gl = np.tile(hg, (3, 1)).astype(np.float64), np.tile(lg, (3, 1)).astype(np.float64)
    count = np.bincount(index, minlength=3 * P).astype(np.float64)
    # units of 1 / 256: 256 hi.hi + lo.hi + hi.lo (the lo.lo product is not part of the mode)
    cx = count[:, None]
    units = 256 * (Xh * cx).T @ Gh + (Xl * cx).T @ Gh + (Xh * cx).T @ Gl
    absu = 256 * (np.abs(Xh) * cx).T @ np.abs(Gh) + (np.abs(Xl) * cx).T @ np.abs(Gh) + \
        (np.abs(Xh) * cx).T @ np.abs(Gl)
    dbu = (count[:, None] * (256 * Gh + Gl)).sum(0)
    absdb = (count[:, None] * np.abs(256 * Gh + Gl)).sum(0)
    # the unit of an output is 1 / 256 where a lo piece reaches it, else 1
    has_lo = (Gl != 0).any(0)
    assert (absu < G.LIMIT * (1.0 if x3 else 256.0)).all(), "dW: the 2^24 rule (gemm_designs)"
    assert (absdb < G.LIMIT * np.where(has_lo, 1.0, 256.0)).all(), "db: the 2^24 rule"
    # every region's rows of dW are non-zero and touched by that region alone
    for r in range(3):
        assert np.abs(units[r * WG_KR:(r + 1) * WG_KR]).sum() > 0

    def pieces(h, l):
        vh, vl = h.astype(np.float32), (l / 256).astype(np.float32)
        out = []
        for v in ((vh, vl) if x3 else (vh,)):
            t = np.zeros((3 * P, -(-v.shape[1] // WG_W) * WG_W), np.uint16)
            t[:, :v.shape[1]] = G.bf16_bits(v)
            assert np.array_equal(G.bf16_value(t[:, :v.shape[1]]), v)
            out.append(t)
        return out
    return dict(index=index, K=K, X=pieces(Xh, Xl), G=pieces(Gh, Gl),
                dW=G.to_f32_exact(units / 256), db=G.to_f32_exact(dbu / 256))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_gemm_wgrad(L, cuda, arena, mode):
    """The contraction over tall X and G (the [hi | lo] pieces 4096 columns apart in bf16x3).  A
    read that wraps takes region 0's rows for a later region's: those rows of dW come out zero
    and region 0's too large -- the message says which."""
    M = M16
    pr = wgrad_problem(mode, M, PITCH)
    K, N = pr["K"], WG_N
    x3 = mode == "bf16x3"
    ld = PITCH // 2
    lo = ld                                               # byte distance of the lo piece: ld / 2 * 2
    xp = [BO.Piece(0, K)] + ([BO.Piece(lo, K)] if x3 else [])
    gp = [BO.Piece(1024, WG_W)] + ([BO.Piece(1024 + lo, WG_W)] if x3 else [])
    X = BO.Field("X", "in", "bf16", xp, bits(np.concatenate(pr["X"], axis=1), cuda))
    Gf = BO.Field("G", "in", "bf16", gp, bits(np.concatenate(pr["G"], axis=1), cuda))
    for t in (np.concatenate(pr["X"] + pr["G"], axis=1),):
        BO.assert_distinct(t, pr["index"], M, PITCH, 2)
    dtype = L.BF16X3 if x3 else L.BF16
    choice = L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype)
    top = min(-(-M // 32), 256)
    assert 1 < choice < top
    arena.stage(PITCH, M, [X, Gf], pr["index"])
    for msplit in (1, choice, top):
        ldw = N + 3
        wt, dW = side(cuda, K, ldw, torch.float32)
        bt_, db = side(cuda, 1, N, torch.float32)
        nfl = msplit * (K + 1) * N
        pt, part = side(cuda, 1, nfl, torch.float32)
        L.check(L.lib.vtd_gemm_wgrad(M, K, N, arena.ptr(0), ld, arena.ptr(1024), ld, dtype,
                                     dW.data_ptr(), ldw, db.data_ptr(), part.data_ptr(),
                                     nfl * 4 if msplit > 1 else 0, msplit, L.stream_ptr()), "wgrad")
        torch.cuda.synchronize()
        got, gdb = dW.cpu().numpy(), db.cpu().numpy()[0]
        what = f"wgrad {mode} msplit {msplit}"
        if not np.array_equal(got[:, :N], pr["dW"]):
            state = []
            for r, name in enumerate(("before 2^31 bytes", "2^31 to 2^32", "past 2^32")):
                g, w = got[r * WG_KR:(r + 1) * WG_KR, :N], pr["dW"][r * WG_KR:(r + 1) * WG_KR]
                state.append(f"rows of the region {name}: " +
                             ("right" if np.array_equal(g, w) else
                              "all zero (never read)" if not g.any() else "wrong"))
            k, n = np.argwhere(got[:, :N] != pr["dW"])[0]
            raise AssertionError(f"{what}: dW differs, first at ({k}, {n}): got {got[k, n]!r}, "
                                 f"want {pr['dW'][k, n]!r}; " + "; ".join(state))
        assert (got[:, N:] == 0).all(), f"{what}: pad columns [N, ldw) must be zero"
        assert np.array_equal(gdb, pr["db"]), f"{what}: db"
        assert side_guards_ok(wt) and side_guards_ok(bt_) and side_guards_ok(pt), what
    arena.assert_guards(f"wgrad {mode}")


# ------------------------------------------------------------------ split, activations, dropout
def design_values(K):
    """[P][K] fp32 values h + l / 256 at power-of-two row and K-block scales (gemm_designs'
    bf16x3 operand, K = 64): both pieces of the split are non-trivial in every element."""
    d = G.make_design("bf16x3", P, 8, 64)
    hi, lo = d.a_op[:, :64], d.a_op[:, 64:]
    x = (G.bf16_value(hi).astype(np.float64) + G.bf16_value(lo)).astype(np.float32)
    assert np.array_equal(np.concatenate(G.split_bits(x), axis=1), d.a_op)
    return x[:, :K]


def act_values(N):
    """[P][N] pre-activations from test_gpu_act_grad.grid_values (6001 values over [-30, 30]):
    element (j, c) is value (37 j + 101 c) mod 6001, so that the rows are pairwise distinct."""
    v = grid_values()[:6001]
    j, c = np.arange(P)[:, None], np.arange(N)[None, :]
    return v[(37 * j + 101 * c) % 6001].astype(np.float32)


def signs(N):
    return np.random.default_rng(N).choice((-1.0, 1.0), size=(P, N)).astype(np.float32)


def split_rows_np(x, Pw):
    """role 0 of vtd_split_bf16x3 restated: [hi | lo], each piece Pw wide, pads zero."""
    xp = np.zeros((x.shape[0], Pw), np.float32)
    xp[:, :x.shape[1]] = x
    return np.concatenate(G.split_bits(xp), axis=1)


def check_tall_output(arena, O, table_np, what, cuda):
    """A whole-row output [M][ld]: all rows against the table's bits, then the guards."""
    arena.compare(O, bits(table_np, cuda), what)
    arena.assert_guards(what)


@pytest.mark.parametrize("role", [0, 1])
def test_split_tall_input(L, cuda, arena, role):
    """x [M][4096] fp32 (K = 32 used) -> a side output of piece width 40."""
    M, K, Pw = M16, 32, 40
    x = design_values(K)
    BO.assert_distinct(x, ROW_INDEX16, M, PITCH, 4)
    X = BO.Field("x", "in", "f32", [BO.Piece(0, K)], bits(x, cuda), band=512)
    arena.stage(PITCH, M, [X], ROW_INDEX16)
    np_ = 3 if role else 2
    ot, out = side(cuda, M, np_ * Pw, torch.int16)
    L.check(L.lib.vtd_split_bf16x3(arena.ptr(0), M, K, PITCH // 4, out.data_ptr(), np_ * Pw, role,
                                   L.stream_ptr()), "split")
    st, small = side(cuda, P, np_ * Pw, torch.int16)
    xs = torch.from_numpy(x).to(cuda)
    L.check(L.lib.vtd_split_bf16x3(xs.data_ptr(), P, K, K, small.data_ptr(), np_ * Pw, role,
                                   L.stream_ptr()), "split")
    torch.cuda.synchronize()
    s = split_rows_np(x, Pw)
    want = s if role == 0 else np.concatenate([s[:, :Pw], s[:, :Pw], s[:, Pw:]], axis=1)
    assert np.array_equal(small.cpu().numpy().view(np.uint16), want), "the 1021-row run"
    equal_rows(out, small, arena.index, f"split role {role}, tall input", M, PITCH, 4)
    rows = BO.window_rows(M, PITCH)
    BO.check_rows(out[torch.from_numpy(rows).to(cuda)].cpu().numpy().view(np.uint16), rows, M,
                  PITCH, 4, want, ROW_INDEX16, f"split role {role} windows", numbers=False)
    arena.assert_guards(f"split role {role}, tall input")
    assert side_guards_ok(ot) and side_guards_ok(st)


def test_split_tall_output(L, cuda, arena):
    """Role 0 into [M][4096] bf16 rows of 8 KiB (pieces of 2048, K = 8): 4 GiB written once.
    (Role 1 needs ldy % 3 == 0, which no power-of-two pitch has: tall input only.)"""
    M, K, ldy = M8, 8, TIED // 2
    x = design_values(K)
    xt, xs = side(cuda, M, K, torch.float32, fill=BO.FILL_IN)
    idx = index_dev(ROW_INDEX8, cuda)
    xs[:] = gather_rows(torch.from_numpy(x).to(cuda), idx)
    O = BO.Field("y", "out", "bf16", [BO.Piece(0, ldy)])
    arena.stage(TIED, M, [O], ROW_INDEX8)
    L.check(L.lib.vtd_split_bf16x3(xs.data_ptr(), M, K, K, arena.ptr(0), ldy, 0, L.stream_ptr()),
            "split")
    torch.cuda.synchronize()
    want = split_rows_np(x, ldy // 2)
    BO.assert_distinct(want, ROW_INDEX8, M, TIED, 2)
    check_tall_output(arena, O, want, "split role 0, tall output", cuda)
    rows = BO.window_rows(M, TIED)
    BO.check_rows(read_windows(arena, O).view(np.uint16), rows, M, TIED, 2, want, ROW_INDEX8,
                  "split tall output windows", numbers=False)
    assert side_guards_ok(xt, BO.FILL_IN)
    assert (M - 1) * TIED > 1 << 32 and M * ldy > 1 << 31


ACT = {"none": 0, "gelu": 1, "mish": 2}


def act_call(L, z_ptr, ldz, ga_ptr, ldga, rows, N, act, y_ptr, ldy, x3):
    code = L.BF16X3 if x3 else L.BF16
    if ga_ptr is None:
        rc = L.lib.vtd_act_forward(z_ptr, rows, N, ldz, ACT[act], y_ptr, ldy, code, L.stream_ptr())
    else:
        rc = L.lib.vtd_act_grad(z_ptr, ldz, ga_ptr, ldga, rows, N, ACT[act], y_ptr, ldy, code,
                                L.stream_ptr())
    L.check(rc, "act")


def act_windows(win_bits, rows, index, z, ga, act, N, Pw, x3, what):
    """The window rows [n][ld] (uint16) against the existing references: VTD_ACT_NONE forward is
    the conversion itself (the numpy split / bf16 rounding, exact); the derivative is within 1e-5
    of float64 read back as hi + lo (test_gpu_act_grad.py's bar, ga = 1)."""
    j = index[rows]
    assert (win_bits[:, N:Pw] == 0).all(), f"{what}: pad columns [N, piece) must be zero"
    if x3:
        assert (win_bits[:, Pw + N:2 * Pw] == 0).all(), what
    if ga is None:
        assert act == "none"
        want = split_rows_np(z, Pw) if x3 else \
            np.pad(G.bf16_bits(z), ((0, 0), (0, Pw - N)))
        assert np.array_equal(win_bits, want[j]), f"{what}: the conversion is not exact"
        return
    assert x3
    got = f32_of(win_bits[:, :N]).astype(np.float64) + f32_of(win_bits[:, Pw:Pw + N])
    ref = H.act_grad64(z.astype(np.float64), act == "mish").numpy() * ga.astype(np.float64)
    err = np.abs(got - ref[j])
    print(f"{what}: worst |err| {err.max():.3g}")
    assert np.isfinite(got).all() and err.max() <= 1e-5


ACT_CASES = [("forward", "none", True), ("forward", "none", False), ("forward", "mish", True),
             ("grad", "mish", True), ("grad", "gelu", True)]


@pytest.mark.parametrize("kind,act,x3", ACT_CASES)
def test_act_tall_input(L, cuda, arena, kind, act, x3):
    """z (and the incoming gradient: +-1, so that test_gpu_act_grad.py's bar for ga = 1 applies
    and the rows differ) tall, N = 32 of 4096 columns; a side output of piece width 48."""
    M, N, Pw = M16, 32, 48
    z = act_values(N)
    BO.assert_distinct(z, ROW_INDEX16, M, PITCH, 4)
    ga = signs(N) if kind == "grad" else None
    Z = BO.Field("z", "in", "f32", [BO.Piece(0, N)], bits(z, cuda), band=512)
    flds = [Z]
    if ga is not None:
        BO.assert_distinct(ga, ROW_INDEX16, M, PITCH, 4)
        flds.append(BO.Field("ga", "in", "f32", [BO.Piece(1024, N)], bits(ga, cuda), band=512))
    arena.stage(PITCH, M, flds, ROW_INDEX16)
    ld = 2 * Pw if x3 else Pw
    ot, out = side(cuda, M, ld, torch.int16)
    st, small = side(cuda, P, ld, torch.int16)
    zs = torch.from_numpy(z).to(cuda)
    gs = torch.from_numpy(ga).to(cuda) if ga is not None else None
    act_call(L, arena.ptr(0), PITCH // 4, arena.ptr(1024) if ga is not None else None, PITCH // 4,
             M, N, act, out.data_ptr(), ld, x3)
    act_call(L, zs.data_ptr(), N, gs.data_ptr() if gs is not None else None, N, P, N, act,
             small.data_ptr(), ld, x3)
    torch.cuda.synchronize()
    what = f"act {kind} {act} {'x3' if x3 else 'bf16'}, tall input"
    equal_rows(out, small, arena.index, what, M, PITCH, 4)
    rows = BO.window_rows(M, PITCH)
    win = out[torch.from_numpy(rows).to(cuda)].cpu().numpy().view(np.uint16)
    if not (kind == "forward" and act != "none"):
        act_windows(win, rows, ROW_INDEX16, z, ga, act, N, Pw, x3, what)
    else:
        # the Mish forward has no float64 bar of its own for the split form: its windows meet the
        # 1021-row run, which the project's epilogue-equality test covers at that size
        assert np.array_equal(win, small.cpu().numpy().view(np.uint16)[ROW_INDEX16[rows]])
    arena.assert_guards(what)
    assert side_guards_ok(ot) and side_guards_ok(st)


@pytest.mark.parametrize("kind,act,x3", [("forward", "none", True), ("grad", "mish", True),
                                         ("forward", "none", False)])
def test_act_tall_output(L, cuda, arena, kind, act, x3):
    """The output [M][4096] bf16 of 8 KiB rows written whole (N = 8, the rest zero)."""
    M, N, ld = M8, 8, TIED // 2
    Pw = ld // 2 if x3 else ld
    z = act_values(N)
    ga = signs(N) if kind == "grad" else None
    idx = index_dev(ROW_INDEX8, cuda)
    zt, zs = side(cuda, M, N, torch.float32, fill=BO.FILL_IN)
    zs[:] = gather_rows(torch.from_numpy(z).to(cuda), idx)
    gt = gs = None
    if ga is not None:
        gt, gs = side(cuda, M, N, torch.float32, fill=BO.FILL_IN)
        gs[:] = gather_rows(torch.from_numpy(ga).to(cuda), idx)
    O = BO.Field("y", "out", "bf16", [BO.Piece(0, ld)])
    arena.stage(TIED, M, [O], ROW_INDEX8)
    st, small = side(cuda, P, ld, torch.int16)
    z1 = torch.from_numpy(z).to(cuda)
    g1 = torch.from_numpy(ga).to(cuda) if ga is not None else None
    act_call(L, zs.data_ptr(), N, gs.data_ptr() if gs is not None else None, N, M, N, act,
             arena.ptr(0), ld, x3)
    act_call(L, z1.data_ptr(), N, g1.data_ptr() if g1 is not None else None, N, P, N, act,
             small.data_ptr(), ld, x3)
    torch.cuda.synchronize()
    what = f"act {kind} {act} {'x3' if x3 else 'bf16'}, tall output"
    arena.compare(O, small, what)
    rows = BO.window_rows(M, TIED)
    act_windows(read_windows(arena, O).view(np.uint16), rows, ROW_INDEX8, z, ga, act, N, Pw, x3,
                what)
    arena.assert_guards(what)
    assert side_guards_ok(zt, BO.FILL_IN) and side_guards_ok(st)
    assert gt is None or side_guards_ok(gt, BO.FILL_IN)


def test_dropout_apply(L, cuda, arena):
    """x and y fp32 in one 16 KiB row, N = 39.  Not row-invariant (the counter carries the row):
    all rows are 0 or x * inv_keep with the kept fraction the rate's; the windows' mask is
    dropout_oracle.mask_rows of those rows (row0 = the window's first row)."""
    M, N, rate = M16, 39, 0.25
    seed, step, site = 0x1234567887654321, 3, 5
    x = design_values(64)[:, :N]
    assert (x != 0).all()
    X = BO.Field("x", "in", "f32", [BO.Piece(0, N)], bits(x, cuda), band=512)
    Y = BO.Field("y", "out", "f32", [BO.Piece(1024, N)])
    arena.stage(PITCH, M, [X, Y], ROW_INDEX16)
    d = L.VtdDropout(seed=seed, step=step, site=site, rate=rate)
    L.check(L.lib.vtd_dropout_apply(ctypes.byref(d), arena.ptr(0), PITCH // 4, M, N,
                                    arena.ptr(1024), PITCH // 4, L.stream_ptr()), "dropout_apply")
    torch.cuda.synchronize()
    c = float(DO.inv_keep(rate))
    xv, yv = arena.view(X, bits=False), arena.view(Y, bits=False)
    kept = torch.zeros((), dtype=torch.int64, device=cuda)
    bad = torch.zeros((), dtype=torch.int64, device=cuda)
    for a in range(0, M, 1 << 15):
        xs, ys = xv[a:a + (1 << 15)], yv[a:a + (1 << 15)]
        k = ys == xs * c                                     # one fp32 multiply
        z = ys.view(torch.int32) == 0                        # +0, not -0
        bad += (~(k | z)).sum()
        kept += k.sum()
    assert int(bad.item()) == 0, "an output is neither +0 nor x * inv_keep"
    frac = int(kept.item()) / (M * N)
    want = 1 - DO.threshold(rate) / 65536
    assert abs(frac - want) < 5 * (want * (1 - want) / (M * N)) ** 0.5, (frac, want)
    for name, a, b in BO.windows(M, PITCH):
        keep = DO.mask_rows(b - a, N, rate, seed, step, site, row0=a)
        got = arena.window(Y, a, b).view(np.float32)
        ref = np.where(keep, x[ROW_INDEX16[a:b]] * DO.inv_keep(rate), np.float32(0)).astype(np.float32)
        if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
            i, j = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[0]
            raise AssertionError(
                f"dropout window {name}: row {a + i} column {j} (byte offset "
                f"{(a + i) * PITCH + 1024 + 4 * j}): got {got[i, j]!r}, want {ref[i, j]!r}")
    arena.assert_guards("dropout_apply")


# ------------------------------------------------------------------ LayerNorm forward and statistics
def ln_case(xdt, D):
    """ln_designs.Case of P rows whose rows are pairwise distinct: the three constant rows once
    each, then order-free, general and high-offset rows in turn."""
    of = len(LD.ORDER_FREE[xdt])
    cyc = [("of", i) for i in range(of)] + [("gen", 0), ("hi", 0)]
    kinds = [("const", 0), ("const", 1), ("const", 2)] + [cyc[r % len(cyc)] for r in range(P - 3)]
    return LD.Case(xdt, P, D, ldx=D, kinds=kinds)


def overwrite(small, rows, index, win):
    """The P-row result with the window's rows put in the place of their table rows: what the
    ln_designs checks (which take a whole case) are given."""
    out = small.copy()
    out[index[rows]] = win
    return out


# (x dtype, D, output form): each layernorm kernel ln_designs.route names
LN_IN = [("f32", 256, "f32", "layernorm_kernel"), ("bf16", 256, "bf16", "layernorm16_kernel"),
         ("f32", 30, "split", "layernorm_generic_kernel"), ("bf16", 264, "f32", "layernorm_kernel")]


@pytest.mark.parametrize("xdt,D,out,kernel", LN_IN)
def test_layernorm_tall_input(L, cuda, arena, xdt, D, out, kernel):
    """x tall (D of the 16 KiB row), y and the statistics as side outputs."""
    M = M16
    c = ln_case(xdt, D)
    xbits = LD.bf16_bits(c.x) if xdt == "bf16" else c.x
    esz = xbits.dtype.itemsize
    BO.assert_distinct(xbits, ROW_INDEX16, M, PITCH, esz)
    band = -(-D * esz // 512) * 512 + 512
    X = BO.Field("x", "in", xdt, [BO.Piece(0, D)], bits(xbits, cuda), band=band)
    arena.stage(PITCH, M, [X], ROW_INDEX16)
    ldx = PITCH // esz
    Pw = D + (4 if D % 4 == 0 else 3)
    ldy = 2 * Pw if out == "split" else Pw
    odt = torch.float32 if out == "f32" else torch.int16
    osz = 4 if out == "f32" else 2
    assert LD.route("layernorm", xdt, D, ldx, P=Pw, out="f32" if out == "f32" else "bf16")[0] == kernel
    assert LD.route("layernorm", xdt, D, D, P=Pw, out="f32" if out == "f32" else "bf16")[0] == kernel
    gam, bet = torch.from_numpy(c.gamma).to(cuda), torch.from_numpy(c.beta).to(cuda)
    xcode = L.BF16 if xdt == "bf16" else L.F32
    code = {"f32": L.F32, "bf16": L.BF16, "split": L.BF16X3}[out]
    xs = bits(xbits, cuda)
    res = {}
    for name, xp, ld, rows in (("big", arena.ptr(0), ldx, M), ("small", xs.data_ptr(), D, P)):
        yt, y = side(cuda, rows, ldy, odt)
        stt, stat = side(cuda, rows, 2, torch.float32)
        L.check(L.lib.vtd_layernorm(xp, xcode, rows, D, ld, gam.data_ptr(), bet.data_ptr(), 1e-3,
                                    y.data_ptr(), ldy, code, L.stream_ptr()), "layernorm")
        L.check(L.lib.vtd_layernorm_stats(xp, xcode, rows, D, ld, 1e-3, stat.data_ptr(),
                                          L.stream_ptr()), "layernorm_stats")
        torch.cuda.synchronize()
        assert side_guards_ok(yt) and side_guards_ok(stt), name
        res[name] = (y, stat)
    what = f"layernorm {xdt} D {D} {out}, tall input"
    ybig, sbig = res["big"]
    ysm, ssm = res["small"]
    yv = (lambda t: t.view(torch.int32)) if out == "f32" else (lambda t: t)
    equal_rows(yv(ybig), yv(ysm), arena.index, what, M, PITCH, esz)
    equal_rows(sbig.view(torch.int32), ssm.view(torch.int32), arena.index, what + " stats", M,
               PITCH, esz)
    # (b) the windows through ln_designs' checks, in the place of their table rows
    rows = BO.window_rows(M, PITCH)
    sk = "ln_stats_kernel" if D % 8 == 0 else "ln_stats_generic_kernel"
    assert LD.route("layernorm_stats", xdt, D, ldx)[0] == sk
    for _, a, b in BO.windows(M, PITCH):
        r = np.arange(a, b)
        st = overwrite(ssm.cpu().numpy(), r, ROW_INDEX16, sbig[a:b].cpu().numpy())
        LD.check_stats(c, st, what=what + " stats", kernel=LD.route("layernorm_stats", xdt, D, ldx))
        yw = overwrite(ysm.cpu().numpy(), r, ROW_INDEX16, ybig[a:b].cpu().numpy())
        kern = LD.route("layernorm", xdt, D, ldx, P=Pw, out="f32" if out == "f32" else "bf16")
        if out == "f32":
            assert (yw[:, D:] == 0).all()
            LD.check_y(c, "f32", yw[:, :D], what=what, kernel=kern)
        elif out == "bf16":
            assert (yw[:, D:] == 0).all()
            LD.check_y(c, "bf16", yw[:, :D].view(np.uint16), what=what, kernel=kern)
        else:
            # the split output is the split of the f32 output (test_gpu_layernorm_designed.py);
            # its hi piece is the bf16 output, which meets float64 here
            u = yw.view(np.uint16)
            assert (u[:, D:Pw] == 0).all() and (u[:, Pw + D:] == 0).all()
            LD.check_y(c, "bf16", u[:, :D], what=what, kernel=kern)
    arena.assert_guards(what)


LN_OUT = [("f32", 8, "f32", "layernorm_kernel"), ("bf16", 16, "bf16", "layernorm16_kernel"),
          ("f32", 6, "split", "layernorm_generic_kernel")]


@pytest.mark.parametrize("xdt,D,out,kernel", LN_OUT)
def test_layernorm_tall_output(L, cuda, arena, xdt, D, out, kernel):
    """y [M][ld] of 8 KiB rows written whole (columns [D, ld) zero), x a side input."""
    M = M8
    c = ln_case(xdt, D)
    xbits = LD.bf16_bits(c.x) if xdt == "bf16" else c.x
    osz = 4 if out == "f32" else 2
    ldy = TIED // osz
    Pw = ldy // 2 if out == "split" else ldy
    assert LD.route("layernorm", xdt, D, D, P=Pw, out="f32" if out == "f32" else "bf16")[0] == kernel
    idx = index_dev(ROW_INDEX8, cuda)
    xt, xs = side(cuda, M, D, torch.int16 if xdt == "bf16" else torch.int32, fill=BO.FILL_IN)
    x1 = bits(xbits, cuda)
    xs[:] = gather_rows(x1, idx)
    O = BO.Field("y", "out", "f32" if out == "f32" else "bf16", [BO.Piece(0, ldy)])
    arena.stage(TIED, M, [O], ROW_INDEX8)
    gam, bet = torch.from_numpy(c.gamma).to(cuda), torch.from_numpy(c.beta).to(cuda)
    xcode = L.BF16 if xdt == "bf16" else L.F32
    code = {"f32": L.F32, "bf16": L.BF16, "split": L.BF16X3}[out]
    st, small = side(cuda, P, ldy, torch.float32 if out == "f32" else torch.int16)
    L.check(L.lib.vtd_layernorm(xs.data_ptr(), xcode, M, D, D, gam.data_ptr(), bet.data_ptr(), 1e-3,
                                arena.ptr(0), ldy, code, L.stream_ptr()), "layernorm")
    L.check(L.lib.vtd_layernorm(x1.data_ptr(), xcode, P, D, D, gam.data_ptr(), bet.data_ptr(), 1e-3,
                                small.data_ptr(), ldy, code, L.stream_ptr()), "layernorm")
    torch.cuda.synchronize()
    what = f"layernorm {xdt} D {D} {out}, tall output"
    arena.compare(O, small.view(torch.int32) if out == "f32" else small, what)
    kern = LD.route("layernorm", xdt, D, D, P=Pw, out="f32" if out == "f32" else "bf16")
    sm = small.cpu().numpy()
    for _, a, b in BO.windows(M, TIED):
        yw = overwrite(sm, np.arange(a, b), ROW_INDEX8,
                       arena.window(O, a, b).view(sm.dtype))
        if out == "f32":
            assert (yw[:, D:] == 0).all()
            LD.check_y(c, "f32", yw[:, :D], what=what, kernel=kern)
        else:
            u = yw.view(np.uint16)
            assert (u[:, D:Pw] == 0).all() and (u[:, Pw + D:] == 0).all()
            LD.check_y(c, "bf16", u[:, :D], what=what, kernel=kern)
    arena.assert_guards(what)
    assert side_guards_ok(xt, BO.FILL_IN) and side_guards_ok(st)
    assert (M - 1) * TIED > 1 << 32


# ------------------------------------------------------------------ vtd_layernorm_backward
@pytest.mark.parametrize("add_mode", ["separate", "alias"])
def test_layernorm_backward(L, cuda, arena, add_mode):
    """x, dy, add and dx tall in one 16 KiB fp32 row (D = 64 of 4096 columns each).  dx: all rows
    against the 1021-row run bit for bit, the windows against float64 within k_dx 2^-24; dgamma
    and dbeta against float64 sums of the 1021 rows' terms times their multiplicities, within
    k_param(M) 2^-24 of the summed magnitudes (tests/ln_grad_oracle.py)."""
    M, D = M16, 64
    c = LG.Case(D, P, designs=False)                      # N(0, 1) rows: pairwise distinct
    ld = PITCH // 4
    assert LG.route(D, (ld, ld, ld, ld)) == "vec"
    cols = dict(x=0, dy=1024, add=2048, dx=4096)
    X = BO.Field("x", "in", "f32", [BO.Piece(cols["x"], D)], bits(c.x, cuda), band=512)
    DY = BO.Field("dy", "in", "f32", [BO.Piece(cols["dy"], D)], bits(c.dy, cuda), band=512)
    for t in (c.x, c.dy, c.add):
        BO.assert_distinct(t, ROW_INDEX16, M, PITCH, 4)
    flds = [X, DY]
    if add_mode == "alias":
        DX = BO.Field("dx", "inout", "f32", [BO.Piece(cols["dx"], D)], bits(c.add, cuda))
        add_col = cols["dx"]
    else:
        flds.append(BO.Field("add", "in", "f32", [BO.Piece(cols["add"], D)], bits(c.add, cuda),
                             band=512))
        DX = BO.Field("dx", "out", "f32", [BO.Piece(cols["dx"], D)])
        add_col = cols["add"]
    flds.append(DX)
    arena.stage(PITCH, M, flds, ROW_INDEX16)
    gam = torch.from_numpy(c.gamma).to(cuda)

    def stats(xp, ldx, rows):
        st = torch.empty((rows, 2), device=cuda)
        L.check(L.lib.vtd_layernorm_stats(xp, L.F32, rows, D, ldx, LG.EPS, st.data_ptr(),
                                          L.stream_ptr()), "stats")
        return st

    def backward(xp, dyp, addp, dxp, ldv, rows, stat):
        n = ctypes.c_size_t()
        L.check(L.lib.vtd_layernorm_backward_workspace_bytes(rows, D, ctypes.byref(n)), "ws")
        wt, ws = side(cuda, 1, n.value, torch.uint8)
        gt, dg = side(cuda, 1, D, torch.float32)
        bt_, db = side(cuda, 1, D, torch.float32)
        L.check(L.lib.vtd_layernorm_backward(xp, ldv, stat.data_ptr(), gam.data_ptr(), dyp, ldv,
                                             addp, ldv, rows, D, dxp, ldv, dg.data_ptr(),
                                             db.data_ptr(), ws.data_ptr(), n.value,
                                             L.stream_ptr()), "layernorm_backward")
        torch.cuda.synchronize()
        assert side_guards_ok(wt) and side_guards_ok(gt) and side_guards_ok(bt_)
        return dg.cpu().numpy()[0], db.cpu().numpy()[0]

    st_big = stats(arena.ptr(0), ld, M)
    dg, db = backward(arena.ptr(cols["x"]), arena.ptr(cols["dy"]), arena.ptr(add_col),
                      arena.ptr(cols["dx"]), ld, M, st_big)
    # the 1021-row run: tight rows, add separate
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(c, k))).to(cuda) for k in ("x", "dy", "add")}
    st_small = stats(t["x"].data_ptr(), D, P)
    dx_small = torch.empty((P, D), device=cuda)
    backward(t["x"].data_ptr(), t["dy"].data_ptr(), t["add"].data_ptr(), dx_small.data_ptr(), D, P,
             st_small)
    what = f"layernorm_backward add {add_mode}"
    equal_rows(st_big.view(torch.int32), st_small.view(torch.int32), arena.index, what + " stats",
               M, PITCH, 4)
    arena.compare(DX, dx_small.view(torch.int32), what + " dx")
    stat = st_small.cpu().numpy()
    ref = LG.backward64(c.x, stat, c.gamma, c.dy, c.add)
    rows = BO.window_rows(M, PITCH)
    j = ROW_INDEX16[rows]
    got = read_windows(arena, DX).view(np.float32)
    r = LG.ratio(got, ref["dx"][j], ref["den_x"][j], LG.k_dx(D, "vec") * LG.U)
    # dgamma, dbeta: float64 terms of the P rows times how often each occurs among the M rows
    mult = np.bincount(ROW_INDEX16, minlength=P).astype(np.float64)[:, None]
    xhat = (c.x.astype(np.float64) - stat[:, :1]) * stat[:, 1:2]
    tg, tb = c.dy.astype(np.float64) * xhat, c.dy.astype(np.float64)
    cg = LG.k_param(M) * LG.U
    rg = LG.ratio(dg, (tg * mult).sum(0), (np.abs(tg) * mult).sum(0), cg)
    rb = LG.ratio(db, (tb * mult).sum(0), (np.abs(tb) * mult).sum(0), cg)
    print(f"{what}: fractions of the bars dx {r:.3f} dgamma {rg:.3f} dbeta {rb:.3f} "
          f"(k_dx {LG.k_dx(D, 'vec')}, k_param {LG.k_param(M)})")
    assert max(r, rg, rb) <= 1.0, (r, rg, rb)
    arena.assert_guards(what)


# ------------------------------------------------------------------ attention
# (staircase has levels for N <= 320 only, ramp no backward bar: neither is used here)
ATT_IMAGES = (("spike", 0), ("tie", 0), ("offset", 0), ("spike", 1), ("tie", 1))
DK = 64


def att_images(N):
    """One period of images, one head of 64: qkv [5 N][192] fp32 (bf16-representable), the
    float64 output [5 N][64] and the extra tolerance of each image's pattern."""
    assert len(ATT_IMAGES) == BO.IMAGE_PERIOD
    qkv, exp, extra = [], [], []
    for pattern, b in ATT_IMAGES:
        full, e, x, _ = make_case(pattern, N, DK)
        rows = full[b * N:(b + 1) * N]
        qkv.append(np.concatenate([rows[:, 0:64], rows[:, 128:192], rows[:, 256:320]], axis=1))
        exp.append(e[b, :, 0, :])
        extra.append(x)
    return np.concatenate(qkv), np.concatenate(exp), extra


# (mode, N, knob, variant): every variant tests/test_gpu_attention_patterns.py reaches
ATT_CASES = [("bf16", 196, -1, "persistent"), ("bf16", 196, 2, "8-wave"),
             ("bf16", 196, 1, "generic"), ("bf16", 196, 6, "lds-dma"), ("bf16", 100, -1, "4-wave"),
             ("bf16", 400, -1, "8-wave"), ("bf16", 400, 6, "lds-dma"), ("bf16", 400, 1, "generic"),
             ("f32", 196, -1, "f32"), ("f32", 400, -1, "f32"), ("x3", 196, -1, "x3 32-key chunks"),
             ("x3", 196, 10, "x3 64-key chunks"), ("x3", 400, -1, "x3 32-key chunks"),
             ("x3", 400, 10, "x3 64-key chunks")]
QKV_COL, O_COL, DO_COL, DQ_COL = 0, 1024, 2048, 4096


def att_layout(mode, cuda, qkv, N, B):
    """Fields of the tall qkv and O of one mode, and the call's leading dimensions."""
    if mode == "bf16":
        Q = BO.Field("qkv", "in", "bf16", [BO.Piece(QKV_COL, 192)], bits(G.bf16_bits(qkv), cuda),
                     band=512)
        assert np.array_equal(G.bf16_value(G.bf16_bits(qkv)), qkv)
        O = BO.Field("O", "out", "bf16", [BO.Piece(O_COL, 64)])
        return Q, O, PITCH // 2, PITCH // 2
    Q = BO.Field("qkv", "in", "f32", [BO.Piece(QKV_COL, 192)], bits(qkv, cuda), band=1024)
    if mode == "f32":
        return Q, BO.Field("O", "out", "f32", [BO.Piece(O_COL, 64)]), PITCH // 4, PITCH // 4
    ldo = PITCH // 2
    O = BO.Field("O", "out", "bf16", [BO.Piece(O_COL, 64), BO.Piece(O_COL + ldo, 64)])
    return Q, O, PITCH // 4, ldo


def att_values(mode, pieces):
    """The output pieces (bits, numpy) as float64: f32, bf16, or hi + lo."""
    if mode == "f32":
        return pieces[0].view(np.float32).astype(np.float64)
    v = f32_of(pieces[0]).astype(np.float64)
    return v + f32_of(pieces[1]) if mode == "x3" else v


def att_small(L, cuda, mode, qkv, N, knob, train=False):
    """The same entry point on one period of images, tight leading dimensions."""
    B = BO.IMAGE_PERIOD
    code = {"bf16": L.BF16, "f32": L.F32, "x3": L.BF16X3}[mode]
    q = bits(G.bf16_bits(qkv), cuda) if mode == "bf16" else torch.from_numpy(qkv).to(cuda)
    ldo = 128 if mode == "x3" else 64
    o = torch.zeros((B * N, ldo), dtype=torch.float32 if mode == "f32" else torch.int16, device=cuda)
    lse = torch.zeros((B, 1, N), device=cuda)
    with L.knob(L.KNOB_ATTN_VARIANT, knob):
        if train:
            L.check(L.lib.vtd_attention_train(q.data_ptr(), B, N, 1, DK, 192, float(LN2_F32),
                                              o.data_ptr(), ldo, lse.data_ptr(), code,
                                              L.stream_ptr()), "attention_train")
        else:
            L.check(L.lib.vtd_attention(q.data_ptr(), B, N, 1, DK, 192, float(LN2_F32),
                                        o.data_ptr(), ldo, code, L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    return q, o, lse


def att_window_check(mode, got64, rows, index, exp, extra, N, what):
    """Window rows against float64: the mode's tolerance times max(1, max |O|) of the row's
    image, plus the pattern's extra term (tests/test_gpu_attention_patterns.py)."""
    j = index[rows]
    img = j // N
    tol = np.array([ATT_TOL[mode] * max(1.0, np.abs(exp[i * N:(i + 1) * N]).max()) + extra[i]
                    for i in range(BO.IMAGE_PERIOD)])[img]
    err = np.abs(got64 - exp[j]).max(axis=1)
    assert np.isfinite(got64).all(), what
    bad = err >= tol
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: row {rows[i]} (image {rows[i] // N}, design image {img[i]}, "
                             f"token {rows[i] % N}): error {err[i]:.3g} >= {tol[i]:.3g}")
    print(f"{what}: worst window error / tolerance {float((err / tol).max()):.3f}")


@pytest.mark.parametrize("mode,N,knob,variant", ATT_CASES)
def test_attention(L, cuda, arena, mode, N, knob, variant):
    B = -(-M16 // N)
    M = B * N
    qkv, exp, extra = att_images(N)
    index = BO.image_index(B, N)
    Q, O, ldq, ldo = att_layout(mode, cuda, qkv, N, B)
    BO.assert_distinct(qkv, index, M, PITCH, Q.esz, clamp_rows=min(BO.WINDOW, BO.IMAGE_PERIOD * N))
    arena.stage(PITCH, M, [Q, O], index)
    code = {"bf16": L.BF16, "f32": L.F32, "x3": L.BF16X3}[mode]
    with L.knob(L.KNOB_ATTN_VARIANT, knob):
        L.check(L.lib.vtd_attention(arena.ptr(QKV_COL), B, N, 1, DK, ldq, float(LN2_F32),
                                    arena.ptr(O_COL), ldo, code, L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    _, o_small, _ = att_small(L, cuda, mode, qkv, N, knob)
    what = f"attention {mode} N {N} knob {knob} ({variant})"
    ob = o_small.view(torch.int32) if mode == "f32" else o_small
    for i in range(len(O.pieces)):
        arena.compare(O, ob, f"{what} piece {i}", piece=i, col0=64 * i)
    rows = BO.window_rows(M, PITCH)
    got = att_values(mode, [read_windows(arena, O, i) for i in range(len(O.pieces))])
    att_window_check(mode, got, rows, index, exp, extra, N, what)
    arena.assert_guards(what)
    assert (M - 1) * PITCH > 1 << 32


def att_grad_reference(qkv, do, N):
    """float64 gradients and magnitudes of each design image: [5 N][192] each."""
    g, den = [], []
    for i in range(BO.IMAGE_PERIOD):
        r = qkv[i * N:(i + 1) * N].astype(np.float64)
        q, k, v = (r[:, c:c + 64].reshape(1, N, 1, 64) for c in (0, 64, 128))
        d = do[i * N:(i + 1) * N].astype(np.float64).reshape(1, N, 1, 64)
        g.append(np.concatenate([t[0, :, 0, :] for t in AG.backward64(q, k, v, d, float(LN2_F32))],
                                axis=1))
        den.append(np.concatenate([t[0, :, 0, :] for t in AG.magnitudes(q, k, v, d, float(LN2_F32))],
                                  axis=1))
    return np.concatenate(g), np.concatenate(den)


@pytest.mark.parametrize("mode,N", [("bf16", 196), ("x3", 196), ("bf16", 400), ("x3", 400)])
def test_attention_train_and_backward(L, cuda, arena, mode, N):
    """vtd_attention_train writes the tall O (and the small lse); vtd_attention_backward reads
    the tall qkv, O and dO and writes the tall dqkv -- all four in one 16 KiB row.  All rows
    against a run on one period of images bit for bit; the windows' gradients against float64,
    componentwise within C_DESIGNED of their magnitudes (tests/attention_grad_oracle.py)."""
    B = -(-M16 // N)
    M = B * N
    x3 = mode == "x3"
    qkv, exp, extra = att_images(N)
    rng = np.random.default_rng([N, 11])
    do = AG.bf16(rng.normal(0.0, 1.0, size=(BO.IMAGE_PERIOD * N, 64)).astype(np.float32)) \
        .astype(np.float32)
    index = BO.image_index(B, N)
    Q, O, ldq, ldo = att_layout(mode, cuda, qkv, N, B)
    ldd = PITCH // 2                                     # dqkv: bf16, or [hi | lo] 4096 apart
    if x3:
        DOf = BO.Field("dO", "in", "f32", [BO.Piece(DO_COL, 64)], bits(do, cuda), band=512)
        DQ = BO.Field("dqkv", "out", "bf16", [BO.Piece(DQ_COL, 192), BO.Piece(DQ_COL + ldd, 192)])
        lddo = PITCH // 4
    else:
        DOf = BO.Field("dO", "in", "bf16", [BO.Piece(DO_COL, 64)], bits(G.bf16_bits(do), cuda),
                       band=512)
        DQ = BO.Field("dqkv", "out", "bf16", [BO.Piece(DQ_COL, 192)])
        lddo = PITCH // 2
    BO.assert_distinct(do, index, M, PITCH, DOf.esz, clamp_rows=min(BO.WINDOW, BO.IMAGE_PERIOD * N))
    arena.stage(PITCH, M, [Q, O, DOf, DQ], index)
    code = L.BF16X3 if x3 else L.BF16
    scale = float(LN2_F32)

    def run(Br, qp, op, dop, dqp, lq, lo_, ld_o, ld_q):
        lt, lse = side(cuda, 1, Br * N, torch.float32)
        L.check(L.lib.vtd_attention_train(qp, Br, N, 1, DK, lq, scale, op, lo_, lse.data_ptr(), code,
                                          L.stream_ptr()), "attention_train")
        n = L.c_size_t(0)
        L.check(L.lib.vtd_attention_backward_workspace_bytes(Br, N, 1, DK, code, ctypes.byref(n)))
        wt, ws = side(cuda, 1, max(n.value, 16), torch.uint8)
        L.check(L.lib.vtd_attention_backward(qp, op, dop, lse.data_ptr(), Br, N, 1, DK, lq, lo_,
                                             ld_o, scale, dqp, ld_q, code, ws.data_ptr(), n.value,
                                             L.stream_ptr()), "attention_backward")
        torch.cuda.synchronize()
        assert side_guards_ok(lt) and side_guards_ok(wt)
        return lse

    lse_big = run(B, arena.ptr(QKV_COL), arena.ptr(O_COL), arena.ptr(DO_COL), arena.ptr(DQ_COL),
                  ldq, ldo, lddo, ldd)
    # one period of images, tight leading dimensions
    Bs = BO.IMAGE_PERIOD
    qs = torch.from_numpy(qkv).to(cuda) if x3 else bits(G.bf16_bits(qkv), cuda)
    ds = torch.from_numpy(do).to(cuda) if x3 else bits(G.bf16_bits(do), cuda)
    os_ = torch.zeros((Bs * N, 128 if x3 else 64), dtype=torch.int16, device=cuda)
    dqs = torch.zeros((Bs * N, 384 if x3 else 192), dtype=torch.int16, device=cuda)
    lse_small = run(Bs, qs.data_ptr(), os_.data_ptr(), ds.data_ptr(), dqs.data_ptr(), 192,
                    os_.shape[1], 64, dqs.shape[1])
    what = f"attention train + backward {mode} N {N}"
    for i in range(len(O.pieces)):
        arena.compare(O, os_, f"{what} O piece {i}", piece=i, col0=64 * i)
    for i in range(len(DQ.pieces)):
        arena.compare(DQ, dqs, f"{what} dqkv piece {i}", piece=i, col0=192 * i)
    li = torch.from_numpy((np.arange(B) % Bs)).to(cuda)
    assert torch.equal(lse_big.view(B, N).view(torch.int32), lse_small.view(Bs, N)[li].view(torch.int32)), \
        f"{what}: lse differs from the one-period run"
    rows = BO.window_rows(M, PITCH)
    o64 = att_values(mode, [read_windows(arena, O, i) for i in range(len(O.pieces))])
    att_window_check(mode, o64, rows, index, exp, extra, N, what + " O")
    g = att_values("x3" if x3 else "bf16", [read_windows(arena, DQ, i) for i in range(len(DQ.pieces))])
    g64, den = att_grad_reference(qkv, do, N)
    j = index[rows]
    err, d = np.abs(g - g64[j]), den[j]
    assert np.isfinite(g).all()
    assert (err[d == 0] == 0).all(), f"{what}: a gradient with no contributing term is not zero"
    worst = float((err[d > 0] / d[d > 0]).max())
    print(f"{what}: worst |g - g64| / den {worst:.3g} (bar {AG.C_DESIGNED[mode]:.3g})")
    assert worst <= AG.C_DESIGNED[mode]
    arena.assert_guards(what)
