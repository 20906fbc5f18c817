"""tests/big_operands.py on the CPU: the arena's layout arithmetic, the proof that the periodic
row data makes a mis-addressed row visible, negative controls (a reference gather with a
32-bit-truncated row address feeding a GEMM emulation and a per-row op must be rejected, with the
alias row named; the correct gather accepted), and the entry points that refuse an operand they
cannot address (VTD_ERR_INVALID_ARG before any launch, no GPU needed)."""
import re

import numpy as np
import pytest

from tests import big_operands as BO
from tests import gemm_designs as G
from tests import ln_designs as LD

P = BO.P
PITCHES = (BO.PITCH, BO.PITCH_TIED)


# ------------------------------------------------------------------ layout
def test_arena_layout():
    assert BO.FRONT_GUARD == 4 << 30 and BO.SPAN == (1 << 32) + (64 << 20)
    assert BO.BACK_GUARD == 64 << 20 and BO.ARENA_BYTES == BO.FRONT_GUARD + BO.SPAN + BO.BACK_GUARD
    assert 8.1 < BO.ARENA_BYTES / 2 ** 30 < 8.2
    for pitch in PITCHES:
        lay = BO.layout(pitch)
        M = BO.tall_rows(pitch)
        assert lay["base_byte"] == BO.FRONT_GUARD and lay["base_row"] * pitch == BO.FRONT_GUARD
        assert lay["total_rows"] * pitch == BO.ARENA_BYTES
        assert lay["total_rows"] == lay["base_row"] + lay["span_rows"] + lay["back_rows"]
        # ragged, a few hundred rows past 2^32 bytes, inside the span
        assert M == (1 << 32) // pitch + 333 and M <= lay["span_rows"]
        assert (M - 1) * pitch > 1 << 32 and M * pitch < (1 << 32) + (6 << 20)
        assert M % 256 and M % 32 and M % 4                  # the last tile / step / row group is partial
    assert BO.tall_rows(16384) == 262477
    # the [hi | lo] row of 8192 bf16 has more than 2^31 elements, the fp32 row does not
    assert BO.tall_rows(16384) * 8192 > 1 << 31 > BO.tall_rows(16384) * 4096


def test_windows():
    for pitch in PITCHES:
        M = BO.tall_rows(pitch)
        w = BO.windows(M, pitch)
        assert [b - a for _, a, b in w] == [512, 512, 512, 512]
        assert w[0][1:] == (0, 512) and w[3][1:] == (M - 512, M)
        for (_, a, b), edge in zip(w[1:3], (1 << 31, 1 << 32)):
            assert a * pitch < edge < b * pitch and (a + 256) * pitch == edge     # astride the byte offset
        rows = BO.window_rows(M, pitch)
        assert len(rows) == 2048 and rows.max() == M - 1
        # each window is shorter than the period: its rows are distinct table rows
        for _, a, b in w:
            assert len(set(BO.row_index(M)[a:b])) == b - a


def test_every_wrap_lands_in_memory_the_test_owns():
    """The reasoning of the front guard, checked: under each truncation every row of a tall
    operand is reached inside the arena -- at worst 2 GiB (signed byte offset) or 4 GiB (int
    element index into bf16) before the base."""
    for pitch in PITCHES:
        M = BO.tall_rows(pitch)
        m = np.arange(M, dtype=np.int64)
        lay = BO.layout(pitch)
        lows = {}
        for esz in (1, 2, 4):
            for wrap in BO.WRAPS:
                r = BO.wrapped_row(m, pitch, esz, wrap)
                assert r.min() >= -lay["base_row"] and r.max() < M, (pitch, esz, wrap)
                lows[(wrap, esz)] = int(r.min()) * pitch
                if wrap == "unsigned byte offset":
                    assert r.min() >= 0                      # lands inside the operand
        assert lows[("signed byte offset", 2)] == -(1 << 31)
        assert lows[("int element index", 2)] == -(1 << 32)
        assert lows[("int element index", 4)] == 0           # no fp32 operand has 2^31 elements
        # rows before the boundary are never moved
        for wrap in BO.WRAPS:
            r = BO.wrapped_row(m, pitch, 2, wrap)
            assert (r[:(1 << 31) // pitch] == m[:(1 << 31) // pitch]).all()


# ------------------------------------------------------------------ the data design
def designed_tables():
    """The P-row tables the GPU tests gather from, by family: (name, table, element size)."""
    d = G.make_design("bf16x3", P, 17, 64)
    f = G.make_design("f32", P, 72, 64, epi=("bias", "resid"))
    kinds = [("const", 0), ("const", 1), ("const", 2)] + \
        [(("of", 0), ("of", 1), ("of", 2), ("of", 3), ("gen", 0), ("hi", 0))[r % 6]
         for r in range(P - 3)]
    ln = LD.Case("f32", P, 256, ldx=256, kinds=kinds)
    return [("gemm bf16x3 A", d.a_op, 2), ("gemm bf16x3 expected", G.cast_f32(d.expected()), 4),
            ("gemm f32 A", f.a_op, 4), ("gemm f32 expected", G.cast_f32(f.expected()), 4),
            ("layernorm x", ln.x, 4)]


def test_period_is_an_odd_prime():
    assert P >= 1021 and P % 2 == 1 and all(P % q for q in range(3, int(P ** 0.5) + 1, 2))
    for pitch in PITCHES:
        for esz in (1, 2, 4):
            for k in (31, 32):
                assert ((1 << k) // pitch) % P != 0 and ((1 << k) // (pitch // esz)) % P != 0


@pytest.mark.parametrize("pitch", PITCHES)
def test_rows_differ_from_their_aliases(pitch):
    M = BO.tall_rows(pitch)
    index = BO.row_index(M)
    for name, table, esz in designed_tables():
        BO.assert_distinct(table, index, M, pitch, esz)
    # the check itself notices a period that divides an alias distance, and equal rows
    with pytest.raises(AssertionError, match="alias"):
        BO.assert_distinct(np.arange(1024)[:, None], BO.row_index(M, 1024), M, pitch, 2)
    dup = np.arange(P)[:, None].copy()
    dup[7] = dup[3]
    with pytest.raises(AssertionError, match="two rows"):
        BO.assert_distinct(dup, index, M, pitch, 2)


def test_images_differ_from_their_aliases():
    from tests.test_gpu_attention_patterns import make_case
    for N in (100, 196, 400):
        B = -(-BO.tall_rows(BO.PITCH) // N)
        index = BO.image_index(B, N)
        assert index.max() == BO.IMAGE_PERIOD * N - 1 and len(index) == B * N
        images = (("spike", 0), ("tie", 0), ("offset", 0), ("spike", 1), ("tie", 1))
        assert len(images) == BO.IMAGE_PERIOD
        full = np.concatenate([np.concatenate(
            [make_case(p, N, 64)[0][b * N:(b + 1) * N, c:c + 64] for c in (0, 128, 256)], axis=1)
            for p, b in images])
        for esz in (2, 4):
            BO.assert_distinct(full, index, B * N, BO.PITCH, esz,
                               clamp_rows=min(BO.WINDOW, BO.IMAGE_PERIOD * N))


# ------------------------------------------------------------------ negative controls
def gather(table, rows, pitch, esz, wrap):
    """Rows `rows` of the tall operand as a kernel with the given truncation reads them: the
    table row of the wrapped row, NaN where the wrap lands in the front guard."""
    src = rows if wrap is None else BO.wrapped_row(rows, pitch, esz, wrap)
    out = np.asarray(table, np.float32)[np.maximum(src, 0) % P].copy()
    out[src < 0] = np.nan
    return out, src


def affected(rows, pitch, esz, wrap):
    return wrap is not None and (BO.wrapped_row(rows, pitch, esz, wrap) != rows).any()


@pytest.mark.parametrize("wrap", (None,) + BO.WRAPS)
@pytest.mark.parametrize("mode,esz", [("bf16x3", 2), ("f32", 4)])
def test_gemm_emulation_with_a_wrapped_gather(mode, esz, wrap):
    """(a) gemm_designs.emulate on the rows a truncated A address delivers."""
    pitch = BO.PITCH
    M = BO.tall_rows(pitch)
    d = G.make_design(mode, P, 5, 64)
    rows, index = BO.window_rows(M, pitch), BO.row_index(M)
    want = G.cast_f32(d.expected())
    a, src = gather(d.a_read, rows, pitch, esz, wrap)
    with np.errstate(invalid="ignore"):
        got = G.emulate(a, d.b_read)
    if not affected(rows, pitch, esz, wrap):
        assert wrap is None or (mode, wrap) == ("f32", "int element index")
        BO.check_rows(got, rows, M, pitch, 4, want, index, "correct gather")
        return
    with pytest.raises(AssertionError) as e:
        BO.check_rows(got, rows, M, pitch, 4, want, index, f"{wrap}")
    msg = str(e.value)
    first = int(rows[np.flatnonzero(src != rows)[0]])
    assert f"row {first} column 0" in msg and "byte offset" in msg
    if src[src != rows][0] < 0:
        assert "NaN: read from a guard" in msg
    else:
        # the unsigned wrap: the value found is that of the row 2^32 bytes before
        assert re.search(rf"alias row {first - (1 << 32) // pitch} \(2\^32 bytes before\)", msg), msg


@pytest.mark.parametrize("wrap", (None,) + BO.WRAPS)
@pytest.mark.parametrize("pitch", PITCHES)
def test_per_row_op_with_a_wrapped_store(pitch, wrap):
    """(b) the split of a row (gemm_designs.split_bits), stored through a truncated row address
    into a bf16 operand: the row itself keeps the fill, and under a wrapped byte offset a row of
    the first window holds the value of the row 2^32 bytes after it."""
    M = BO.tall_rows(pitch)
    d = G.make_design("bf16x3", P, 5, 64)
    x = (G.bf16_value(d.a_op[:, :64]).astype(np.float64) + G.bf16_value(d.a_op[:, 64:])).astype(np.float32)
    table = np.concatenate(G.split_bits(x), axis=1).view(np.int16)
    index = BO.row_index(M)
    m = np.arange(M, dtype=np.int64)
    dst = m if wrap is None else BO.wrapped_row(m, pitch, 2, wrap)
    rows = BO.window_rows(M, pitch)
    fill = np.int16(np.array([BO.FILL_OUT] * 2, np.uint8).view(np.int16)[0])
    got = np.full((len(rows), table.shape[1]), fill, np.int16)
    landed = {int(dst[r]): int(index[r]) for r in m[np.isin(dst, rows)]}   # a later store wins
    for i, r in enumerate(rows):                             # (the last two windows overlap)
        if int(r) in landed:
            got[i] = table[landed[int(r)]]
    if wrap is None:
        BO.check_rows(got, rows, M, pitch, 2, table, index, "correct store", numbers=False)
        return
    with pytest.raises(AssertionError) as e:
        BO.check_rows(got, rows, M, pitch, 2, table, index, wrap, numbers=False)
    msg = str(e.value)
    if wrap != "int element index":                          # rows past 2^32 bytes land on rows 0 ..
        assert re.search(r"row 0 column 0 .*alias row %d \(2\^32 bytes after\)" % ((1 << 32) // pitch),
                         msg), msg
    else:
        first = int(m[dst != m][0])
        assert f"row {first} column 0" in msg, msg
    # the same comparison names the fill when given it
    bad = int(np.flatnonzero((got != table[index[rows]]).any(1) & (got == fill).all(1))[0])
    text = BO.describe(got[bad, 0], int(rows[bad]), 0, M, pitch, 2, 0, table, index, fill=fill)
    assert "never written" in text
    landed_on = int(BO.wrapped_row(int(rows[bad]), pitch, 2, wrap))
    assert f"truncated {wrap} lands on alias row {landed_on} " in text, text
    assert fill == BO.fill_value(2) and BO.fill_value(2, numbers=True) < 0


def test_clamped_last_row_is_named():
    """A row clamp off by one (the last row read for the one before it) in the last window."""
    pitch = BO.PITCH
    M = BO.tall_rows(pitch)
    d = G.make_design("bf16", P, 5, 64)
    rows, index = BO.window_rows(M, pitch), BO.row_index(M)
    a, _ = gather(d.a_read, rows, pitch, 2, None)
    a[-2] = a[-1]
    with pytest.raises(AssertionError, match=rf"row {M - 2} column .*alias row {M - 1} \(the clamped last row\)"):
        BO.check_rows(G.emulate(a, d.b_read), rows, M, pitch, 4, G.cast_f32(d.expected()), index,
                      "clamp")


# ------------------------------------------------------------------ refusals, no GPU
def test_long_sequence_attention_refuses_an_image_over_2_31_bytes():
    """The LDS-DMA attention kernel (VTD_KNOB_ATTN_VARIANT 6) addresses an image through 32-bit
    buffer offsets: N * ld * 2 >= 2^31 bytes is VTD_ERR_INVALID_ARG before any launch
    (include/vtd.h, vtd_attention).  The pointers are never dereferenced."""
    from vision_transformer_detector_amd import _lib as L
    X = 0x10000
    with L.knob(L.KNOB_ATTN_VARIANT, 6):
        for N, ldqkv, ldo in ((70000, 16384, 64), (70000, 192, 16384), (131072, 8192, 8192)):
            rc = L.lib.vtd_attention(X, 1, N, 1, 64, ldqkv, 0.5, X + 4096, ldo, L.BF16, None)
            assert rc == -1 and b"too large for the long-sequence kernel" in L.lib.vtd_last_error()
