"""Operands whose last row lies more than 2^32 bytes from their base: the arena, the periodic
row data and the comparisons of tests/test_gpu_big_operands.py (no test functions here;
tests/test_big_operands_host.py checks this module on the CPU).

The arena.  One device allocation per test module:

    front guard   4 GiB
    span          2^32 bytes + 64 MiB     every tall operand is a view [rows][pitch] from its start
    back guard    64 MiB

Why the front guard is 4 GiB: a kernel that truncates a row address to 32 bits must give a wrong
answer the test can read, not a fault on a shared machine.  Relative to the operand's base,
  a signed 32-bit BYTE offset wraps to at most 2^31 bytes (2 GiB) before the base;
  an `int` ELEMENT index into bf16 wraps to at most 2^31 elements = 2^32 bytes (4 GiB) before it
  (into fp32 it would be 8 GiB, but no fp32 operand here has 2^31 elements: 2^32 bytes + 64 MiB
  are 1.09e9 floats);
  an unsigned wrap of either lands inside the operand itself.
So every wrapped access falls into memory the test owns and has filled.  The back guard takes an
overrun past the last row (64 MiB: 4096 rows of the widest pitch).

Fill and check.  Before a call the whole arena is filled on the device: the byte 0xA5, and 0xFF
(a NaN in fp32, bf16 and e4m3) in the column bands of the inputs -- in every row of the arena, the
guards included, so that a wrapped read meets NaN.  Then the inputs' rows are written: row m of
every tall operand is row index[m] of a small designed table (gathered on the device; nothing of
the operand's size exists on the host).  After the call `Arena.guard_count` counts, on the device,
the bytes that differ from that fill outside what the contract writes, and the input elements that
changed; both must be 0.  What the contract writes is compared by `Arena.compare`.

Row data.  index[m] = m mod P with P = 1021, an odd prime: a row and its alias under any of the
wraps above are 2^k rows apart, and 2^k mod P != 0, so they hold different rows of the table
(`alias_rows`, `assert_distinct`); the table's rows are pairwise distinct by design.  For the
attention kernels the unit is an image: image b is image b mod IMAGE_PERIOD of the designed
images (`image_index`).

Pitch: 16 KiB (a 4096-wide fp32 row, an 8192-wide [hi | lo] bf16 row) with 2^32 / 16384 + 333 =
262,477 rows; 8 KiB with 524,621 rows where an entry point writes the whole leading dimension.
"""
import numpy as np

GIB, MIB = 1 << 30, 1 << 20
FRONT_GUARD = 4 * GIB
SPAN = (1 << 32) + 64 * MIB
BACK_GUARD = 64 * MIB
ARENA_BYTES = FRONT_GUARD + SPAN + BACK_GUARD
HEADROOM = 2 * GIB                       # free memory asked for beyond the arena
P = 1021                                 # rows of the designed table: an odd prime
IMAGE_PERIOD = 5
PITCH, PITCH_TIED = 16384, 8192
EXTRA_ROWS = 333
WINDOW = 512
FILL_OUT, FILL_IN = 0xA5, 0xFF
CHUNK_BYTES = 128 * MIB                  # device temporaries of the fill / check loops


# ------------------------------------------------------------------ layout arithmetic (pure)
def tall_rows(pitch):
    """The ragged row count: the operand ends EXTRA_ROWS rows past byte offset 2^32."""
    return (1 << 32) // pitch + EXTRA_ROWS


def layout(pitch):
    """Rows of `pitch` bytes in each region of the arena, and the span's first row."""
    assert FRONT_GUARD % pitch == 0 and SPAN % pitch == 0 and BACK_GUARD % pitch == 0
    return dict(base_byte=FRONT_GUARD, base_row=FRONT_GUARD // pitch, span_rows=SPAN // pitch,
                back_rows=BACK_GUARD // pitch, total_rows=ARENA_BYTES // pitch)


def windows(M, pitch, width=WINDOW):
    """The four row windows copied to the host: (name, first row, end row)."""
    r31, r32 = (1 << 31) // pitch, (1 << 32) // pitch
    assert M >= r32 + width // 2 and r31 - width // 2 >= width
    return [("first", 0, width), ("across 2^31 bytes", r31 - width // 2, r31 + width // 2),
            ("across 2^32 bytes", r32 - width // 2, min(r32 + width // 2, M)),
            ("last", M - width, M)]


def window_rows(M, pitch):
    return np.concatenate([np.arange(a, b) for _, a, b in windows(M, pitch)])


def wrap_s32(v):
    """v truncated to a signed 32-bit integer (numpy int64 in, int64 out)."""
    v = np.asarray(v, np.int64) & 0xFFFFFFFF
    return np.where(v >= 1 << 31, v - (1 << 32), v)


def wrap_u32(v):
    return np.asarray(v, np.int64) & 0xFFFFFFFF


WRAPS = ("signed byte offset", "unsigned byte offset", "int element index")


def wrapped_row(m, pitch, esz, wrap):
    """The row a kernel with a 32-bit-truncated row address reaches instead of row m (negative:
    in the front guard).  The leading dimension is the pitch, in elements of esz bytes."""
    m = np.asarray(m, np.int64)
    if wrap == "signed byte offset":
        return wrap_s32(m * pitch) // pitch
    if wrap == "unsigned byte offset":
        return wrap_u32(m * pitch) // pitch
    if wrap == "int element index":
        ld = pitch // esz
        return wrap_s32(m * ld) // ld
    raise ValueError(wrap)


def alias_rows(m, M, pitch, esz):
    """name -> the row whose content a mis-addressed access to row m would show (may be
    negative: the front guard)."""
    ld = pitch // esz
    out = {}
    for name, rows in (("2^31 bytes", (1 << 31) // pitch), ("2^32 bytes", (1 << 32) // pitch),
                       ("2^31 elements", (1 << 31) // ld), ("2^32 elements", (1 << 32) // ld)):
        out[name + " before"] = m - rows           # a wrapped read of row m
        out[name + " after"] = m + rows            # a wrapped write of that row, landed on row m
    out["the clamped last row"] = M - 1
    return out


def row_index(M, period=P):
    return np.arange(M, dtype=np.int64) % period


def image_index(B, N, period=IMAGE_PERIOD):
    """Row b N + t of B images of N tokens -> row (b mod period) N + t of `period` images."""
    m = np.arange(B * N, dtype=np.int64)
    return (m // N) % period * N + m % N


def assert_distinct(table, index, M, pitch, esz, clamp_rows=WINDOW):
    """The data design does its job: the table's rows are pairwise distinct, and past each
    boundary row m holds another table row than each of its aliases (the clamped last row: over
    the last clamp_rows rows, where a clamp acts -- at most one period of the index)."""
    t = np.ascontiguousarray(table)
    t = t.reshape(t.shape[0], -1)
    rows = t.view(np.uint8).reshape(t.shape[0], -1)
    assert len(np.unique(rows, axis=0)) == len(rows), "two rows of the designed table are equal"
    index = np.asarray(index)
    assert len(index) == M and index.max() < len(rows)
    m = np.arange(M, dtype=np.int64)
    for name, a in alias_rows(m, M, pitch, esz).items():
        a = np.broadcast_to(a, m.shape)
        if name == "the clamped last row":
            sel = (m >= M - clamp_rows) & (m < M - 1)
        else:
            sel = (a >= 0) & (a < M)
            if not sel.any():
                continue                          # the operand does not reach that boundary
        assert (index[m[sel]] != index[a[sel]]).all(), f"row == its alias {name}"


# ------------------------------------------------------------------ comparison and diagnosis
def fill_value(esz, numbers=False):
    """The output fill as the comparison sees it: integer bits, or the number they encode."""
    raw = np.array([FILL_OUT] * esz, np.uint8)
    if not numbers:
        return raw.view({4: np.int32, 2: np.int16, 1: np.uint8}[esz])[0]
    if esz == 4:
        return raw.view(np.float32)[0]
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)[0]


def describe(got, m, col, M, pitch, esz, col_byte, table, index, fill=None, initial=None):
    """What the wrong value `got` at (row m, column col) of a tall operand is: its byte offset
    and the alias row, if any, that holds this value in this column.  A value that is the fill
    (or `initial`, what an in-place operand held before the call) was never written: the rows
    its store reaches under each 32-bit truncation are named instead."""
    index = np.asarray(index)
    want = table[index[m], col]
    off = m * pitch + col_byte + col * esz
    text = [f"row {m} column {col} (byte offset {off} = 2^32 {off - (1 << 32):+d}): got {got!r}, "
            f"want {want!r}"]
    unwritten = (fill is not None and got == fill) or (initial is not None and got == initial)
    if unwritten:
        text.append("the value is the arena's fill: never written" if initial is None or
                    got != initial else "the value is the operand's input: never written")
        for wrap in WRAPS:
            r = int(wrapped_row(m, pitch, esz, wrap))
            if r != m:
                where = "in the front guard" if r < 0 else "of the operand"
                text.append(f"a store through a truncated {wrap} lands on alias row {r} ({where})")
    elif got != got:
        text.append("the value is NaN: read from a guard or a pad")
    hits = []
    for name, a in alias_rows(m, M, pitch, esz).items():
        if 0 <= a < M and a != m and table[index[a], col] == got:
            hits.append(f"row {a} ({name})")
    if hits:
        text.append("it is the value of alias " + " and of ".join(hits))
    else:
        owners = np.flatnonzero(table[:, col] == got)[:4]
        if len(owners):
            text.append(f"no named alias holds it; table rows {owners.tolist()} do")
    return "; ".join(text)


def check_rows(got, rows, M, pitch, esz, table, index, what, col_byte=0, numbers=True):
    """got [len(rows)][w] (the values of the global rows `rows` of a tall operand) equals
    table[index[rows]]: as numbers (NaN never equal), or bit for bit on integer views."""
    rows = np.asarray(rows, np.int64)
    want = table[np.asarray(index)[rows]]
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        bad = ~(got == want) if numbers else got != want
    if bad.any():
        i, c = np.argwhere(bad)[0]
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} values differ, first at "
            + describe(got[i, c], int(rows[i]), int(c), M, pitch, esz, col_byte, table, index))


# ------------------------------------------------------------------ the device arena
class Piece:
    """`width` elements at byte column `col` of every row."""

    def __init__(self, col, width):
        self.col, self.width = col, width


class Field:
    """One tall operand: rows of `pieces` (one, or hi and lo of a split row) of `dtype`
    ("f32" | "bf16" | "u8").  role "in": `table` (bits, [table rows][sum of widths]) is written
    before the call and must be intact after it; "out": the pieces are what the contract writes;
    "inout": both (an in-place residual).  band: bytes from each piece's column that are NaN-filled
    for an input (its pad columns)."""

    def __init__(self, name, role, dtype, pieces, table=None, band=0):
        self.name, self.role, self.dtype, self.pieces = name, role, dtype, pieces
        self.table, self.band = table, band
        self.esz = {"f32": 4, "bf16": 2, "u8": 1}[dtype]
        for p in pieces:
            assert p.col % 8 == 0

    @property
    def col(self):
        return self.pieces[0].col


class Arena:
    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev
        self.buf = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=dev)
        self.base = self.buf.data_ptr() + FRONT_GUARD
        assert self.base % 256 == 0

    def free(self):
        self.buf = None
        self.torch.cuda.empty_cache()

    # ---- views
    def ptr(self, col=0):
        return self.base + col

    def _bits(self, esz):
        t = self.torch
        return {4: t.int32, 2: t.int16, 1: t.uint8}[esz]

    def view(self, field, piece=0, bits=True):
        """[M][width] strided view of one piece: integer bits, or the floating type."""
        t = self.torch
        p = field.pieces[piece]
        dt = self._bits(field.esz) if bits else {"f32": t.float32, "bf16": t.bfloat16,
                                                 "u8": t.uint8}[field.dtype]
        flat = self.buf[FRONT_GUARD:FRONT_GUARD + self.M * self.pitch].view(dt)
        c0 = p.col // field.esz
        return flat.view(self.M, self.pitch // field.esz)[:, c0:c0 + p.width]

    def _row_chunks(self, r0, r1, row_bytes):
        step = max(1, CHUNK_BYTES // row_bytes)
        return [(r, min(r + step, r1)) for r in range(r0, r1, step)]

    # ---- before the call
    def stage(self, pitch, M, fields, index):
        """Fill the arena, then write the inputs: row m = table[index[m]]."""
        t = self.torch
        lay = layout(pitch)
        assert M <= lay["span_rows"]
        self.pitch, self.M, self.fields, self.lay = pitch, M, fields, lay
        self.index = index if t.is_tensor(index) else t.from_numpy(np.asarray(index)).to(self.dev)
        assert self.index.shape == (M,)
        fill = np.full(pitch, FILL_OUT, np.uint8)
        written = np.zeros(pitch, bool)           # columns of the operand rows not held to the fill
        for f in fields:
            for p in f.pieces:
                if f.role != "out":
                    fill[p.col:p.col + max(f.band, p.width * f.esz)] = FILL_IN
        for f in fields:
            for p in f.pieces:
                assert not written[p.col:p.col + p.width * f.esz].any(), "fields overlap"
                written[p.col:p.col + p.width * f.esz] = True
        self.fill = t.from_numpy(fill).to(self.dev)
        self.held = t.from_numpy(~written).to(self.dev)
        rows = self.buf.view(lay["total_rows"], pitch)
        for a, b in self._row_chunks(0, lay["total_rows"], pitch // 8):
            rows[a:b] = self.fill
        for f in fields:
            if f.role == "out":
                continue
            self._write(f)

    def _write(self, f):
        c = 0
        for i, p in enumerate(f.pieces):
            v = self.view(f, i)
            for a, b in self._row_chunks(0, self.M, self.pitch):
                v[a:b] = f.table[self.index[a:b], c:c + p.width]
            c += p.width

    # ---- after the call
    def guard_count(self):
        """(bytes outside the written region that differ from the fill, input elements that
        changed) -- two device counts, one synchronisation."""
        t = self.torch
        lay, M = self.lay, self.M
        rows = self.buf.view(lay["total_rows"], self.pitch)
        r0 = lay["base_row"]
        n = t.zeros((), dtype=t.int64, device=self.dev)
        for lo, hi, held in ((0, r0, None), (r0, r0 + M, self.held),
                             (r0 + M, lay["total_rows"], None)):
            for a, b in self._row_chunks(lo, hi, self.pitch):
                ne = rows[a:b] != self.fill
                if held is not None:
                    ne &= held
                n += ne.sum()
        changed = t.zeros((), dtype=t.int64, device=self.dev)
        for f in self.fields:
            if f.role != "in":
                continue
            c = 0
            for i, p in enumerate(f.pieces):
                v = self.view(f, i)
                for a, b in self._row_chunks(0, M, self.pitch):
                    changed += (v[a:b] != f.table[self.index[a:b], c:c + p.width]).sum()
                c += p.width
        return int(n.item()), int(changed.item())

    def assert_guards(self, what):
        n, changed = self.guard_count()
        assert n == 0, f"{what}: {n} bytes outside the written region changed"
        assert changed == 0, f"{what}: {changed} input elements changed"

    def compare(self, field, table, what, numbers=False, piece=0, col0=0, index=None):
        """All M rows of one piece equal table[index[m], col0:col0 + width]: bit for bit, or as
        numbers (numbers=True: -0 == 0, NaN never equal).  On a mismatch the message names the
        first bad (row, column), its byte offset and the alias row that holds the value."""
        t = self.torch
        index = self.index if index is None else index
        p = field.pieces[piece]
        v = self.view(field, piece, bits=not numbers)
        want = table[:, col0:col0 + p.width]
        if numbers:
            want = want.view(v.dtype) if want.dtype != v.dtype else want
        counts, chunks = [], self._row_chunks(0, self.M, self.pitch)
        for a, b in chunks:
            g, w = v[a:b], want[index[a:b]]
            bad = ~(g.float() == w.float()) if numbers else g != w
            counts.append(bad.sum())
        counts = t.stack(counts).cpu().numpy()
        if not counts.any():
            return
        a, b = chunks[int(np.flatnonzero(counts)[0])]
        g, w = v[a:b], want[index[a:b]]
        bad = ~(g.float() == w.float()) if numbers else g != w
        i, c = (int(x) for x in bad.nonzero()[0])
        m = a + i
        # the diagnosis on the host, over this column of the table
        conv = (lambda x: x.float().cpu().numpy()) if numbers else (lambda x: x.cpu().numpy())
        tab = conv(want)
        initial = None
        if field.role == "inout":
            c0 = sum(q.width for q in field.pieces[:piece])
            init = field.table[index[m], c0 + c]
            initial = conv(init.view(v.dtype) if numbers else init).item()
        raise AssertionError(
            f"{what} ({field.name}): {int(counts.sum())} of {self.M * p.width} values differ, "
            f"first at " + describe(conv(g[i, c]).item(), m, c, self.M, self.pitch, field.esz,
                                    p.col, tab, index.cpu().numpy(),
                                    fill_value(field.esz, numbers).item(), initial))

    def window(self, field, a, b, piece=0):
        """Rows [a, b) of one piece on the host, as integer bits."""
        return self.view(field, piece)[a:b].cpu().numpy()
