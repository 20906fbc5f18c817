"""A JPEG writer from quantized coefficients, and designed streams for the device decoder.

A plain helper (numpy only: no GPU, no torch, no Pillow) for tests/test_jpeg_streams_host.py
and tests/test_gpu_jpeg_streams.py, written from the JPEG standard (ITU-T T.81: Annex B marker
segments, Annex C / K.2 Huffman tables, Annex F sequential and Annex G progressive entropy
coding).  Pillow's encoder only ever writes libjpeg's habits; `write_jpeg` writes what a test
dictates: the coefficients themselves, SOF0 / SOF1 / SOF2, sampling factors, component ids,
quantization tables with 8- or 16-bit entries under any id, JFIF / Adobe / COM / APPn
segments, Huffman tables that are the Annex K ones, optimal for the stream, or dictated as
(bits, values), any table ids, tables grouped per segment as asked, a restart interval in
MCUs with 0xFF fill bytes before RSTn / EOI, and for SOF2 a scan script.

Coefficients are per component int arrays [blocks_y][blocks_x][64] in zigzag order, on the
component's real block grid ceil(dw / 8) x ceil(dh / 8) or on the MCU-padded one; a real grid
is padded with zero blocks.  Non-interleaved scans cover the real grid, interleaved scans the
MCU-padded one (T.81 A.2.3 / A.2.4).

The safe-range rule.  libjpeg has two forms of its slow integer IDCT.  The C form
(jidctint.c jpeg_idct_islow) computes in 32 bits and clamps through a table indexed by
(x & 1023); that is what vtd_jpeg.hip restates.  The SIMD form, which Pillow and TF run,
holds dequantized coefficients and the pass-1 workspace in 16 bits and clamps by saturating
packs.  The two agree while
    - every dequantized coefficient fits int16,
    - every pass-1 workspace value fits int16,
    - every centred sample before the clamp lies in [-512, 511];
outside that they can differ, and TF is not available to say which one it would give.  The
SIMD form also adds two such 16-bit values before widening, so `check_safe_range` holds the
first two to 16383, half the int16 range.  Every design that sets coefficients freely
asserts the rule, and `islow_numpy` (the C form in numpy int64) is compared with Pillow's
pixels on the host, which checks the premise against the library build in use.

Scan scripts are checked to be complete: every coefficient of every component must reach
Al = 0.  libjpeg applies inter-block smoothing to incomplete progressive files and the
device does not; such files are out of scope and `write_jpeg` refuses to write them.

EOBRUN length category 14 (runs of 16384..32767 blocks) would need 16384 consecutive empty
blocks, a 1024 x 1024 gray image; the designs stop at category 11 (2048..4095).
"""
import numpy as np

# zigzag index -> natural (row-major) index of the 8x8 block
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15,
                   23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])

# ------------------------------------------------------------------ Annex K.3 tables
_AC_LUM_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209"
    "0a161718191a25262728292a3435363738393a434445464748494a535455565758595a636465"
    "666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9ea"
    "f1f2f3f4f5f6f7f8f9fa")
_AC_CHR_VALS = bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a16"
    "2434e125f11718191a262728292a35363738393a434445464748494a535455565758595a6364"
    "65666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9"
    "eaf2f3f4f5f6f7f8f9fa".replace(" ", ""))
STD_TABLES = {
    ("dc", "lum"): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ("dc", "chr"): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ("ac", "lum"): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(_AC_LUM_VALS)),
    ("ac", "chr"): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(_AC_CHR_VALS)),
}


# ------------------------------------------------------------------ Huffman tables
def code_map(bits, vals):
    """Canonical codes of a table given as (bits[1..16], values) (T.81 Annex C):
    {symbol: (code, length)}."""
    assert len(bits) == 16 and sum(bits) == len(vals) <= 256
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            assert vals[p] not in out, "symbol listed twice"
            out[vals[p]] = (code, length)
            code += 1
            p += 1
        assert code <= (1 << length), "more codes than the length allows"
        code <<= 1
    return out


def optimal_table(counts):
    """(bits, vals) of a length-limited Huffman code for symbol counts {symbol: n} by the
    procedure of T.81 K.2 (figures K.1 - K.4): a reserved 257th symbol keeps the all-ones
    code unused, code lengths above 16 are shortened pairwise."""
    freq = [0] * 257
    for s, n in counts.items():
        freq[s] = n
    if not any(freq):
        freq[0] = 1
    freq[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if freq[i]]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda i: (freq[i], -i))
        c2 = min((i for i in live if i != c1), key=lambda i: (freq[i], -i))
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    nb = [0] * (max(size) + 2)
    for s in size:
        if s:
            nb[s] += 1
    for i in range(len(nb) - 1, 16, -1):         # figure K.3: no code longer than 16 bits
        while nb[i] > 0:
            j = i - 2
            while nb[j] == 0:
                j -= 1
            nb[i] -= 2
            nb[i - 1] += 1
            nb[j + 1] += 2
            nb[j] -= 1
    nb = (nb + [0] * 17)[:17]
    i = 16
    while nb[i] == 0:
        i -= 1
    nb[i] -= 1                                    # the reserved symbol's code
    vals = [s for length in range(1, max(size) + 1) for s in range(256) if size[s] == length]
    return nb[1:17], vals


def dictated_table(symbols, lengths):
    """A (bits, vals) table in which symbols[i] gets a code of lengths[i] bits (ascending)
    and the symbols beyond `lengths` get 16-bit codes: a test dictates which symbols meet
    the 9-bit lookahead and which the 10..16-bit walk.  The lengths must leave the all-ones
    16-bit code unused (Kraft sum <= 1 - 2^-16).  One code of every length 1..16 fills the
    code space exactly, so a table of more than 16 symbols cannot have every length: 162
    AC symbols fit with lengths 2..15 once each and 16 bits for the rest."""
    symbols, lengths = list(symbols), list(lengths)
    assert lengths == sorted(lengths) and len(lengths) <= len(symbols)
    lengths += [16] * (len(symbols) - len(lengths))
    assert sum(1 << (16 - n) for n in lengths) <= (1 << 16) - 1, "code space exceeded"
    bits = [0] * 16
    for n in lengths:
        bits[n - 1] += 1
    return bits, symbols


# ------------------------------------------------------------------ entropy coding
def _nbits(v):
    return int(v).bit_length()


class _BitWriter:
    """Entropy-coded segment: bits packed MSB first, a zero byte stuffed after every 0xFF,
    1-bits padding the last byte (T.81 F.1.2.3)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.clean = 0            # bytes before stuffing

    def put(self, value, nbits):
        if not nbits:
            return
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.clean += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            pad = 8 - self.n
            self.put((1 << pad) - 1, pad)


class _Frame:
    def __init__(self, coefs, height, width, sampling):
        self.nc = len(coefs)
        self.h, self.w = height, width
        self.samp = list(sampling)
        eff = [(1, 1)] if self.nc == 1 else self.samp     # one component: never interleaved
        self.eff = eff
        self.hmax = max(s[0] for s in eff)
        self.vmax = max(s[1] for s in eff)
        self.mcux = -(-width // (8 * self.hmax))
        self.mcuy = -(-height // (8 * self.vmax))
        self.real, self.coefs = [], []
        for c, a in enumerate(coefs):
            a = np.asarray(a)
            hs, vs = eff[c]
            dw, dh = -(-width * hs // self.hmax), -(-height * vs // self.vmax)
            rbw, rbh = -(-dw // 8), -(-dh // 8)
            pbw, pbh = self.mcux * hs, self.mcuy * vs
            assert a.ndim == 3 and a.shape[2] == 64, a.shape
            assert a.shape[:2] in ((rbh, rbw), (pbh, pbw)), (c, a.shape, (rbh, rbw), (pbh, pbw))
            full = np.zeros((pbh, pbw, 64), np.int64)
            full[:a.shape[0], :a.shape[1]] = a
            self.real.append((rbh, rbw))
            self.coefs.append(full)

    def mcus(self, comps):
        """The scan's MCUs, each a list of (component, block row, block column)."""
        if len(comps) == 1:
            c = comps[0]
            rbh, rbw = self.real[c]
            return [[(c, y, x)] for y in range(rbh) for x in range(rbw)]
        out = []
        for my in range(self.mcuy):
            for mx in range(self.mcux):
                out.append([(c, my * self.eff[c][1] + v, mx * self.eff[c][0] + h)
                            for c in comps for v in range(self.eff[c][1])
                            for h in range(self.eff[c][0])])
        return out


def _amp(v, n):
    """The n appended bits of amplitude v (T.81 F.1.2.1.1: negative values as v - 1)."""
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _scan_tokens(fr, comps, ss, se, ah, al, restart, td, ta, progressive, cats):
    """The scan as tokens (table key or None for raw bits, symbol, appended value, its bit
    count), with ("rst",) between restart intervals."""
    T = []
    pred = {c: 0 for c in comps}
    eobrun = 0
    be = []                                   # buffered correction bits of the EOB run

    def emit_eobrun():
        nonlocal eobrun, be
        if eobrun:
            n = _nbits(eobrun) - 1
            cats.add(n)
            T.append((("ac", ta[comps[0]]), n << 4, eobrun & ((1 << n) - 1), n))
            eobrun = 0
        for b in be:
            T.append((None, 0, b, 1))
        be = []

    for m, mcu in enumerate(fr.mcus(comps)):
        if restart and m and m % restart == 0:
            emit_eobrun()
            T.append(("rst",))
            pred = {c: 0 for c in comps}
        for c, by, bx in mcu:
            blk = fr.coefs[c][by, bx]
            if ss == 0:
                if ah == 0:                                   # DC, first or sequential
                    v = int(blk[0]) >> al
                    d = v - pred[c]
                    pred[c] = v
                    n = _nbits(abs(d))
                    assert n <= 11, "DC difference out of range"
                    T.append((("dc", td[c]), n, _amp(d, n), n))
                else:                                         # DC refinement: one raw bit
                    T.append((None, 0, (int(blk[0]) >> al) & 1, 1))
                if progressive:
                    continue
            lo = max(ss, 1)
            key = ("ac", ta[c])
            if not progressive:                               # F.1.2.2
                run = 0
                for k in range(lo, se + 1):
                    v = int(blk[k])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        T.append((key, 0xF0, 0, 0))
                        run -= 16
                    n = _nbits(abs(v))
                    assert n <= 10, "AC coefficient out of range"
                    T.append((key, run << 4 | n, _amp(v, n), n))
                    run = 0
                if run:
                    T.append((key, 0x00, 0, 0))
            elif ah == 0:                                     # G.1.2.2 AC first
                run = 0
                for k in range(lo, se + 1):
                    v = int(blk[k])
                    a = abs(v) >> al
                    if a == 0:
                        run += 1
                        continue
                    emit_eobrun()
                    while run > 15:
                        T.append((key, 0xF0, 0, 0))
                        run -= 16
                    n = _nbits(a)
                    assert n <= 10
                    T.append((key, run << 4 | n, _amp(a if v > 0 else -a, n), n))
                    run = 0
                if run:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        emit_eobrun()
            else:                                             # G.1.2.3 AC refinement
                absv = [abs(int(blk[k])) >> al for k in range(64)]
                eob = max([k for k in range(lo, se + 1) if absv[k] == 1], default=-1)
                run, br = 0, []
                for k in range(lo, se + 1):
                    a = absv[k]
                    if a == 0:
                        run += 1
                        continue
                    while run > 15 and k <= eob:
                        emit_eobrun()
                        T.append((key, 0xF0, 0, 0))
                        run -= 16
                        T.extend((None, 0, b, 1) for b in br)
                        br = []
                    if a > 1:
                        br.append(a & 1)
                        continue
                    emit_eobrun()
                    T.append((key, run << 4 | 1, 1 if blk[k] > 0 else 0, 1))
                    T.extend((None, 0, b, 1) for b in br)
                    br = []
                    run = 0
                if run or br:
                    eobrun += 1
                    be.extend(br)
                    if eobrun == 0x7FFF:
                        emit_eobrun()
    emit_eobrun()
    return T


def check_script(script, nc):
    """Every coefficient of every component must be sent and refined down to Al = 0, each
    refinement one bit below the pass before it, the DC of a component before its AC."""
    state = [[None] * 64 for _ in range(nc)]
    for comps, ss, se, ah, al in (s for s in script if s[0] != "dri"):
        assert 0 <= ss <= se <= 63 and (ss > 0 or se == 0), "DC and AC never share a scan"
        assert ss == 0 or len(comps) == 1, "AC scans carry one component"
        for c in comps:
            assert ss == 0 or state[c][0] is not None, "AC before the component's DC"
            for k in range(ss, se + 1):
                if ah == 0:
                    assert state[c][k] is None, "coefficient sent twice"
                else:
                    assert state[c][k] == ah and al == ah - 1, "refinement out of order"
                state[c][k] = al
    assert all(v == 0 for row in state for v in row), \
        "incomplete script: libjpeg would smooth such a file, the device does not"


# ------------------------------------------------------------------ marker segments
def _seg(marker, payload=b""):
    return b"\xff" + bytes([marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _marker_seg(spec):
    kind = spec[0]
    if kind == "jfif":
        return _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    if kind == "adobe":
        return _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, spec[1]]))
    if kind == "com":
        return _seg(0xFE, spec[1])
    if kind == "app":
        return _seg(0xE0 + spec[1], spec[2])
    raise ValueError(kind)


def _dht(tables, per_segment):
    """tables: [((class, id), (bits, vals))]"""
    parts = [bytes([(1 if k[0] == "ac" else 0) << 4 | k[1]]) + bytes(bits) + bytes(vals)
             for k, (bits, vals) in tables]
    n = per_segment or len(parts) or 1
    return [_seg(0xC4, b"".join(parts[i:i + n])) for i in range(0, len(parts), n)]


def write_jpeg(coefs, height, width, *, sof=0, sampling=None, ids=None, tq=None, qtables=None,
               q16=(), markers=(("jfif",),), huffman=None, td=None, ta=None,
               tables_per_segment=0, order=("dqt", "sof", "dht"), restart=0, fill=0, script=None,
               dht_per_scan=False, between=False, marker_fill=0, stats=None):
    """The file's bytes.

    coefs      per component [blocks_y][blocks_x][64] quantized coefficients, zigzag order
    sof        0 baseline, 1 extended sequential, 2 progressive
    sampling   (H, V) per component as written into the frame header (default all (1, 1))
    ids, tq    component ids and quantization table ids per component
    qtables    {id: 64 entries in zigzag order} (default {0: all ones}); ids in q16 are
               written with 16-bit entries, as is any table with an entry above 255
    markers    ("jfif",), ("adobe", transform), ("com", bytes), ("app", n, bytes), each with
               an optional last element "before_sof" / "before_sos" (default: after SOI)
    huffman    "standard" (Annex K; component 0's tables the luminance ones), "optimal"
               (from the stream's symbol counts), or {("dc" | "ac", id): (bits, vals)};
               default "standard" for sequential files, "optimal" for progressive ones
    td, ta     DC / AC table id per component (default 0 for the first, 1 for the others)
    tables_per_segment   tables per DQT / DHT segment (0: all in one)
    order      the order of the "dqt", "sof" and "dht" groups
    restart    MCUs per restart interval (0: none); fill: 0xFF bytes before RSTn and EOI
    script     scans (components, Ss, Se, Ah, Al) and ("dri", n) entries that change the
               restart interval from the next scan on; sequential default: one scan of all
    dht_per_scan   progressive: send optimal tables before every scan, under the same ids;
               otherwise one table per id for the whole file, sent once
    between    COM and APPn segments between every pair of marker segments
    marker_fill   0xFF fill bytes before every marker segment (T.81 B.1.1.2)
    stats      a dict that receives, per scan, the restart segments' clean byte lengths
               ("segments"), and the EOBRUN length categories written ("eobrun_cats")
    """
    nc = len(coefs)
    sampling = list(sampling or [(1, 1)] * nc)
    ids = list(ids or range(1, nc + 1))
    tq = list(tq or [0] * nc)
    qtables = {k: np.asarray(v, np.int64) for k, v in (qtables or {0: np.ones(64)}).items()}
    td = list(td or [0] + [1] * (nc - 1))
    ta = list(ta or [0] + [1] * (nc - 1))
    progressive = sof == 2
    huffman = huffman or ("optimal" if progressive else "standard")
    fr = _Frame(coefs, height, width, sampling)
    if script is None:
        assert not progressive, "a progressive file needs a scan script"
        script = [(tuple(range(nc)), 0, 63, 0, 0)]
    if progressive:
        check_script(script, nc)
        assert huffman == "optimal", "the Annex K tables have no EOBn symbols"

    # scans -> tokens
    scans, cur = [], restart
    for s in script:
        if s[0] == "dri":
            cur = s[1]
            scans.append(("dri", cur))
            continue
        comps, ss, se, ah, al = s
        cats = set()
        toks = _scan_tokens(fr, list(comps), ss, se, ah, al, cur, td, ta, progressive, cats)
        scans.append((s, toks, cats))

    def counts_of(token_lists):
        cnt = {}
        for toks in token_lists:
            for t in toks:
                if t[0] not in (None, "rst"):
                    cnt.setdefault(t[0], {})
                    cnt[t[0]][t[1]] = cnt[t[0]].get(t[1], 0) + 1
        return cnt

    def tables_for(cnt):
        out = {}
        for key in sorted(cnt, key=lambda k: (k[0] == "ac", k[1])):
            if huffman == "optimal":
                out[key] = optimal_table(cnt[key])
            elif huffman == "standard":
                first = (td if key[0] == "dc" else ta)[0]
                out[key] = STD_TABLES[(key[0], "lum" if key[1] == first else "chr")]
            else:
                out[key] = huffman[key]
        return out

    all_tokens = [s[1] for s in scans if s[0] != "dri"]
    global_tabs = tables_for(counts_of(all_tokens))

    # marker segments
    groups = {"dqt": [], "sof": [], "dht": []}
    parts = []
    for t in sorted(qtables):
        wide = t in q16 or int(qtables[t].max()) > 255
        assert sof != 0 or not wide, "baseline files carry 8-bit tables"
        parts.append(bytes([(16 if wide else 0) | t]) +
                     (qtables[t].astype(">u2").tobytes() if wide else bytes(qtables[t].tolist())))
    n = tables_per_segment or len(parts)
    groups["dqt"] = [_seg(0xDB, b"".join(parts[i:i + n])) for i in range(0, len(parts), n)]
    frame = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        frame += bytes([ids[c], sampling[c][0] << 4 | sampling[c][1], tq[c]])
    groups["sof"] = [_seg(0xC0 + sof, frame)]
    if not (progressive and dht_per_scan):
        groups["dht"] = _dht(list(global_tabs.items()), tables_per_segment)
    head = [_marker_seg(m) for m in markers if m[-1] not in ("before_sof", "before_sos")]
    before_sof = [_marker_seg(m) for m in markers if m[-1] == "before_sof"]
    before_sos = [_marker_seg(m) for m in markers if m[-1] == "before_sos"]
    segs = list(head)
    for g in order:
        if g == "sof":
            segs += before_sof
        segs += groups[g]
    if restart:
        segs.append(_seg(0xDD, restart.to_bytes(2, "big")))
    segs += before_sos

    body = []                                     # (marker segments, entropy-coded bytes)
    per_scan = []
    for s in scans:
        if s[0] == "dri":
            body.append(([_seg(0xDD, s[1].to_bytes(2, "big"))], b""))
            continue
        (comps, ss, se, ah, al), toks, cats = s
        pre = []
        if progressive and dht_per_scan:
            tabs = tables_for(counts_of([toks]))
            pre += _dht(list(tabs.items()), tables_per_segment)
        else:
            tabs = global_tabs
        maps = {k: code_map(*v) for k, v in tabs.items()}
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([ids[c], td[c] << 4 | ta[c]])
        sos += bytes([ss, se, ah << 4 | al])
        pre.append(_seg(0xDA, sos))
        w = _BitWriter()
        seglens, mark, rst = [], 0, 0
        for t in toks:
            if t[0] == "rst":
                w.flush()
                seglens.append(w.clean - mark)
                mark = w.clean
                w.out += b"\xff" * fill + bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                continue
            if t[0] is not None:
                code, length = maps[t[0]][t[1]]
                w.put(code, length)
            w.put(t[2], t[3])
        w.flush()
        seglens.append(w.clean - mark)
        per_scan.append({"segments": seglens, "eobrun_cats": cats})
        body.append((pre, bytes(w.out)))
    if stats is not None:
        stats["scans"] = per_scan
        stats["symbols"] = counts_of(all_tokens)
        stats["tables"] = global_tabs

    out = bytearray(b"\xff\xd8")
    extra = [0]

    def add(seg):
        if between and len(out) > 2:
            k = extra[0]
            out.extend(_seg(0xFE, b"comment %d" % k) if k % 2 == 0
                       else _seg(0xE1 + k % 13, b"application data %d" % k))
            extra[0] += 1
        out.extend(b"\xff" * marker_fill + seg)

    for sg in segs:
        add(sg)
    for pre, ecs in body:
        for sg in pre:
            add(sg)
        out.extend(ecs)
    out.extend(b"\xff" * fill + b"\xff\xd9")
    return bytes(out)


# ------------------------------------------------------------------ IDCT restatement
_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299,
          f1847=15137, f1961=16069, f2053=16819, f2562=20995, f3072=25172)


def _islow_1d(x, shift):
    """One pass of jpeg_idct_islow over the first axis of x [8][...] (int64)."""
    f = _F
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * f["f0541"]
    tmp2 = z1 - z3 * f["f1847"]
    tmp3 = z1 + z2 * f["f0765"]
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * f["f1175"]
    tmp0, tmp1 = tmp0 * f["f0298"], tmp1 * f["f2053"]
    tmp2, tmp3 = tmp2 * f["f3072"], tmp3 * f["f1501"]
    z1, z2 = -z1 * f["f0899"], -z2 * f["f2562"]
    z3, z4 = -z3 * f["f1961"] + z5, -z4 * f["f0390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([(tmp10 + tmp3 + r) >> shift, (tmp11 + tmp2 + r) >> shift,
                     (tmp12 + tmp1 + r) >> shift, (tmp13 + tmp0 + r) >> shift,
                     (tmp13 - tmp0 + r) >> shift, (tmp12 - tmp1 + r) >> shift,
                     (tmp11 - tmp2 + r) >> shift, (tmp10 - tmp3 + r) >> shift])


def islow_numpy(coefs, qtable):
    """libjpeg's jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2) and its range
    limit table (index & 1023) in numpy int64, for coefs [..., 64] and a table of 64
    entries, both in zigzag order.  Returns the samples uint8 [..., 8, 8] and three maxima:
    the largest |dequantized coefficient|, |pass-1 workspace value| and |centred sample
    before the table| (counting -512 as 511)."""
    c = np.asarray(coefs, np.int64)
    lead = c.shape[:-1]
    nat = np.zeros(lead + (64,), np.int64)
    nat[..., ZIGZAG] = c * np.asarray(qtable, np.int64)
    blk = nat.reshape(lead + (8, 8))
    ws = np.moveaxis(_islow_1d(np.moveaxis(blk, -2, 0), 11), 0, -2)       # columns
    out = np.moveaxis(_islow_1d(np.moveaxis(ws, -1, 0), 18), 0, -1)       # rows
    i = out & 1023
    px = np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
    centred = int(max(out.max(), -out.min() - 1)) if out.size else 0
    return (px.astype(np.uint8), int(np.abs(nat).max()), int(np.abs(ws).max()), centred)


def check_safe_range(coefs, qtable):
    """The safe-range rule of the module docstring; returns islow_numpy's samples."""
    px, deq, ws, centred = islow_numpy(coefs, qtable)
    assert deq <= 16383, f"dequantized coefficient {deq} leaves the safe range"
    assert ws <= 16383, f"pass-1 workspace value {ws} leaves the safe range"
    assert centred <= 511, f"centred sample {centred} leaves [-512, 511]"
    return px


def plane_from_blocks(px, height, width):
    """Samples [by][bx][8][8] -> the image plane [height][width]."""
    by, bx = px.shape[:2]
    return px.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)[:height, :width]


# ------------------------------------------------------------------ designs
class Case:
    """One file of a design: its bytes, what Pillow must report (mode, (height, width)),
    the coefficients and tables it was written from, and the writer's statistics."""

    def __init__(self, name, data, mode, size, coefs, qtabs, stats, progressive):
        self.name, self.data, self.mode, self.size = name, data, mode, size
        self.coefs, self.qtabs, self.stats, self.progressive = coefs, qtabs, stats, progressive

    def __repr__(self):
        return f"Case({self.name})"


def make_case(name, coefs, height, width, *, check=True, **kw):
    """write_jpeg plus the safe-range rule on every component."""
    nc = len(coefs)
    qtables = kw.get("qtables") or {0: np.ones(64, np.int64)}
    tq = kw.get("tq") or [0] * nc
    if check:
        for c in range(nc):
            check_safe_range(coefs[c], qtables[tq[c]])
    stats = {}
    data = write_jpeg(coefs, height, width, stats=stats, **kw)
    mode = {1: "L", 3: "RGB", 4: "CMYK"}[nc]
    return Case(name, data, mode, (height, width), coefs, [qtables[t] for t in tq], stats,
                kw.get("sof", 0) == 2)


def nchunks_of(case, chunk_bits):
    """Restatement of make_chunks (vtd_jpeg.hip) for a sequential file: the number of
    entropy-decode chunks at a smallest chunk of `chunk_bits` bits."""
    segs = case.stats["scans"][0]["segments"]
    bits = 8 * sum(segs)
    s = max(max(64, chunk_bits) // 32 * 32, (bits + 1023) // 1024 + 31) // 32 * 32
    return sum(max(1, -(-8 * n // s)) for n in segs)


def noisy_coefs(rng, bh, bw, dc=300, low=12, nlow=6, mid=4, nmid=20, high=2, p_high=0.25):
    """Photo-like blocks that resynchronise quickly: a DC level, larger low-frequency
    values, small middle ones and sparse +-1 / +-2 above."""
    a = np.zeros((bh, bw, 64), np.int64)
    a[..., 0] = rng.integers(-dc, dc + 1, (bh, bw))
    a[..., 1:nlow] = rng.integers(-low, low + 1, (bh, bw, nlow - 1))
    a[..., nlow:nmid] = rng.integers(-mid, mid + 1, (bh, bw, nmid - nlow))
    hi = rng.integers(-high, high + 1, (bh, bw, 64 - nmid))
    a[..., nmid:] = hi * (rng.random((bh, bw, 64 - nmid)) < p_high)
    return a


def grids(height, width, sampling):
    """Real block grids (rows, columns) per component."""
    hmax = max(s[0] for s in sampling)
    vmax = max(s[1] for s in sampling)
    return [(-(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8))
            for h, v in sampling]


SAMPLINGS = {"444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)],
             "420": [(2, 2), (1, 1), (1, 1)], "gray": [(1, 1)], "cmyk": [(1, 1)] * 4}
Q8 = np.full(64, 8, np.int64)


# ---- 1. symbols and code lengths
def symbol_blocks():
    """Gray 64 x 64 (64 blocks) that together use every DC size 0..11, every AC run/size
    0/1..15/10, ZRL (also two and three in a row), EOB and a block ending at k = 63 without
    EOB; the large coefficients are spread so that the safe-range rule holds."""
    blk = np.zeros((64, 64), np.int64)
    dc, dcs = 0, []
    for s in range(1, 12):                      # sizes 1..11 up: +1, -3, +7, ..., largest of each
        d = (1 << s) - 1 if s < 11 else 1364
        dc += d if s % 2 else -d
        dcs.append(dc)
    for s in range(11, 0, -1):                  # and down: the smallest magnitude of each size
        d = 1 << (s - 1)
        dc += -d if dc > 0 else d
        dcs.append(dc)
    dcs += [dcs[-1]] * (64 - len(dcs))          # size 0 from here on
    blk[:, 0] = dcs
    todo = [(r, s) for s in range(10, 0, -1) for r in range(16)]
    for b in range(56):
        k, budget = 1, 4 * 380 - abs(int(blk[b, 0])) // 2
        for r, s in list(todo):
            v = (1 << s) - 1 if r % 2 == 0 else -(1 << (s - 1))
            if k + r <= 63 and abs(v) <= budget:
                blk[b, k + r] = v
                k += r + 1
                budget -= abs(v)
                todo.remove((r, s))
    assert not todo, todo
    blk[56, 19] = 5                             # 18 zeros: ZRL + 2/3
    blk[57, 36] = -6                            # 35 zeros: ZRL ZRL + 3/3
    blk[58, 50] = 3                             # 49 zeros: ZRL ZRL ZRL + 1/2, then EOB
    blk[59, 63] = -1                            # 62 zeros: three ZRL + 14/1, no EOB
    blk[61, 1:] = np.where(np.arange(63) % 2, 1, -1)   # ends at 63 without EOB
    blk[62, [1, 3, 40]] = [7, -2, 1]
    return blk.reshape(8, 8, 64)


AC_SYMBOLS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]


def design_symbols():
    y = symbol_blocks()
    ones = np.ones(64, np.int64)
    rng = np.random.default_rng(11)
    # chroma of the 4:2:0 file: 4 x 4 blocks with DC sizes 0..5 and a few AC symbols only,
    # so that its dictated tables can hold the code lengths the luma tables cannot
    ch = []
    for _ in range(2):
        a = np.zeros((4, 4, 64), np.int64)
        a[..., 0] = np.cumsum(rng.permutation([0, 1, -1, 2, -3, 5, -7, 12, -15, 25, -31, 3,
                                               -2, 0, 9, -20])).reshape(4, 4)
        a[..., 1] = rng.integers(-3, 4, (4, 4))
        a[..., 3] = rng.integers(-1, 2, (4, 4))
        a[0, 0, 20] = 1                         # a ZRL in chroma too
        ch.append(a)
    dict_y = {("dc", 2): dictated_table(range(12), [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16]),
              ("ac", 3): dictated_table(AC_SYMBOLS, range(2, 16))}
    dict_c = {("dc", 3): dictated_table(range(12), [1, 3, 11, 13, 15, 16]),
              ("ac", 2): dictated_table([0x00, 0x01, 0x11, 0x02, 0xF0, 0x21, 0x12, 0x31, 0x22,
                                         0x41, 0x51, 0x61, 0x71, 0x81, 0x91, 0xA1, 0xB1, 0xC1,
                                         0xD1, 0xE1, 0xF1],
                                        [1, 2, 9, 10, 11, 12, 13, 14, 15])}
    out = []
    for how, tabs in (("standard", "standard"), ("optimal", "optimal"), ("dictated", dict_y)):
        out.append(make_case(f"symbols gray {how}", [y], 64, 64, huffman=tabs, td=[2], ta=[3],
                             qtables={0: ones}))
    for how, tabs in (("standard", "standard"), ("optimal", "optimal"),
                      ("dictated", {**dict_y, **dict_c})):
        out.append(make_case(f"symbols 4:2:0 {how}", [y] + ch, 64, 64, sampling=SAMPLINGS["420"],
                             huffman=tabs, td=[2, 3, 3], ta=[3, 2, 2], qtables={0: ones}))
    return out


# ---- 2. range limit and wide tables
def design_range():
    """Gray 32 x 32: centred samples from -500 to +500 through both clamp regions, DC-only
    blocks, blocks with one low AC coefficient and mixed ones; with an 8-bit table of 8s, and
    as SOF1 with a 16-bit table (256..300 at low frequencies, up to 1000 against +-1)."""
    a = np.zeros((16, 64), np.int64)
    a[:11, 0] = [-500, -400, -200, -129, -128, -127, 127, 128, 129, 300, 500]
    a[11, 1], a[12, 2], a[13, 4] = 350, -350, 250
    a[14, [0, 1, 2, 5]] = [250, 80, -50, 30]
    a[15, [0, 1, 3, 8]] = [-260, -80, 50, -30]
    out = [make_case("range 8-bit table", [a.reshape(4, 4, 64)], 32, 32, qtables={0: Q8})]
    q = np.array([256, 260, 270, 280, 290, 300] + [300 + 12 * (k - 5) for k in range(6, 63)]
                 + [1000], np.int64)
    b = np.zeros((16, 64), np.int64)
    b[:, 0] = [-15, -12, -9, -5, -4, -3, 3, 4, 5, 9, 12, 15, 0, 0, 2, -2]
    b[12, [1, 63]] = [4, 1]
    b[13, [2, 62, 63]] = [-4, -1, 1]
    b[14, [1, 3, 30, 50]] = [3, -2, 1, -1]
    b[15, [2, 4, 5, 40, 63]] = [-3, 2, 1, 1, -1]
    b[3, 63], b[8, 45] = -1, 1
    out.append(make_case("range SOF1 16-bit table", [b.reshape(4, 4, 64)], 32, 32, sof=1,
                         qtables={0: q}, q16={0}, huffman="optimal"))
    out.append(make_case("range SOF2 16-bit table", [b.reshape(4, 4, 64)], 32, 32, sof=2,
                         qtables={0: q}, q16={0},
                         script=[((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0), ((0,), 0, 0, 1, 0)]))
    return out


# ---- 3. periodic streams
_PERIOD = [dict(zip((1, 2, 4, 7, 10), v)) for v in
           ((5, -3, 2, -1, 1), (-4, 6, -1, 2, -1), (3, 3, -2, -1, 2))]


def periodic_blocks(bh, bw, period, dcs=(40, -25, 10)):
    a = np.zeros((bh * bw, 64), np.int64)
    for i in range(bh * bw):
        p = i % period
        a[i, 0] = dcs[p]
        for k, v in _PERIOD[p].items():
            a[i, k] = v
    return a.reshape(bh, bw, 64)


def design_periodic():
    """Identical blocks make a periodic bit string: a chunk that starts at a wrong guess can
    decode it consistently out of phase to its end, so only the iteration "until no thread
    changes" puts it right.  Gray 352 x 352 with the same five AC coefficients in every
    block (about 40 bits per block with the Annex K tables: more than 1024 chunks of 64
    bits), the same with periods of two and three blocks, a flat gray 128 x 128 (6 bits per
    block), and a 4:2:0 image whose MCUs repeat."""
    out = [make_case(f"periodic gray 352x352 period {p}", [periodic_blocks(44, 44, p)], 352, 352)
           for p in (1, 2, 3)]
    flat = np.zeros((16, 16, 64), np.int64)
    flat[..., 0] = 77
    out.append(make_case("periodic flat gray 128x128", [flat], 128, 128))
    y = periodic_blocks(12, 12, 1)
    cb = periodic_blocks(6, 6, 1, dcs=(-30,))
    cr = periodic_blocks(6, 6, 1, dcs=(55,))
    cr[..., 2] = 4
    out.append(make_case("periodic 4:2:0 96x96", [y, cb, cr], 96, 96, sampling=SAMPLINGS["420"]))
    return out


# ---- 4. restart intervals
def design_restart():
    """DRI in {1, 2, 3, 7, mcux - 1, mcux + 1, more than all MCUs} on 40 x 72 images in
    4:4:4, 4:2:2, 4:2:0 and gray and a 24 x 40 CMYK one: nine and more intervals (RSTn
    wraps), short last intervals, intervals that do not divide the MCU row, and 0, 1 or 3
    fill bytes before the markers."""
    out, n = [], 0
    for layout, (h, w) in (("444", (40, 72)), ("422", (40, 72)), ("420", (40, 72)),
                           ("gray", (40, 72)), ("cmyk", (24, 40))):
        samp = SAMPLINGS[layout]
        rng = np.random.default_rng(40 + len(out))
        coefs = [noisy_coefs(rng, *g) for g in grids(h, w, samp)]
        hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
        mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
        for dri in (1, 2, 3, 7, mcux - 1, mcux + 1, mcux * mcuy + 5):
            fill = (0, 1, 3)[n % 3]
            n += 1
            out.append(make_case(f"restart {layout} {h}x{w} DRI {dri} fill {fill}", coefs, h, w,
                                 sampling=samp, restart=dri, fill=fill,
                                 markers=(("adobe", 0),) if layout == "cmyk" else (("jfif",),),
                                 huffman="optimal" if n % 2 else "standard"))
    return out


def heavy_blocks(rng, bh, bw):
    """About 300 bits per block: 21 coefficients of 6 bits each."""
    a = np.zeros((bh, bw, 64), np.int64)
    a[..., 0] = rng.integers(-200, 201, (bh, bw))
    a[..., 1:22] = rng.integers(32, 64, (bh, bw, 21)) * rng.choice([-1, 1], (bh, bw, 21))
    return a


def design_restart_many():
    """More restart segments than the 1024 threads of the entropy decoder, so that every
    thread takes a run of two or three chunks: DRI = 1 on gray 264 x 264 (1089 segments) and
    368 x 368 (2116), and on 4:2:0 528 x 528 (1089 MCUs); and heavy blocks (about 300 bits)
    with DRI = 2 on gray 96 x 144, where at 64-bit chunks the runs mix segment starts with
    segments of several chunks."""
    rng = np.random.default_rng(77)
    out = [make_case(f"restart gray {s}x{s} DRI 1", [noisy_coefs(rng, s // 8, s // 8)], s, s,
                     restart=1) for s in (264, 368)]
    coefs = [noisy_coefs(rng, *g) for g in grids(528, 528, SAMPLINGS["420"])]
    out.append(make_case("restart 4:2:0 528x528 DRI 1", coefs, 528, 528,
                         sampling=SAMPLINGS["420"], restart=1, fill=1))
    out.append(make_case("restart heavy gray 96x144 DRI 2", [heavy_blocks(rng, 12, 18)], 96, 144,
                         restart=2))
    return out


# ---- 5. progressive scripts
def prog_scripts(nc):
    """name -> (script, writer options) for nc components."""
    comps = tuple(range(nc))
    dc = [(comps, 0, 0, 0, 0)]

    def ac(bands, order=comps):
        return [((c,), lo, hi, 0, 0) for c in order for lo, hi in bands]

    sa = [(comps, 0, 0, 0, 3)] + [(comps, 0, 0, a, a - 1) for a in (3, 2, 1)]
    for c in comps:
        sa += [((c,), 1, 63, 0, 3)] + [((c,), 1, 63, a, a - 1) for a in (3, 2, 1)]
    split_dc = [((0,), 0, 0, 0, 0)] + ([((1, 2), 0, 0, 0, 0)] if nc == 3 else [])
    full = dc + ac([(1, 63)])
    return {
        "one AC scan per component": (full, {}),
        "narrow bands": (dc + ac([(1, 1), (2, 2), (3, 5), (6, 63)]), {}),
        "successive approximation 3..0": (sa, {}),
        "DC Y alone then Cb Cr": (split_dc + ac([(1, 63)]), {}),
        "chroma AC before luma": (dc + ac([(1, 5), (6, 63)], comps[::-1]), {}),
        "tables before every scan": (sa, dict(dht_per_scan=True, ta=[0] * nc, td=[0] * nc)),
        "DRI 2, then 5, then 0": (dc + [("dri", 5)] + ac([(1, 63)])[:1] + [("dri", 0)] +
                                  ac([(1, 63)])[1:] if nc > 1 else
                                  dc + [("dri", 5)] + ac([(1, 9)]) + [("dri", 0)] + ac([(10, 63)]),
                                  dict(restart=2)),
    }


PROG_LAYOUTS = [("420", 48, 56), ("444", 48, 56), ("gray", 48, 56), ("420", 17, 17)]


def prog_coefs(layout, h, w):
    """Rich in +-1 and +-2 at high frequencies, larger values below; tables of 8s."""
    rng = np.random.default_rng(500 + h)
    return [noisy_coefs(rng, *g, dc=40, low=12, nlow=6, mid=4, nmid=20, high=2, p_high=0.6)
            for g in grids(h, w, SAMPLINGS[layout])]


def design_progressive():
    out = []
    for layout, h, w in PROG_LAYOUTS:
        coefs = prog_coefs(layout, h, w)
        for name, (script, kw) in prog_scripts(len(coefs)).items():
            out.append(make_case(f"progressive {layout} {h}x{w} {name}", coefs, h, w, sof=2,
                                 sampling=SAMPLINGS[layout], script=script,
                                 qtables={0: Q8}, **kw))
    return out


def _runs(n, lengths, values, ks, rng):
    """n blocks: empty runs of the given lengths, one separator block between them (and a
    last run to the end) carrying `values` at positions drawn from ks.  A separator's own
    end of band counts into the EOBRUN that follows it, so a run of ln empty blocks after a
    separator is written as an EOBRUN of ln + 1 (length 0 gives category 0)."""
    a = np.zeros((n, 64), np.int64)
    i = 0
    for ln in lengths:
        i += ln
        a[i, rng.choice(ks, 2, replace=False)] = rng.choice(values, 2)
        i += 1
    assert i < n
    return a


def design_eobrun():
    """Gray 384 x 384, 2304 blocks, three AC bands each sent at Al = 1 and refined to 0.
    Bands 1..5 and 21..63 hold +-2 / +-3 in separator blocks: their first scans see empty
    runs of every length category between them, their refinement scans one run over all
    2304 blocks (category 11) that carries the separators' correction bits.  Band 6..20
    holds +-1 in its separators: its first scan is one run of 2304, its refinement scan sees
    the runs.  Together: categories 0..11 in first scans and in refinement scans."""
    rng = np.random.default_rng(5)
    n = 48 * 48
    a = np.zeros((n, 64), np.int64)
    a[:, 0] = rng.integers(-60, 61, n)
    a += _runs(n, [2048, 0, 2, 4, 8, 16, 33, 64], [2, -2, 3, -3], np.arange(1, 6), rng)
    a += _runs(n, [128, 300, 512, 1024, 0, 2, 4, 8, 16, 32, 64], [1, -1], np.arange(6, 21), rng)
    a += _runs(n, [130, 256, 600, 1100], [2, -2, 3, -3], np.arange(21, 64), rng)
    script = [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0)]
    for lo, hi in ((1, 5), (6, 20), (21, 63)):
        script += [((0,), lo, hi, 0, 1), ((0,), lo, hi, 1, 0)]
    return [make_case("eobrun gray 384x384", [a.reshape(48, 48, 64)], 384, 384, sof=2,
                      script=script, qtables={0: Q8})]


# ---- 6. colour space
def colour_coefs(layout):
    dcs = [[400, -400, 100, 0], [-300, 300, 500, -500], [600, -100, -600, 250],
           [300, -200, 100, 500]]
    out = []
    for c, g in enumerate(grids(16, 16, SAMPLINGS[layout])):
        a = np.zeros(g + (64,), np.int64)
        a[..., 0] = np.array(dcs[c][:g[0] * g[1]]).reshape(g)
        a[..., 1] = 20 - 10 * c
        a[..., 2] = -15 + 8 * c
        out.append(a)
    return out


COLOUR_CASES3 = [  # (name, markers, component ids)
    ("no markers, ids 1 2 3", (), (1, 2, 3)),
    ("no markers, ids R G B", (), (82, 71, 66)),
    ("no markers, ids 0 1 2", (), (0, 1, 2)),
    ("no markers, ids 10 20 30", (), (10, 20, 30)),
    ("JFIF", (("jfif",),), (1, 2, 3)),
    ("Adobe transform 0", (("adobe", 0),), (1, 2, 3)),
    ("Adobe transform 1", (("adobe", 1),), (1, 2, 3)),
    ("JFIF and Adobe transform 0", (("jfif",), ("adobe", 0)), (1, 2, 3)),
    ("JFIF, ids R G B", (("jfif",),), (82, 71, 66)),
]
COLOUR_CASES4 = [("no Adobe", ()), ("Adobe transform 0", (("adobe", 0),)),
                 ("Adobe transform 1", (("adobe", 1),)), ("Adobe transform 2", (("adobe", 2),))]


def design_colour():
    out = []
    for layout in ("444", "420"):
        coefs = colour_coefs(layout)
        for name, markers, ids in COLOUR_CASES3:
            out.append(make_case(f"colour {layout} {name}", coefs, 16, 16, ids=ids,
                                 sampling=SAMPLINGS[layout], markers=markers))
    coefs = colour_coefs("cmyk")
    for name, markers in COLOUR_CASES4:
        out.append(make_case(f"colour 4 components {name}", coefs, 16, 16, markers=markers,
                             sampling=SAMPLINGS["cmyk"]))
    return out


# ---- 7. headers
def design_headers():
    rng = np.random.default_rng(9)
    gray = [noisy_coefs(rng, 3, 3)]
    out = [make_case(f"headers gray 17x23 SOF sampling {s[0]}x{s[1]}", gray, 17, 23,
                     sampling=[s], qtables={0: Q8}) for s in ((2, 2), (2, 1))]
    coefs = [noisy_coefs(rng, *g, dc=30, low=6, mid=2, high=1)
             for g in grids(24, 40, SAMPLINGS["420"])]
    qt = {3: Q8 + np.arange(64) // 8, 0: Q8 + 3, 2: Q8 + np.arange(64) % 5, 1: Q8 * 2}
    kw = dict(sampling=SAMPLINGS["420"], tq=[3, 0, 2], qtables=qt, td=[0, 1, 2], ta=[1, 3, 0])
    for name, extra in (("all tables in one DQT and one DHT", dict(tables_per_segment=0)),
                        ("one table per segment", dict(tables_per_segment=1)),
                        ("DQT and DHT after SOF", dict(order=("sof", "dht", "dqt"),
                                                       tables_per_segment=2)),
                        ("COM and APPn between all segments", dict(between=True,
                                                                   tables_per_segment=1)),
                        ("optimal tables, ids 7 200 255", dict(huffman="optimal",
                                                               ids=(7, 200, 255)))):
        out.append(make_case(f"headers 4:2:0 24x40 {name}", coefs, 24, 40, **kw, **extra))
    out.append(make_case("headers progressive, COM and APPn everywhere", coefs, 24, 40, sof=2,
                         script=prog_scripts(3)["narrow bands"][0], between=True,
                         dht_per_scan=True, **kw))
    out.append(make_case("headers fill bytes before every marker", coefs, 24, 40, marker_fill=2,
                         restart=2, fill=2, **kw))
    out.append(make_case("headers progressive, fill bytes before every marker", coefs, 24, 40,
                         sof=2, script=prog_scripts(3)["narrow bands"][0], marker_fill=3,
                         dht_per_scan=True, **kw))
    out.append(make_case("headers progressive gray 17x23 SOF sampling 2x2", gray, 17, 23, sof=2,
                         sampling=[(2, 2)], qtables={0: Q8},
                         script=prog_scripts(1)["successive approximation 3..0"][0]))
    # markers that libjpeg reads where they stand: an Adobe segment between SOF and SOS
    # still counts; an APP0 that says JFIF but is shorter than a JFIF header does not
    rgb = colour_coefs("444")
    out.append(make_case("headers Adobe transform 0 just before SOS", rgb, 16, 16,
                         markers=(("adobe", 0, "before_sos"),)))
    out.append(make_case("headers short APP0 'JFIF' (no JFIF marker), ids R G B", rgb, 16, 16,
                         ids=(82, 71, 66), markers=(("app", 0, b"JFIF\0\1\1\0\0\1\0\1"),)))
    return out


DESIGNS = {"symbols": design_symbols, "range": design_range, "periodic": design_periodic,
           "restart": design_restart, "restart_many": design_restart_many,
           "progressive": design_progressive, "eobrun": design_eobrun,
           "colour": design_colour, "headers": design_headers}
_cache = {}


def design(name):
    """The cases of a design, built once per process."""
    if name not in _cache:
        _cache[name] = DESIGNS[name]()
    return _cache[name]
