"""The JPEG writer of tests/jpeg_streams.py and its designed streams, checked without a GPU:
every design loads under Pillow (libjpeg-turbo) with the stated size and mode; one
coefficient set gives the same pixels however it is written; the numpy restatement of
libjpeg's slow integer IDCT equals Pillow's pixels on every gray design, which confirms the
safe-range premise on the library build in use; the expected pixels depend on what a design
exercises (one quantum, one refinement bit); the designs reach the symbols, code lengths,
EOBRUN categories and chunk counts they are built for; and the decoder's host entry points
accept every design and still refuse the documented flavours by name."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_streams as J


def _pil(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _pixels(data):
    return np.asarray(_pil(data))


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


# ------------------------------------------------------------------ the writer
def test_standard_tables_are_the_ones_libjpeg_writes():
    """The Annex K tables as typed into the helper equal the DHT segments of a file Pillow
    writes without optimize (libjpeg's std_huff_tables)."""
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, format="JPEG")
    f, found, pos = b.getvalue(), {}, 2
    while f[pos + 1] != 0xDA:
        ln = int.from_bytes(f[pos + 2:pos + 4], "big")
        if f[pos + 1] == 0xC4:
            p = pos + 4
            while p < pos + 2 + ln:
                bits = list(f[p + 1:p + 17])
                found[f[p]] = (bits, list(f[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        pos += 2 + ln
    assert found == {0x00: J.STD_TABLES[("dc", "lum")], 0x01: J.STD_TABLES[("dc", "chr")],
                     0x10: J.STD_TABLES[("ac", "lum")], 0x11: J.STD_TABLES[("ac", "chr")]}


def test_optimal_table_is_a_prefix_code_within_16_bits():
    rng = np.random.default_rng(0)
    for counts in ({5: 1}, {0: 10, 1: 1}, {s: int(1.6 ** (s % 40)) for s in range(200)},
                   {s: int(rng.integers(1, 1000)) for s in range(256)}):
        bits, vals = J.optimal_table(counts)
        assert sorted(vals) == sorted(counts) and sum(bits) == len(vals)
        codes = J.code_map(bits, vals)
        assert all(n <= 16 and c < (1 << n) - 1 for c, n in codes.values())   # never all ones
        assert sum(2.0 ** -n for _, n in codes.values()) < 1.0
        # no code is a prefix of another
        words = sorted(format(c, "0%db" % n) for c, n in codes.values())
        assert not any(b2.startswith(a) for a, b2 in zip(words, words[1:]))


def test_incomplete_scripts_are_refused():
    coefs = J.prog_coefs("gray", 48, 56)
    with pytest.raises(AssertionError, match="incomplete script"):
        J.write_jpeg(coefs, 48, 56, sof=2, script=[((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)])
    with pytest.raises(AssertionError, match="incomplete script"):
        J.write_jpeg(coefs, 48, 56, sof=2, script=[((0,), 0, 0, 0, 0), ((0,), 1, 5, 0, 0)])
    with pytest.raises(AssertionError, match="out of order"):
        J.write_jpeg(coefs, 48, 56, sof=2, script=[((0,), 0, 0, 0, 2), ((0,), 0, 0, 1, 0)])


def test_safe_range_rule_refuses_what_leaves_it():
    a = np.zeros((1, 1, 64), np.int64)
    a[0, 0, 4] = 2500                               # centred samples of about +-600
    with pytest.raises(AssertionError, match="centred sample"):
        J.check_safe_range(a, np.ones(64, np.int64))
    a[0, 0, 4] = 0
    a[0, 0, 0] = 600
    with pytest.raises(AssertionError, match="workspace"):
        J.check_safe_range(a, J.Q8)
    a[0, 0, 0] = 3
    with pytest.raises(AssertionError, match="dequantized"):
        J.check_safe_range(a, np.full(64, 6000))


# ------------------------------------------------------------------ round trip
@pytest.mark.parametrize("name", list(J.DESIGNS))
def test_every_design_loads_under_pillow(name):
    for c in J.design(name):
        im = _pil(c.data)
        assert (im.height, im.width) == c.size and im.mode == c.mode, c
        assert (b"\xff\xc2" in c.data) == c.progressive, c


@pytest.mark.parametrize("name", [n for n in J.DESIGNS if n != "colour"])
def test_islow_numpy_equals_pillow_on_gray_designs(name):
    """The C form of the IDCT restated in numpy gives the pixels of the SIMD form Pillow
    runs: inside the safe range the two agree, on this library build.  (Every design but the
    colour one has gray files.)"""
    gray = [c for c in J.design(name) if c.mode == "L"]
    assert gray
    for c in gray:
        px, deq, ws, centred = J.islow_numpy(c.coefs[0], c.qtabs[0])
        assert deq <= 16383 and ws <= 16383 and centred <= 511
        mine = J.plane_from_blocks(px, *c.size)
        ref = _pixels(c.data)
        bad = np.argwhere(mine != ref)
        assert bad.size == 0, (f"{c.name}: {len(bad)} differing samples, first at "
                               f"{bad[0].tolist()}: {mine[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")


def test_range_design_reaches_both_clamp_regions():
    for c in J.design("range"):
        _, _, _, centred = J.islow_numpy(c.coefs[0], c.qtabs[0])
        px = _pixels(c.data)
        assert centred >= 450 and (px == 0).any() and (px == 255).any(), (c, centred)
    assert int(J.design("range")[1].qtabs[0].max()) == 1000
    assert b"\xff\xc1" in J.design("range")[1].data


# ------------------------------------------------------------------ writer consistency
def _dictated(keys):
    return {k: (J.dictated_table(range(12), [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16])
                if k[0] == "dc" else J.dictated_table(J.AC_SYMBOLS, range(2, 16))) for k in keys}


@pytest.mark.parametrize("layout,h,w", J.PROG_LAYOUTS)
def test_one_coefficient_set_gives_one_image_however_written(layout, h, w):
    coefs = J.prog_coefs(layout, h, w)
    nc = len(coefs)
    kw = dict(sampling=J.SAMPLINGS[layout], qtables={0: J.Q8})
    ref = _pixels(J.write_jpeg(coefs, h, w, **kw))
    keys = [("dc", 0), ("ac", 0)] + ([("dc", 1), ("ac", 1)] if nc > 1 else [])
    ways = {"optimal": dict(huffman="optimal"), "dictated": dict(huffman=_dictated(keys)),
            "SOF1": dict(sof=1), "restart 1": dict(restart=1),
            "restart 3, fill 2": dict(restart=3, fill=2),
            "restart 1000": dict(restart=1000, fill=1),
            "tables 1 per segment": dict(tables_per_segment=1),
            "COM / APPn between": dict(between=True), "marker fill": dict(marker_fill=2)}
    for name, (script, extra) in J.prog_scripts(nc).items():
        ways["progressive " + name] = dict(sof=2, script=script, **extra)
    ways["progressive, restart 4"] = dict(sof=2, script=J.prog_scripts(nc)["narrow bands"][0],
                                          restart=4, fill=1)
    for name, extra in ways.items():
        got = _pixels(J.write_jpeg(coefs, h, w, **kw, **extra))
        assert np.array_equal(got, ref), f"{layout} {h}x{w} written as {name}"


def test_symbol_design_files_agree():
    cases = J.design("symbols")
    for group in (cases[:3], cases[3:]):
        px = [_pixels(c.data) for c in group]
        assert all(np.array_equal(p, px[0]) for p in px[1:])


# ------------------------------------------------------------------ what the designs reach
def test_symbol_design_uses_every_symbol_and_code_length():
    cases = J.design("symbols")
    for c in cases:
        sym = c.stats["symbols"]
        assert set(sym[("dc", 2)]) == set(range(12)), c
        assert set(sym[("ac", 3)]) == set(J.AC_SYMBOLS), c
    y = J.symbol_blocks().reshape(64, 64)
    assert y[59, 63] != 0 and y[61, 63] != 0                   # blocks that end without EOB
    assert not y[56, 1:19].any() and not y[57, 1:36].any() and not y[58, 1:50].any()   # 1, 2, 3 ZRL
    # dictated tables: the code lengths of the symbols that occur
    used = {"dc": set(), "ac": set()}
    c = cases[5]
    for key, counts in c.stats["symbols"].items():
        codes = J.code_map(*c.stats["tables"][key])
        used[key[0]] |= {codes[s][1] for s in counts}
    assert used["dc"] == set(range(1, 17)) and used["ac"] == set(range(1, 17)), used
    gray = cases[2]
    for key, counts in gray.stats["symbols"].items():
        codes = J.code_map(*gray.stats["tables"][key])
        lens = {codes[s][1] for s in counts}
        assert min(lens) <= 9 and max(lens) == 16 and len(lens) >= 12, (key, lens)


def test_eobrun_design_reaches_every_category():
    (c,) = J.design("eobrun")
    scans = c.stats["scans"]
    first = set().union(*[scans[i]["eobrun_cats"] for i in (2, 4, 6)])
    refine = set().union(*[scans[i]["eobrun_cats"] for i in (3, 5, 7)])
    assert first == set(range(12)) and refine == set(range(12)), (first, refine)


def test_progressive_design_refinements_meet_nonzero_history():
    """The successive-approximation scripts refine over many already-nonzero coefficients
    and write ZRL inside refinement scans."""
    c = [c for c in J.design("progressive") if "420 48x56 successive" in c.name][0]
    y = c.coefs[0]
    assert (np.abs(y[..., 1:]) >= 8).sum() > 50 and (np.abs(y[..., 20:]) == 1).sum() > 200
    assert any(0xF0 in counts for key, counts in c.stats["symbols"].items() if key[0] == "ac")


def test_sizing_of_the_chunked_designs(capsys):
    """ceil(chunks / 1024) of the restart designs, chunks restated from make_chunks: the
    many-segment files give every decoder thread two and three chunks at both settings, the
    heavy file two at 64-bit chunks; the periodic files hold more than 1024 chunks' worth of
    bits at 64."""
    want = {"restart gray 264x264 DRI 1": (1089, 2, 2),
            "restart gray 368x368 DRI 1": (2116, 3, 3),
            "restart 4:2:0 528x528 DRI 1": (1089, 2, 2),
            "restart heavy gray 96x144 DRI 2": (108, 2, 1)}
    with capsys.disabled():
        for c in J.design("restart_many") + J.design("periodic"):
            segs = c.stats["scans"][0]["segments"]
            n64, n1024 = J.nchunks_of(c, 64), J.nchunks_of(c, 1024)
            print(f"\n{c.name}: {len(segs)} segments, {8 * sum(segs)} clean bits, "
                  f"{n64} chunks at 64 bits, {n1024} at 1024", end="")
            if c.name in want:
                nseg, m64, m1024 = want[c.name]
                assert len(segs) == nseg and -(-len(segs) // 1024) >= min(m64, m1024)
                assert -(-n64 // 1024) == m64 and -(-n1024 // 1024) == m1024, (c, n64, n1024)
            elif "352x352" in c.name:
                assert 8 * sum(segs) > 1024 * 64
    heavy = J.design("restart_many")[3].stats["scans"][0]["segments"]
    assert min(heavy) * 8 > 3 * 64                              # every segment several chunks


def test_restart_design_wraps_rst_numbers_and_has_short_last_intervals():
    cases = J.design("restart")
    assert sum(len(c.stats["scans"][0]["segments"]) >= 9 for c in cases) >= 5
    assert any(b"\xff\xff\xff\xff\xd7" in c.data for c in cases)          # 3 fill bytes
    assert any(len(c.stats["scans"][0]["segments"]) == 1 for c in cases)  # DRI beyond the image


# ------------------------------------------------------------------ sensitivity
def _sens_families():
    """(name, coefs, height, width, writer options) per design family.  Families whose
    tables are all ones are written here with tables of 8s where the rule allows; the
    others move the coefficient by 8 units, the same dequantized step."""
    ones = {0: np.ones(64, np.int64)}
    yield "symbols", [J.symbol_blocks()], 64, 64, dict(qtables=ones), 8
    r = J.design("range")
    yield "range 8-bit", r[0].coefs, 32, 32, dict(qtables={0: J.Q8}), 1
    yield "range 16-bit", r[1].coefs, 32, 32, dict(qtables={0: r[1].qtabs[0]}, sof=1,
                                                   huffman="optimal"), 1
    yield "periodic", [J.periodic_blocks(44, 44, 3)], 352, 352, dict(qtables={0: J.Q8}), 1
    rs = J.design("restart")[14]
    yield "restart", rs.coefs, 40, 72, dict(sampling=J.SAMPLINGS["420"], restart=3, fill=1,
                                            qtables=ones), 8
    pc = J.prog_coefs("420", 48, 56)
    sa = J.prog_scripts(3)["successive approximation 3..0"][0]
    yield "progressive", pc, 48, 56, dict(sampling=J.SAMPLINGS["420"], qtables={0: J.Q8}, sof=2,
                                          script=sa), 1
    e = J.design("eobrun")[0]
    yield "eobrun", e.coefs, 384, 384, dict(qtables={0: J.Q8}, sof=2, script=[
        ((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]), 1
    yield "colour", J.colour_coefs("420"), 16, 16, dict(sampling=J.SAMPLINGS["420"],
                                                        qtables=ones), 8
    h = J.design("headers")[2]
    yield "headers", h.coefs, 24, 40, dict(sampling=J.SAMPLINGS["420"], tq=[3, 0, 2],
                                           qtables={3: h.qtabs[0], 0: h.qtabs[1], 2: h.qtabs[2]}), 1


SENS_FAMILIES = ["symbols", "range 8-bit", "range 16-bit", "periodic", "restart", "progressive",
                 "eobrun", "colour", "headers"]


@pytest.mark.parametrize("family", SENS_FAMILIES)
def test_one_quantum_changes_the_pixels(family):
    """One coefficient moved by one quantum of a table entry >= 8 (8 units under a table of
    ones) changes Pillow's pixels: in the first block and in the last, at a low and at a
    high frequency, in every component."""
    fams = {f[0]: f for f in _sens_families()}
    assert list(fams) == SENS_FAMILIES
    name, coefs, h, w, kw, step = fams[family]
    ref = _pixels(J.write_jpeg(coefs, h, w, **kw))
    for comp in range(len(coefs)):
        last = (coefs[comp].shape[0] - 1, coefs[comp].shape[1] - 1)
        # the range design's first blocks are clamped flat: take two that are not
        for by, bx in ((1, 1), last) if name.startswith("range") else ((0, 0), last):
            for k in (0, 1, 27):
                moved = [a.copy() for a in coefs]
                v = moved[comp][by, bx, k]
                moved[comp][by, bx, k] = v - step if v > 0 else v + step
                got = _pixels(J.write_jpeg(moved, h, w, **kw))
                assert not np.array_equal(got, ref), (name, comp, by, bx, k)


def test_one_refinement_bit_changes_the_pixels():
    """The lowest bit of a coefficient of magnitude >= 2 travels as a correction bit of the
    last refinement scan (AC) or as the DC refinement bit: flipping it changes the pixels."""
    coefs = J.prog_coefs("420", 48, 56)
    kw = dict(sampling=J.SAMPLINGS["420"], qtables={0: J.Q8}, sof=2,
              script=J.prog_scripts(3)["successive approximation 3..0"][0])
    ref = _pixels(J.write_jpeg(coefs, 48, 56, **kw))
    for comp in range(3):
        a = coefs[comp]
        for k in (0, 2, 30):
            by, bx = np.argwhere(np.abs(a[..., k]) >= 2)[-1]
            moved = [x.copy() for x in coefs]
            v = int(a[by, bx, k])
            moved[comp][by, bx, k] = (abs(v) ^ 1) * (1 if v > 0 else -1)
            got = _pixels(J.write_jpeg(moved, 48, 56, **kw))
            assert not np.array_equal(got, ref), (comp, k)


# ------------------------------------------------------------------ host entry points
def _info(L, f):
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = L.lib.vtd_jpeg_info(f, len(f), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c))
    return rc, (h.value, w.value, c.value)


def _plan(L, files):
    n = len(files)
    ptrs = (ctypes.c_char_p * n)(*files)
    lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
    dims = np.zeros((n, 2), np.int32)
    ws = ctypes.c_size_t()
    rc = L.lib.vtd_jpeg_workspace_bytes(ptrs, lens, n, dims.ctypes.data, ctypes.byref(ws))
    return rc, dims, ws.value


@pytest.mark.parametrize("name", list(J.DESIGNS))
def test_host_entry_points_accept_every_design(L, name):
    cases = J.design(name)
    for c in cases:
        rc, dims = _info(L, c.data)
        assert rc == 0, (c, L.lib.vtd_last_error())
        assert dims == c.size + (len(c.coefs),), c
    rc, dims, ws = _plan(L, [c.data for c in cases])
    assert rc == 0 and ws > 0, L.lib.vtd_last_error()
    assert [tuple(d) for d in dims] == [c.size for c in cases]


def test_documented_refusals_name_their_reason(L):
    rng = np.random.default_rng(1)

    def refused(data, word):
        rc, _ = _info(L, data)
        assert rc != 0 and word in L.lib.vtd_last_error(), L.lib.vtd_last_error()

    coefs = [J.noisy_coefs(rng, 2, 2) for _ in range(3)]
    # sequential, one scan per component: libjpeg decodes it, the device does not
    multi = J.write_jpeg(coefs, 16, 16, script=[((c,), 0, 63, 0, 0) for c in range(3)])
    assert _pil(multi).size == (16, 16)
    refused(multi, b"single-scan")
    samp = [(1, 2), (1, 1), (1, 1)]
    coefs = [J.noisy_coefs(rng, *g) for g in J.grids(32, 32, samp)]
    refused(J.write_jpeg(coefs, 32, 32, sampling=samp), b"4:4:0")
    samp = [(3, 1), (1, 1), (1, 1)]
    coefs = [J.noisy_coefs(rng, *g) for g in J.grids(16, 48, samp)]
    three = J.write_jpeg(coefs, 16, 48, sampling=samp)
    assert _pil(three).size == (48, 16)
    refused(three, b"sampling factors")
    # a DQT with other values between the scans of a progressive file
    coefs = J.prog_coefs("420", 48, 56)
    f = J.write_jpeg(coefs, 48, 56, sof=2, sampling=J.SAMPLINGS["420"], qtables={0: J.Q8},
                     script=J.prog_scripts(3)["narrow bands"][0])
    second = f.index(b"\xff\xda", f.index(b"\xff\xda") + 2)
    dqt = lambda v: b"\xff\xdb\x00\x43\x00" + bytes([v] * 64)     # noqa: E731
    rc, dims = _info(L, f[:second] + dqt(8) + f[second:])
    assert rc == 0 and dims == (48, 56, 3), L.lib.vtd_last_error()
    refused(f[:second] + dqt(9) + f[second:], b"latched")
