"""Device JPEG decode (vtd_jpeg_decode) on hand-built streams: what Pillow's encoder never
writes.  tests/jpeg_streams.py writes each file from quantized coefficients; every design is
decoded in one ragged batch through preprocess.decode_jpegs and every pixel compared with
Pillow's (libjpeg-turbo's) decode of the same bytes.  The sequential designs run at the
default entropy-decode chunk and at 64 bits, where nearly every chunk starts at a guessed
state.  The premises (the files load under Pillow, the designs reach what they are built for,
libjpeg's two IDCT forms agree on them) are checked on the host in
tests/test_jpeg_streams_host.py.

Fixed with these tests: the colour space of a 3-component file.  parse_jpeg looked at the
Adobe marker only; libjpeg (jdapimin.c default_decompress_parms) lets a JFIF marker win over
it and falls back to the component ids, so a file with ids 'R' 'G' 'B' and no marker was
converted from YCbCr although it is RGB, and a JFIF file with an Adobe transform 0 was left
unconverted although it is YCbCr."""
import io
import math

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_streams as J
from tests.test_gpu_jpeg import _tf_cmyk_rgb

pytestmark = pytest.mark.gpu

CHUNKS = [None, 64]


def _expected(data, mode):
    if mode == "CMYK":
        return _tf_cmyk_rgb(data)
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _mismatches(cuda, named_files, chunk_bits=None):
    """Decodes [(name, bytes, mode)] in one batch; the failure messages of the files whose
    pixels differ from the expectation."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd.preprocess import decode_jpegs
    files = [f for _, f, _ in named_files]
    with L.knob(L.KNOB_JPEG_CHUNK_BITS, int(chunk_bits) if chunk_bits else -1):
        pixels, offsets, sizes = decode_jpegs(files, device=cuda)
        torch.cuda.synchronize()
    got = pixels.cpu().numpy()
    out = []
    for i, (name, f, mode) in enumerate(named_files):
        ref = _expected(f, mode)
        h, w = sizes[i]
        assert (h, w) == ref.shape[:2], name
        mine = got[offsets[i]:offsets[i] + h * w * 3].reshape(h, w, 3)
        bad = np.argwhere(mine != ref)
        if bad.size:
            out.append(f"{name}: {len(bad)} differing values, first at {bad[0].tolist()}: "
                       f"{mine[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    return out


def _check(cuda, design, chunk_bits=None):
    cases = J.design(design)
    bad = _mismatches(cuda, [(c.name, c.data, c.mode) for c in cases], chunk_bits)
    assert not bad, f"{len(bad)} of {len(cases)} files differ:\n" + "\n".join(bad)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_symbols_and_code_lengths(cuda, chunk_bits):
    """Gray 64 x 64 and the same blocks as the Y plane of a 4:2:0 image: every DC size
    0..11, every AC run/size 0/1..15/10, one to three ZRL in a row, EOB, blocks ending at
    k = 63 without EOB; written with the Annex K tables, optimal tables and dictated tables
    under table ids 2 and 3.  The dictated luma tables give the symbols that occur 12 DC
    code lengths from 2 to 16 and every AC length 2..16 (162 symbols leave no room for a
    1-bit code); the chroma tables of the 4:2:0 file add the lengths missing, so that every
    length 1..16 decodes a real symbol in DC and in AC, through the 9-bit lookahead and
    through the maxcode walk."""
    _check(cuda, "symbols", chunk_bits)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_range_limit_and_wide_tables(cuda, chunk_bits):
    """Centred samples from -500 to +500, both clamp regions of the range-limit table, with
    an 8-bit table and as SOF1 with a 16-bit table (entries up to 1000)."""
    _check(cuda, "range", chunk_bits)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_periodic_streams(cuda, chunk_bits):
    """Identical blocks (period 1, 2, 3), a flat image and periodic 4:2:0 MCUs: a chunk that
    starts at a wrong guess never resynchronises by itself."""
    _check(cuda, "periodic", chunk_bits)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_restart_intervals(cuda, chunk_bits):
    """DRI of 1, 2, 3, 7, one less and one more than the MCU row, and more than the image,
    in 4:4:4, 4:2:2, 4:2:0, gray and CMYK, with fill bytes before the markers."""
    _check(cuda, "restart", chunk_bits)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_more_restart_segments_than_threads(cuda, chunk_bits, capsys):
    """Every thread of the entropy decoder takes a run of chunks: ceil(chunks / 1024) is 2
    and 3 (a file has at least as many chunks as restart segments), and 2 for the heavy
    file at 64-bit chunks, where runs mix segment starts with segments of several chunks.
    Sizes used: gray 264 x 264 and 368 x 368, 4:2:0 528 x 528, gray 96 x 144."""
    cases = J.design("restart_many")
    with capsys.disabled():
        for c in cases:
            segs = c.stats["scans"][0]["segments"]
            print(f"\n{c.name}: {len(segs)} segments, {8 * sum(segs)} clean bits, "
                  f"{J.nchunks_of(c, chunk_bits or 1024)} chunks", end="")
    per_thread = [math.ceil(len(c.stats["scans"][0]["segments"]) / 1024) for c in cases[:3]]
    assert per_thread == [2, 3, 2]
    if chunk_bits == 64:
        assert math.ceil(J.nchunks_of(cases[3], 64) / 1024) == 2
    _check(cuda, "restart_many", chunk_bits)


def test_progressive_scripts(cuda):
    """One coefficient set (48 x 56 in 4:2:0, 4:4:4 and gray, 17 x 17 in 4:2:0) under seven
    scan scripts: one AC scan per component, narrow bands, successive approximation from
    Al 3 for DC and AC (three refinements over many nonzero coefficients, ZRL inside them),
    a partly interleaved DC, chroma before luma, tables re-sent before every scan, DRI
    changed between scans."""
    _check(cuda, "progressive")


def test_progressive_eobrun_categories(cuda):
    """Gray 384 x 384: EOBRUNs of every length category 0..11 in first scans and in
    refinement scans (category 14 would need 16384 consecutive empty blocks)."""
    _check(cuda, "eobrun")


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_colour_space_follows_libjpeg(cuda, chunk_bits):
    """JFIF, then the Adobe transform, then the component ids decide the colour space of a
    3-component file; 4-component files as TF converts them."""
    _check(cuda, "colour", chunk_bits)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_headers(cuda, chunk_bits):
    """Gray with sampling factors 2 x 2 / 2 x 1 in SOF, quantization tables 3, 0, 2, Huffman
    table ids 0..3, one or all tables per segment, tables after SOF, COM / APPn segments
    between all others, arbitrary component ids."""
    _check(cuda, "headers", chunk_bits)


SMALL = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("chunk_bits", CHUNKS)
def test_small_sizes_pillow_encoded(cuda, chunk_bits):
    """Every height and width in SMALL as gray, 4:4:4, 4:2:2 and 4:2:0 (576 baseline files,
    one batch): the edges of the upsampling, the context rows and the row-segment stores at
    every alignment."""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (33, 33, 3), dtype=np.uint8)
    base[::5] //= 3                                         # some structure besides noise
    files = []
    for h in SMALL:
        for w in SMALL:
            for mode, sub in (("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2)):
                b = io.BytesIO()
                kw = {} if sub is None else dict(subsampling=sub)
                Image.fromarray(base[:h, :w]).convert(mode).save(b, format="JPEG", quality=90, **kw)
                files.append((f"{h}x{w} {mode} subsampling {sub}", b.getvalue(), mode))
    assert len(files) == 576
    bad = _mismatches(cuda, files, chunk_bits)
    assert not bad, f"{len(bad)} of {len(files)} files differ:\n" + "\n".join(bad[:20])
