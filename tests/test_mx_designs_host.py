"""tests/mx_designs.py on the CPU: the byte codec, the classes each design reaches, and the power
of the designs to notice a wrong quantizer -- every named fault of mx_designs.emulate changes at
least one byte or scale byte of the memory tests/test_gpu_mx8_designed.py compares.

Why the designs are needed: tests/test_gpu_mx8.py quantizes randn x 2^[-20, 20] rows.  Inside a
Gaussian block no value lies 2^14 below the maximum, so no element reaches the e4m3 subnormal
range, the 2^-10 tie or an underflow, no block maximum sits on the m > 0.875 boundary, and a
maximum taken over 31 of the 32 positions is wrong in one block of 32 only
(test_gaussian_blocks_miss_the_classes counts them on that test's own data).
"""
import numpy as np
import pytest

from oracle import mx8 as MX
from tests import mx_designs as D

# (K, Kq) of the standalone quantizer's GPU cases: K == Kq; K ending inside a block at a multiple
# of 8; K % 8 != 0 (bf16: the ragged branch; f32: mid-block); whole blocks of padding
QUANT_SHAPES = ((256, 256), (232, 256), (203, 256), (96, 256), (100, 128))


@pytest.fixture(scope="module")
def designs():
    return {"bf16": D.design_matrix(D.bf16_blocks()), "f32": D.design_matrix(D.f32_blocks())}


# ------------------------------------------------------------------ the codec
def test_e4m3_codec_known_answers():
    codes = np.arange(256, dtype=np.uint8)
    finite = codes[(codes & 0x7F) != 0x7F]
    assert len(finite) == 254
    v = MX.decode_e4m3(finite)
    assert np.array_equal(MX.encode_e4m3(v), finite)              # -0 keeps its sign bit
    assert np.array_equal(MX.encode_e4m3(MX.round_e4m3(v)), finite)
    assert np.isnan(MX.decode_e4m3([0x7F, 0xFF])).all()
    # a few values by hand: 2^-9, 2^-6, 1, 1.125, 448
    assert MX.decode_e4m3([0x01, 0x08, 0x38, 0x39, 0x7E, 0x80 | 0x38]).tolist() == \
        [2.0 ** -9, 2.0 ** -6, 1.0, 1.125, 448.0, -1.0]
    # the 126 midpoints between adjacent magnitudes go to the even code, with either sign
    mag = MX.decode_e4m3(np.arange(127, dtype=np.uint8))
    mid = (mag[:-1] + mag[1:]) / 2
    assert len(mid) == 126
    even = np.arange(126) + (np.arange(126) % 2)
    assert np.array_equal(MX.encode_e4m3(MX.round_e4m3(mid)), even.astype(np.uint8))
    assert np.array_equal(MX.encode_e4m3(MX.round_e4m3(-mid)), (even | 0x80).astype(np.uint8))
    # one float64 ulp either side of a midpoint goes to the nearer code
    assert np.array_equal(MX.encode_e4m3(MX.round_e4m3(np.nextafter(mid, 0))), np.arange(126))
    assert np.array_equal(MX.encode_e4m3(MX.round_e4m3(np.nextafter(mid, 1e9))),
                          np.arange(1, 127))
    assert MX.encode_e4m3(MX.round_e4m3(np.array([-2.0 ** -11, -0.0, 2.0 ** -11]))).tolist() == \
        [0x80, 0x80, 0x00]
    with pytest.raises(AssertionError, match="not an e4m3 value"):
        MX.encode_e4m3(np.array([1.0625]))


def test_block_exponent_known_answers():
    amax = [0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -118, 2.0 ** -117, 448.0,
            np.nextafter(np.float32(448), np.float32(1e9)), 450.0, 1.0, 2.0 ** 126,
            float(np.finfo(np.float32).max)]
    want = [-126, -126, -126, -126, -126, -125, 0, 1, 1, -8, 118, 120]
    assert MX.block_exponent(np.array(amax, np.float64)).tolist() == want


# ------------------------------------------------------------------ the designs
def test_designs_reach_every_class(designs):
    b, f = designs["bf16"], designs["f32"]
    assert 256 <= len(b) <= 1100 and b.shape[1] == 256 and f.shape[1] == 256
    assert np.array_equal(D.to_bf16(b), b), "a value of the bf16 design is not a bf16 number"
    assert not np.array_equal(D.to_bf16(f), f)
    cb, cf = D.coverage(b), D.coverage(f)
    print("bf16:", D.summary(cb))
    print("f32: ", D.summary(cf))
    D.assert_coverage(cb, ["a", "b_bf16", "c", "d", "e", "f"], "bf16 design")
    D.assert_coverage(cf, ["a", "b_f32", "c", "d", "e"], "f32 design")
    assert 0x80 in cb["bytes"] and 0x00 in cb["bytes"]
    # the counts hold in every K the GPU cases cut the matrix at, except what the cut removes
    for K, Kq in QUANT_SHAPES:
        c = D.coverage(b[:, :K], Kq)
        D.assert_coverage(c, ["a", "b_bf16", "c", "d", "e"], f"bf16 design K {K}")
        if K < Kq - 32:
            assert c["zero_block"] >= len(b)


@pytest.mark.parametrize("heads,dkp", [(4, 32), (2, 64), (1, 128), (2, 128)])
def test_attention_design(heads, dkp):
    v = D.attention_values(heads, dkp)
    assert np.array_equal(D.to_bf16(v), v)
    D.assert_coverage(D.coverage(v), ["a", "b_bf16", "d", "e", "zero"], "attention values")
    # 10 keys of one class (N = 290): the fp32 sum of 10 equal values and its product with
    # fl(1 / 10) round back to the value
    s = (v.astype(np.float64) * 10).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), v.astype(np.float64) * 10)
    assert np.array_equal(D.to_bf16(s * np.float32(1 / np.float32(10))), v)
    body, want = D.attention_qkv(2, 33, heads, dkp, 3 * heads * dkp + 8)
    assert np.array_equal(want[32], want[0]) and np.array_equal(want[33], want[0])
    assert (body[:, 3 * heads * dkp:] == 0x7FC0).all()
    q = D.bf16_value(body[:, :heads * dkp]).reshape(66, heads, dkp)
    assert (q[40].argmax(axis=1) == 7).all() and q[40].sum() == 16 * heads


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("N", [256, 512])
def test_gemm_design(N, act):
    g = D.gemm_design(N, act)
    assert g["bt"].shape == (N, 128) and g["sb"].shape == (N, 4) and g["bias"].shape == (N,)
    assert ((g["bt"] & 0x7F) != 0x7F).all()
    # z is what the operands decode to
    bt = MX.decode_e4m3(g["bt"]).reshape(N, 4, 32) * np.exp2(g["sb"].astype(np.float64) - 127)[..., None]
    z = (bt.reshape(N, 128).T + g["bias"].astype(np.float64)[None, :]).astype(np.float32)
    assert np.array_equal(z.astype(np.float64), g["z"])
    out = D.to_bf16(D.act64(g["z"], act))
    c = D.coverage(out)
    print(f"act {act} N {N}:", D.summary(c))
    D.assert_coverage(c, ["a", "d", "e"] + (["b_bf16"] if act == 0 else []), "GEMM design")


# ------------------------------------------------------------------ the faults
@pytest.mark.parametrize("src", ["bf16", "f32"])
def test_emulation_without_a_fault_is_the_oracle(designs, src):
    x = designs[src]
    for K, Kq in QUANT_SHAPES:
        q, s = D.emulate(x[:, :K], Kq, s_rows=len(x) + 8)
        wq, ws, mask = D.expected_memory(x[:, :K], Kq, len(x) + 8)
        assert np.array_equal(q, wq) and np.array_equal(s, ws)
        assert (s[~mask] == D.PATTERN).all()
        if K < Kq:
            assert (q[:, K:] == 0).all()
            plane = s.reshape(Kq // 128, len(x) + 8, 4)[:, :len(x)].transpose(1, 0, 2)
            assert (plane.reshape(len(x), -1)[:, -(-K // 32):] == 1).all()


@pytest.mark.parametrize("fault", D.FAULTS, ids=lambda f: f if isinstance(f, str) else f"{f[0]}_{f[1]}")
def test_every_fault_changes_the_memory(designs, fault):
    """Each design sees each fault, in the ragged case (K = 203 in Kq = 256) and, but for the
    unwritten pad, at K == Kq."""
    for src, x in designs.items():
        for K, Kq in ((203, 256), (256, 256)):
            if fault == "pad_unwritten" and K == Kq:
                continue
            q0, s0 = D.emulate(x[:, :K], Kq, s_rows=len(x) + 8)
            q1, s1 = D.emulate(x[:, :K], Kq, fault, s_rows=len(x) + 8)
            diff = int((q0 != q1).sum()) + int((s0 != s1).sum())
            assert diff > 0, f"the {src} design at K {K} does not see {fault}"


def test_gaussian_blocks_miss_the_classes():
    """The data of test_gpu_mx8.test_quantize_matches_oracle (rows x 2^[-20, 20], one zero row)
    reach none of the element classes and see neither rounding fault nor a flushed subnormal."""
    rng = np.random.default_rng(0)
    rows, K = 129, 768
    x = rng.standard_normal((rows, K)) * np.exp2(np.linspace(-20, 20, rows))[:, None]
    x[rows // 2] = 0
    x = x.astype(np.float32)
    c = D.coverage(x, K)
    print(D.summary(c))
    for name in ("at_448", "above_448_f32", "amax_tiny", "amax_f32_subnormal", "amax_huge",
                 "tie10_pos", "tie10_neg", "tie_up_sub", "tie_down_sub"):
        assert c[name] == 0, name
    q0, s0 = D.emulate(x, K)
    for fault in ("ge_boundary", "no_clamp", "flush_f32_subnormals", "half_up"):
        q1, s1 = D.emulate(x, K, fault)
        assert np.array_equal(q0, q1) and np.array_equal(s0, s1), fault
