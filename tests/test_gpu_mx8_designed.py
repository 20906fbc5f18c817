"""The MX-fp8 producers on designed blocks, byte for byte, every kernel instantiation, every
device output inside 0xA5 guard bands (tests/mx_designs.py has the blocks and their classes,
tests/test_mx_designs_host.py shows on the CPU that each design notices each named fault).

  vtd_quantize_mx8     against the bytes and scale bytes of oracle/mx8.py;
  vtd_attention_mx8    against oracle/mx8.py applied on the host to the bf16 output vtd_attention
                       wrote on the device, and against vtd_quantize_mx8 of that output;
  vtd_gemm_mx8         out_dtype VTD_FP8 against oracle/mx8.py applied on the host to the bf16
                       output of the same GEMM.
No tolerance anywhere.  The only other conditions are the coverage counts: the fused producers'
inputs are built so that designed blocks arrive at the epilogue, and `coverage` of the bf16 output
the device actually wrote must still reach the classes -- a construction that drifts fails instead
of testing nothing.  (vtd_layernorm_mx8: tests/test_gpu_layernorm_designed.py.)

Guards: in front of and behind each buffer (at least 64 KiB), the columns [Kq, ldq) of the byte
outputs and the scale rows [rows, s_rows) of every K-step plane hold 0xA5 and must come back
unchanged; every leading dimension exceeds its width; input pad columns hold NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import mx_designs as D
from tests.test_gpu_gemm_designed import PATTERN, col_mask, in_buf, knobs, out_buf

pytestmark = pytest.mark.gpu

QUANT_SHAPES = ((256, 256), (232, 256), (203, 256), (96, 256), (100, 128))
ATT_HEADS = {32: (4,), 64: (2,), 128: (1, 2)}        # heads dkp % 128 == 0; 2 x 128: two K-steps
ATT_N = (33, 128, 129, 290)                          # <= 128: 4 waves; 290: a ragged last block
ATT_CASES = [(dkp, h, N) for dkp, hs in ATT_HEADS.items() for h in hs for N in ATT_N
             if h == hs[0] or N in (128, 290)]       # two K-steps: one 4-wave, one 8-wave case
GEMM_SHAPES = ((256, 256, 128), (256, 512, 128))     # the second fills scale planes 0 .. 3

# kernel instantiation -> the case that reaches it
INSTANTIATIONS = {
    "quantize_mx8_kernel<bf16_t>": "test_quantize[bf16-*]; the ragged branch (K % 8 != 0): K = 203",
    "quantize_mx8_kernel<float>": "test_quantize[f32-*]; K ending inside a block: 232, 203, 100",
    "attention_bf16_kernel<32, 4, MX8>": "test_attention[32-4-33], [32-4-128]",
    "attention_bf16_kernel<32, 8, MX8>": "test_attention[32-4-129], [32-4-290]",
    "attention_bf16_kernel<64, 4, MX8>": "test_attention[64-2-33], [64-2-128]",
    "attention_bf16_kernel<64, 8, MX8>": "test_attention[64-2-129], [64-2-290]",
    "attention_bf16_kernel<128, 4, MX8>": "test_attention[128-1-33], [128-2-128]",
    "attention_bf16_kernel<128, 8, MX8>": "test_attention[128-1-129], [128-2-290]",
    "gemm_mx8_pp_kernel<4 | EPI_F8O>": "test_gemm_fp8_output[1-none-tr0] and [1-none-tr1]: no "
                                       "transposed kernel has this code (VTD_MX_TR_CODES)",
    "gemm_mx8_pp_kernel<5 | EPI_F8O>": "test_gemm_fp8_output[1-gelu-tr0]",
    "gemm_mx8_pp_kernel<6 | EPI_F8O>": "test_gemm_fp8_output[1-mish-tr0]",
    "gemm_mx8_pp_kernel<5 | EPI_F8O, true>": "test_gemm_fp8_output[1-gelu-tr1]",
    "gemm_mx8_pp_kernel<6 | EPI_F8O, true>": "test_gemm_fp8_output[1-mish-tr1]",
    "gemm_mx8_x4 (diagnostic library)": "test_gemm_fp8_output[2-*]: VTD_MX_VARIANT = 2, skipped "
                                        "where vtd_diag_build is absent",
}


def attention_route(dkp, N):
    """attention_mx8_launch restated: N <= 128 picks the 4-wave workgroup, else 8 waves."""
    return f"attention_bf16_kernel<{dkp}, {4 if N <= 128 else 8}, MX8>"


def gemm_route(act, tr, variant):
    """gemm_mx8_launch restated for a fast MX-fp8 output: code (4 + act) | EPI_F8O; the transposed
    kernel under KNOB_GEMM_TR = 1 where VTD_MX_TR_CODES has the code (GELU, Mish)."""
    if variant == "2":
        return "gemm_mx8_x4 (diagnostic library)"
    code = f"{4 + act} | EPI_F8O"
    return f"gemm_mx8_pp_kernel<{code}, true>" if tr == 1 and act != 0 else f"gemm_mx8_pp_kernel<{code}>"


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def designs():
    return {"bf16": D.design_matrix(D.bf16_blocks()), "f32": D.design_matrix(D.f32_blocks())}


def test_every_instantiation_has_a_case():
    reached = {attention_route(dkp, N) for dkp, _, N in ATT_CASES}
    reached |= {gemm_route(a, tr, v) for a in (0, 1, 2) for tr in (0, 1) for v in ("1", "2")}
    reached |= {"quantize_mx8_kernel<bf16_t>", "quantize_mx8_kernel<float>"}
    assert reached == set(INSTANTIATIONS)
    assert any(K % 8 for K, _ in QUANT_SHAPES) and any(K % 32 and K % 8 == 0 for K, _ in QUANT_SHAPES)
    assert any(K == Kq for K, Kq in QUANT_SHAPES) and any(Kq - K >= 64 for K, Kq in QUANT_SHAPES)


# ------------------------------------------------------------------ guarded byte buffers
def assert_bytes(buf, want, what):
    """The bytes the contract writes equal `want`; everything else (guards included) is unchanged.
    A mismatch lists the commonest (got, want) pairs."""
    got = buf.read()                                   # asserts the guards
    m = buf.mask
    assert m.any()
    if not np.array_equal(got[m], want[m]):
        bad = m & (got != want)
        pairs, counts = np.unique(np.stack([got[bad], want[bad]], axis=1), axis=0, return_counts=True)
        top = [f"got {g:#04x} want {w:#04x} x {c}" for (g, w), c in
               sorted(zip(pairs.tolist(), counts.tolist()), key=lambda t: -t[1])[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(m.sum())} bytes differ, first at "
                             f"{np.argwhere(bad)[:4].tolist()}: " + "; ".join(top))
    assert np.array_equal(got[~m], buf.initial()[~m]), \
        f"{what}: a byte the contract does not write was touched"


def mx_outputs(dev, rows, Kq, s_rows):
    """(q, s): e4m3 bytes [rows][Kq + 16] and scales [Kq / 128][4 s_rows], 0xA5 where unwritten."""
    assert s_rows >= rows + 8
    q = out_buf(dev, rows, Kq + 16, np.uint8, col_mask(rows, Kq + 16, (0, Kq)))
    smask = np.zeros((Kq // 128, s_rows, 4), bool)
    smask[:, :rows] = True
    s = out_buf(dev, Kq // 128, 4 * s_rows, np.uint8, smask.reshape(Kq // 128, 4 * s_rows))
    return q, s


def check_mx(q, s, values, Kq, s_rows, what):
    """q, s against oracle/mx8.py of `values` [rows][K] (columns [K, Kq) zero)."""
    wq, ws, mask = D.expected_memory(values, Kq, s_rows)
    assert np.array_equal(mask, s.mask)
    want = np.full(q.shape, PATTERN, np.uint8)
    want[:, :Kq] = wq
    assert_bytes(s, ws, what + " scale bytes")
    assert_bytes(q, want, what + " e4m3 bytes")


def quantize(L, x_ptr, dtype, rows, K, ldx, Kq, q, s, s_rows):
    L.check(L.lib.vtd_quantize_mx8(x_ptr, dtype, rows, K, ldx, Kq, q.ptr, q.shape[1], s.ptr,
                                   s_rows, L.stream_ptr()), "quantize_mx8")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. the standalone quantizer
@pytest.mark.parametrize("K,Kq", QUANT_SHAPES)
@pytest.mark.parametrize("src", ["bf16", "f32"])
def test_quantize(L, cuda, designs, src, K, Kq):
    x = designs[src][:, :K]
    rows, s_rows = len(x), len(x) + 8
    if src == "bf16":
        ldx = -(-K // 8) * 8 + 8                       # ldx % 8 == 0
        xin = in_buf(cuda, D.bf16_bits(x), ldx)
    else:
        ldx = K + 3
        xin = in_buf(cuda, x, ldx)
    q, s = mx_outputs(cuda, rows, Kq, s_rows)
    quantize(L, xin.ptr, L.BF16 if src == "bf16" else L.F32, rows, K, ldx, Kq, q, s, s_rows)
    check_mx(q, s, x, Kq, s_rows, f"quantize {src} K {K} Kq {Kq}")
    # the pad columns are zero bytes, the blocks wholly inside them have scale byte 1
    got_q = q.read()
    assert (got_q[:, K:Kq] == 0).all()
    planes = s.read().reshape(Kq // 128, s_rows, 4)[:, :rows].transpose(1, 0, 2).reshape(rows, -1)
    assert (planes[:, -(-K // 32):] == 1).all()
    assert np.array_equal(xin.read().view(np.uint8), xin.initial().view(np.uint8))


# ------------------------------------------------------------------ 2. attention
@pytest.mark.parametrize("dkp,heads,N", ATT_CASES)
def test_attention(L, cuda, dkp, heads, N):
    assert attention_route(dkp, N) in INSTANTIATIONS
    B, inner = 2, heads * dkp
    rows, s_rows = B * N, B * N + 8
    ld, ldo = 3 * inner + 8, inner + 8
    body, ideal = D.attention_qkv(B, N, heads, dkp, ld)
    qkv = in_buf(cuda, body, ld)
    o16 = out_buf(cuda, rows, ldo, np.uint16, col_mask(rows, ldo, (0, inner)))
    with knobs(L, ATTN_VARIANT=2):                     # the streaming kernel, as the MX epilogue
        L.check(L.lib.vtd_attention(qkv.ptr, B, N, heads, dkp, ld, 1.0, o16.ptr, ldo, L.BF16,
                                    L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    bits = o16.read()
    assert np.array_equal(bits[:, inner:], o16.initial()[:, inner:])
    vals = D.bf16_value(bits[:, :inner])
    assert np.isfinite(vals).all()
    what = f"attention dkp {dkp} heads {heads} N {N}"
    drift = int((vals != ideal).sum())
    cov = D.coverage(vals, inner)
    print(f"{what}: {drift} outputs differ from the designed values; {D.summary(cov)}")
    D.assert_coverage(cov, ["a", "b_bf16", "d", "e", "zero"], what)

    q, s = mx_outputs(cuda, rows, inner, s_rows)
    L.check(L.lib.vtd_attention_mx8(qkv.ptr, B, N, heads, dkp, ld, 1.0, q.ptr, q.shape[1], s.ptr,
                                    s_rows, L.stream_ptr()), "attention_mx8")
    torch.cuda.synchronize()
    check_mx(q, s, vals, inner, s_rows, what + " fused")
    q2, s2 = mx_outputs(cuda, rows, inner, s_rows)
    quantize(L, o16.ptr, L.BF16, rows, inner, ldo, inner, q2, s2, s_rows)
    check_mx(q2, s2, vals, inner, s_rows, what + " vtd_quantize_mx8 of the bf16 output")
    assert np.array_equal(qkv.read(), qkv.initial())


# ------------------------------------------------------------------ 3. the GEMM epilogues
ACTS = {"none": 0, "gelu": 1, "mish": 2}


def _need_variant(L, variant):
    """VTD_MX_VARIANT 2 (the x4 kernel) exists in the diagnostic library only."""
    if variant != "1" and not hasattr(L.lib, "vtd_diag_build"):
        pytest.skip("the x4 kernel is in the diagnostic build only (make diag)")


@pytest.mark.parametrize("tr", [0, 1], ids=["tr0", "tr1"])
@pytest.mark.parametrize("act_name", list(ACTS))
@pytest.mark.parametrize("variant", ["1", "2"])
def test_gemm_fp8_output(L, cuda, monkeypatch, variant, act_name, tr):
    _need_variant(L, variant)
    monkeypatch.setenv("VTD_MX_VARIANT", variant)
    act = ACTS[act_name]
    assert gemm_route(act, tr, variant) in INSTANTIATIONS
    for M, N, K in GEMM_SHAPES:
        g = D.gemm_design(N, act)
        sa_rows, sb_rows, so_rows = M + 4, N + 8, M + 8
        a = np.zeros((M, K), np.uint8)
        a[np.arange(M), np.arange(M) % K] = 0x38       # e4m3 1.0
        A = in_buf(cuda, a, K + 16)
        Bt = in_buf(cuda, g["bt"], K + 16)
        sA = in_buf(cuda, np.full(sa_rows * 4, 127, np.uint8), sa_rows * 4, nan=0xFF)
        sb = np.full((sb_rows, 4), 127, np.uint8)      # rows past N: readable, 2^0
        sb[:N] = g["sb"]
        sB = in_buf(cuda, sb.reshape(-1), sb_rows * 4, nan=0xFF)
        bias = in_buf(cuda, g["bias"], N + 4)
        what = f"mx8 {M}x{N}x{K} variant {variant} {act_name} tr {tr}"

        def run(ep):
            with knobs(L, GEMM_TR=tr):
                L.check(L.lib.vtd_gemm_mx8(M, N, K, A.ptr, K + 16, sA.ptr, sa_rows, Bt.ptr, K + 16,
                                           sB.ptr, sb_rows, ctypes.byref(ep), L.stream_ptr()), what)
            torch.cuda.synchronize()

        o16 = out_buf(cuda, M, N + 8, np.uint16, col_mask(M, N + 8, (0, N)))
        ep = L.VtdEpilogue()
        ep.bias, ep.act, ep.out, ep.ldo, ep.out_dtype = bias.ptr, act, o16.ptr, N + 8, L.BF16
        run(ep)
        bits = o16.read()
        assert np.array_equal(bits[:, N:], o16.initial()[:, N:])
        vals = D.bf16_value(bits[:, :N])
        assert np.isfinite(vals).all()
        if act == 0:                                   # z is exact: the bf16 output is known
            assert np.array_equal(vals, D.to_bf16(g["z"])[np.arange(M) % 128]), what
        cov = D.coverage(vals, N)
        print(f"{what}: {D.summary(cov)}")
        D.assert_coverage(cov, ["a", "d", "e"] + (["b_bf16"] if act == 0 else []), what)

        q, s = mx_outputs(cuda, M, N, so_rows)
        ep2 = L.VtdEpilogue()
        ep2.bias, ep2.act, ep2.out, ep2.ldo, ep2.out_dtype = bias.ptr, act, q.ptr, q.shape[1], L.FP8
        ep2.scale_out, ep2.scale_rows = s.ptr, so_rows
        run(ep2)
        check_mx(q, s, vals, N, so_rows, what)
        for b in (A, Bt, sA, sB, bias):
            assert np.array_equal(b.read().view(np.uint8), b.initial().view(np.uint8)), what
