"""The start of a pp2 workgroup (tile coordinates, buffer resources and per-lane DMA offsets,
the prologue DMA issued ahead of the statistics loads and the accumulator zeroing, the
prologue's and the first K-step's counted waits) on EXACT designed operands: the harness of
tests/test_gpu_gemm_designed.py (guard bands, np.array_equal against the float64 / int64
expectation of tests/gemm_designs.py), at the smallest shapes where that code takes another
path:

  K = 64 .. 256      nk = 1, 2, 3, 4: both prologue branches and every compile-time tail step,
                     on one tile (256 x 256) and on 6 tiles (512 x 768: an XCD remap whose
                     workgroup count is no multiple of 8); plain and LayerNorm-fold launches
                     (the fold kernels run the first K-step as a body of its own from nk = 3)
  512 x 2304         9 n-tiles: n-groups of 4, 4 and 1 in the grouped tile order
  300 x 260          partial tiles: the clamped (non-specialised) per-lane offsets
  4 | EPI_LNF        256 x 256 x 128 with (mean, rstd) that differ from row to row: statistics
                     waited for at a wrong count show as wrong rows
  12 | EPI_STAT      residual + partial statistics.  vtd_gemm writes statistics only from 64
                     tiles on (gemm_emits_stats refuses a 256 x 256 problem), so the launch is
                     64 tiles of 256 x 256 x 128: M = 16384
  split-K, bf16x3    ksplit = 2 at K = 256 (k0 != 0 in the source setup) and a split-bf16 A
                     operand whose K' range crosses the wrap (PP2Src<true>), split and unsplit
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_designs as G
from tests.test_gpu_gemm_designed import (check_out, col_mask, collect, in_buf, knobs, out_buf,
                                          route, run_gemm)

pytestmark = pytest.mark.gpu

KS = (64, 128, 192, 256)


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("fields", [("bias",), ("bias", "lnfold")], ids=["plain", "lnfold"])
def test_k_steps_one_tile_and_six(L, cuda, fields, tr):
    cases = [(M, N, K) for M, N in ((256, 256), (512, 768)) for K in KS]

    def one(c):
        M, N, K = c
        d = G.make_design("bf16", M, N, K, epi=fields)
        assert route("bf16", M, N, K, 0) == "pp2"
        with knobs(L, SKINNY=0, GEMM_TR=tr):
            run_gemm(L, cuda, d, out="bf16", fast=True, what=f"{fields} tr {tr} {c}")
    collect(cases, one)


@pytest.mark.parametrize("tr", [0, 1])
def test_grouped_order_with_narrow_last_group(L, cuda, tr):
    M, N, K = 512, 2304, 64
    d = G.make_design("bf16", M, N, K, epi=("bias",))
    assert route("bf16", M, N, K) == "pp2"
    with knobs(L, GEMM_TR=tr):
        run_gemm(L, cuda, d, out="bf16", fast=True, what=f"9 n-tiles tr {tr}")


@pytest.mark.parametrize("tr", [0, 1])
def test_partial_tiles_keep_the_clamped_start(L, cuda, tr):
    M, N, K = 300, 260, 128
    assert route("bf16", M, N, K, 0) == "pp2"
    with knobs(L, SKINNY=0, GEMM_TR=tr):
        run_gemm(L, cuda, G.make_design("bf16", M, N, K), what=f"partial generic tr {tr}")
        d = G.make_design("bf16", M, N, K, epi=("bias", "lnfold"))
        run_gemm(L, cuda, d, out="bf16", fast=True, what=f"partial fold tr {tr}")


def test_residual_and_statistics_launch(L, cuda):
    """Code 12 | EPI_STAT: the outputs exactly; the partial statistics (block mean, centred sum
    of squares of the STORED bf16 values, float32 arithmetic of at most 63 additions each)
    within their rounding bound: with u = 2^-24, |mean' - mean| <= d = 64 u mean|x| and
    |m2' - m2| <= 64 d^2 + 80 u (m2 + 64 d^2) (the shift of the centre adds exactly 64 d'^2;
    subtract, square, 63 additions: under 80 roundings)."""
    M, N, K = 256 * 64, 256, 128
    d = G.make_design("bf16", M, N, K, epi=("bias", "resid"))
    A, Bt = in_buf(cuda, d.a_op, K + 8), in_buf(cuda, d.b_op, K + 16)
    bias = in_buf(cuda, d.epi["bias"].astype(np.float32), N + 4)
    resid = in_buf(cuda, G.bf16_bits(d.epi["resid"].astype(np.float32)), N + 8)
    ldo, slots, stat_ld = N + 8, N // 64, M + 4
    want = np.zeros((M, ldo), np.uint16)
    want[:, :N] = G.cast_bf16(d.expected())
    o = out_buf(cuda, M, ldo, np.uint16, col_mask(M, ldo, (0, N)))
    st = out_buf(cuda, slots, 2 * stat_ld, np.float32, col_mask(slots, 2 * stat_ld, (0, 2 * M)))
    ep = L.VtdEpilogue()
    ep.bias, ep.resid, ep.ldr = bias.ptr, resid.ptr, N + 8
    ep.out, ep.ldo, ep.out_dtype = o.ptr, ldo, L.BF16
    ep.statout, ep.stat_ld = st.ptr, stat_ld
    L.check(L.lib.vtd_gemm(M, N, K, A.ptr, K + 8, Bt.ptr, K + 16, L.BF16, ctypes.byref(ep),
                           L.stream_ptr()), "residual + statistics")
    torch.cuda.synchronize()
    check_out(o, want, "residual + statistics")
    got = st.read()
    assert np.array_equal(got[:, 2 * M:].view(np.uint32), st.initial()[:, 2 * M:].view(np.uint32))
    got = got[:, :2 * M].reshape(slots, M, 2).astype(np.float64)
    xs = G.bf16_value(want[:, :N]).astype(np.float64).reshape(M, slots, 64).transpose(1, 0, 2)
    mean = xs.mean(2)
    m2 = ((xs - mean[..., None]) ** 2).sum(2)
    u = 2.0 ** -24
    dm = 64 * u * np.abs(xs).mean(2)
    em, e2 = np.abs(got[..., 0] - mean), np.abs(got[..., 1] - m2)
    b2 = 64 * dm ** 2 + 80 * u * (m2 + 64 * dm ** 2)
    print(f"statistics: worst mean error / bound {np.max(em / np.maximum(dm, 1e-300)):.3g}, "
          f"m2 error / bound {np.max(e2 / np.maximum(b2, 1e-300)):.3g}")
    assert (em <= dm).all() and (e2 <= b2).all()
    for b in (A, Bt, bias, resid):
        assert np.array_equal(b.read().view(np.uint8), b.initial().view(np.uint8))


def test_split_k_and_wrapped_a_operand(L, cuda):
    def bf16_split(c):
        M, N = c
        d = G.make_design("bf16", M, N, 256, epi=("bias",))
        assert route("bf16", M, N, 256) == "pp2"
        run_gemm(L, cuda, d, ksplit=2, what=f"splitk {c}")
        run_gemm(L, cuda, d, ksplit=2, out="bf16", fast=True, what=f"splitk bf16 out {c}")
    collect([(256, 512), (300, 328)], bf16_split)

    def x3(c):
        M, N, P = c
        # K' = 3 P = 6 or 9 K-steps, the wrap after 2 P / 64 = 4 or 6 of them
        d = G.make_design("bf16x3", M, N, P, epi=("bias",))
        assert route("bf16x3", M, N, d.Kcall) == "pp2"
        run_gemm(L, cuda, d, out="f32", fast=True, what=f"x3 f32 {c}")
        run_gemm(L, cuda, d, out="split", fast=True, what=f"x3 split out {c}")
        run_gemm(L, cuda, d, ksplit=2, what=f"x3 splitk {c}")      # the wrap inside split 1
    collect([(256, 512, 128), (300, 328, 192)], x3)
