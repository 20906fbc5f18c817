"""vtd_gemm_wgrad on the GPU: dW = X^T G and db = sum_m G against float64, in both operand
modes, at every msplit the head backward would pick and at forced ones.

Bounds (derived, not measured), componentwise with S = |X|^T |G|:
  VTD_BF16X3, against the f32 values before the split: (2^-15 + M 2^-24) S -- hi + lo holds
    each factor to 2^-17 (two factors: 2^-16), the dropped lo lo term is <= 2^-18, together
    under 2^-15; M 2^-24 for the fp32 accumulation;
  VTD_BF16, against the stored bf16 values: 2^-7 S;
  db against the stored values (hi + lo is exact in f32): M 2^-24 sum |g|.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, K, N, forced msplit values)
SHAPES = [
    (17, 64, 6, ()),              # smallest
    (51, 200, 136, ()),           # ragged M, K and N padded to 256 / 192
    (187, 320, 272, ()),          # more than one output tile both ways
    (300, 64, 17, (1, 2, 5)),     # uneven ranges
    (4352, 256, 320, ()),         # head row count
    (2 * 400, 32, 17, ()),        # the Dense(17) shape of tiny_seq400
]


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def pad64(n):
    return -(-n // 64) * 64


def operand(L, x32, dtype):
    """The device operand of f32 x [M][K] and the float64 values it stores."""
    M, K = x32.shape
    P = pad64(K)
    if dtype == L.BF16:
        op = torch.zeros((M, P), dtype=torch.bfloat16, device=x32.device)
        op[:, :K] = x32.to(torch.bfloat16)
        return op, P, op[:, :K].double()
    op = torch.empty((M, 2 * P), dtype=torch.bfloat16, device=x32.device)
    L.check(L.lib.vtd_split_bf16x3(x32.data_ptr(), M, K, K, op.data_ptr(), 2 * P, 0,
                                   L.stream_ptr()), "split")
    return op, 2 * P, op[:, :K].double() + op[:, P:P + K].double()


def run(L, M, K, N, xop, ldx, gop, ldg, dtype, msplit, ldw, with_db=True):
    dev = xop.device
    dW = torch.full((K, ldw), float("nan"), dtype=torch.float32, device=dev)
    db = torch.full((N,), float("nan"), dtype=torch.float32, device=dev) if with_db else None
    nbytes = msplit * (K + 1) * N * 4 if msplit > 1 else 0
    part = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    L.check(L.lib.vtd_gemm_wgrad(M, K, N, xop.data_ptr(), ldx, gop.data_ptr(), ldg, dtype,
                                 dW.data_ptr(), ldw, L.ptr(db), part.data_ptr(), nbytes, msplit,
                                 L.stream_ptr()), "vtd_gemm_wgrad")
    torch.cuda.synchronize()
    return dW, db


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_wgrad_against_float64(L, cuda, shape, mode):
    M, K, N, forced = shape
    dtype = L.BF16X3 if mode == "bf16x3" else L.BF16
    g = torch.Generator(device="cpu").manual_seed(M * 131 + K * 7 + N)
    x32 = torch.randn((M, K), generator=g).to(cuda)
    g32 = (torch.randn((M, N), generator=g) * 0.1).to(cuda)
    xop, ldx, xs = operand(L, x32, dtype)
    gop, ldg, gs = operand(L, g32, dtype)
    if mode == "bf16x3":
        ref = x32.double().T @ g32.double()
        S = x32.double().abs().T @ g32.double().abs()
        bound = (2.0 ** -15 + M * 2.0 ** -24) * S
    else:
        ref = xs.T @ gs
        S = xs.abs().T @ gs.abs()
        bound = 2.0 ** -7 * S
    db_ref = gs.sum(0)
    db_bound = M * 2.0 ** -24 * gs.abs().sum(0)
    choice = L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype)
    assert 1 <= choice <= -(-M // 32)
    ldw = N + 3
    for msplit in sorted({1, choice, *forced}):
        dW, db = run(L, M, K, N, xop, ldx, gop, ldg, dtype, msplit, ldw)
        err = (dW[:, :N].double() - ref).abs()
        worst = float((err / S.clamp_min(1e-300)).max())
        print(f"{mode} {M}x{K}x{N} msplit {msplit}: worst |err| / S = {worst:.3g}, "
              f"db worst {float(((db.double() - db_ref).abs() / gs.abs().sum(0)).max()):.3g}")
        assert bool((err <= bound).all()), f"msplit {msplit}: |err| / S up to {worst:.3g}"
        assert bool(((db.double() - db_ref).abs() <= db_bound).all())
        assert bool((dW[:, N:] == 0).all()), "pad columns [N, ldw) must be written as zero"
        dW2, db2 = run(L, M, K, N, xop, ldx, gop, ldg, dtype, msplit, ldw)
        assert torch.equal(dW, dW2) and torch.equal(db, db2), "two runs differ"


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
def test_padded_k_rows_are_zero_and_db_is_optional(L, cuda, mode):
    """The padding rule of vtd.h: K may be the padded width; the rows of X's zero pad columns
    come out zero.  db_dev may be NULL."""
    M, K, N = 51, 200, 136
    dtype = L.BF16X3 if mode == "bf16x3" else L.BF16
    g = torch.Generator(device="cpu").manual_seed(5)
    x32 = torch.randn((M, K), generator=g).to(cuda)
    g32 = torch.randn((M, N), generator=g).to(cuda)
    xop, ldx, _ = operand(L, x32, dtype)
    gop, ldg, _ = operand(L, g32, dtype)
    Kp = pad64(K)
    for msplit in (1, 2):
        full, _ = run(L, M, Kp, N, xop, ldx, gop, ldg, dtype, msplit, N, with_db=False)
        real, _ = run(L, M, K, N, xop, ldx, gop, ldg, dtype, msplit, N)
        assert bool((full[K:] == 0).all())
        assert torch.equal(full[:K], real)
