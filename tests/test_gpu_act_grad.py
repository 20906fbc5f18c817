"""The elementwise pieces of the head backward on the GPU: vtd_act_grad against the float64
derivatives, vtd_act_forward against the GEMM epilogue's activation, vtd_head_unscatter
against a torch reshape.

Derivative bound: |err| <= 1e-5.  The derivatives are O(1); the same formulas in fp32 on the
CPU give 2e-7 (Mish) and 2e-6 (GELU), the ~1-ulp exp2 / rcp get 5x over that.  The result is
read back from its split-bf16 pieces, which hold a value v to 2^-17 |v|: measured on the GPU
7.7e-6 (Mish, at z = 1.1) and 7.6e-6 (GELU, at z = 2.44), all but ~1e-7 of it that
representation (the fp32 formula followed by the split gives 7.6e-6 on the CPU).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_grad_oracle as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def grid_values():
    special = [88.0, -88.0, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 20.0, 20.000002, 12.0, -12.0]
    g = np.linspace(-30.0, 30.0, 6001, dtype=np.float64)
    v = np.concatenate([g, np.asarray(special)]).astype(np.float32)
    pad = (-len(v)) % 64
    return np.concatenate([v, np.zeros(pad, np.float32)])


def split_ref(L, x32, P):
    rows, K = x32.shape
    out = torch.empty((rows, 2 * P), dtype=torch.bfloat16, device=x32.device)
    L.check(L.lib.vtd_split_bf16x3(x32.data_ptr(), rows, K, K, out.data_ptr(), 2 * P, 0,
                                   L.stream_ptr()), "split")
    return out


def act_grad(L, z, ga, act, dtype, N=None):
    rows, ld = z.shape
    N = ld if N is None else N
    P = -(-N // 64) * 64
    width = 2 * P if dtype == L.BF16X3 else P
    out = torch.full((rows, width), 7.0, dtype=torch.bfloat16, device=z.device)
    L.check(L.lib.vtd_act_grad(z.data_ptr(), ld, ga.data_ptr(), ld, rows, N, act, out.data_ptr(),
                               width, dtype, L.stream_ptr()), "vtd_act_grad")
    return out, P


@pytest.mark.parametrize("act_name", ["mish", "gelu"])
def test_act_grad_against_float64(L, cuda, act_name):
    act = L.ACT_MISH if act_name == "mish" else L.ACT_GELU_TANH
    v = grid_values()
    z = torch.from_numpy(v).reshape(-1, 64).to(cuda)
    ga = torch.ones_like(z)
    ref = H.act_grad64(v.astype(np.float64), act_name == "mish").reshape(-1, 64)
    out, P = act_grad(L, z, ga, act, L.BF16X3)
    hi, lo = out[:, :P].float(), out[:, P:].float()
    got = (hi.double() + lo.double()).cpu()
    assert bool(torch.isfinite(got).all()), "the derivative must be finite for every finite z"
    err = (got - ref).abs()
    print(f"{act_name}: worst |err| {float(err.max()):.3g} at z = "
          f"{float(z.flatten()[int(err.argmax())]):.6g}")
    assert float(err.max()) <= 1e-5
    if act_name == "mish":        # exactly 1 where the forward returns x
        big = z > 20.0
        assert bool((hi[big] == 1.0).all()) and bool((lo[big] == 0.0).all())
    # the bf16 form is the hi piece: both round the same fp32 result
    out16, _ = act_grad(L, z, ga, act, L.BF16)
    assert torch.equal(out16.view(torch.int16), out[:, :P].contiguous().view(torch.int16))


@pytest.mark.parametrize("act_name", ["mish", "gelu"])
def test_act_grad_is_finite_at_the_ends_of_the_float_range(L, cuda, act_name):
    act = L.ACT_MISH if act_name == "mish" else L.ACT_GELU_TANH
    v = np.zeros(64, np.float32)
    v[:8] = [1e30, -1e30, 3.0e38, -3.0e38, 1e19, -1e19, 200.0, -200.0]
    z = torch.from_numpy(v).reshape(1, 64).to(cuda)
    out, P = act_grad(L, z, torch.ones_like(z), act, L.BF16X3)
    got = (out[:, :P].float() + out[:, P:].float())[0, :8].cpu().numpy()
    assert np.array_equal(got, np.asarray([1, 0, 1, 0, 1, 0, 1, 0], np.float32)), got


def test_act_grad_scales_by_the_incoming_gradient_and_zeroes_the_pad(L, cuda):
    g = torch.Generator(device="cpu").manual_seed(3)
    z = (torch.randn((37, 136), generator=g) * 3).to(cuda)
    ga = torch.randn((37, 136), generator=g).to(cuda)
    ref = (ga.double().cpu() * H.act_grad64(z.cpu().numpy().astype(np.float64), True))
    for N in (136, 100):
        out, P = act_grad(L, z, ga, L.ACT_MISH, L.BF16X3, N=N)
        got = out[:, :P].double() + out[:, P:].double()
        assert float((got[:, :N].cpu() - ref[:, :N]).abs().max()) <= 1e-5 * float(ga.abs().max())
        assert bool((out[:, N:P] == 0).all()) and bool((out[:, P + N:] == 0).all())


def test_act_grad_pieces_are_the_split_of_the_fp32_result(L, cuda):
    """VTD_ACT_NONE makes the fp32 result the incoming gradient itself: the pieces are then
    vtd_split_bf16x3 role 0 of it, bit for bit (ragged N: pad columns zero)."""
    g = torch.Generator(device="cpu").manual_seed(8)
    z = torch.randn((33, 100), generator=g).to(cuda)
    ga = (torch.randn((33, 100), generator=g) * 1e-3).to(cuda)
    out, P = act_grad(L, z, ga, L.ACT_NONE, L.BF16X3)
    assert torch.equal(out.view(torch.int16), split_ref(L, ga, P).view(torch.int16))


def test_act_forward_none_is_the_split(L, cuda):
    """VTD_ACT_NONE: the conversion alone, bit for bit what vtd_split_bf16x3 role 0 writes
    (ragged N: the pad columns zero) and, in bf16, torch's round-to-nearest-even."""
    g = torch.Generator(device="cpu").manual_seed(4)
    z = torch.randn((29, 100), generator=g).to(cuda)
    P = 128
    want = split_ref(L, z, P)
    out = torch.full((29, 2 * P), 7.0, dtype=torch.bfloat16, device=cuda)
    L.check(L.lib.vtd_act_forward(z.data_ptr(), 29, 100, 100, L.ACT_NONE, out.data_ptr(), 2 * P,
                                  L.BF16X3, L.stream_ptr()), "vtd_act_forward")
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    out16 = torch.full((29, P), 7.0, dtype=torch.bfloat16, device=cuda)
    L.check(L.lib.vtd_act_forward(z.data_ptr(), 29, 100, 100, L.ACT_NONE, out16.data_ptr(), P,
                                  L.BF16, L.stream_ptr()), "vtd_act_forward")
    assert torch.equal(out16[:, :100], z.to(torch.bfloat16)) and bool((out16[:, 100:] == 0).all())


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("act_name", ["mish", "gelu"])
def test_act_forward_equals_the_gemm_epilogue(L, cuda, act_name, mode):
    """z through an identity GEMM (the accumulator is z exactly: z is chosen to be hi + lo of a
    split, resp. a bf16 value) with the activation in its epilogue, against vtd_act_forward of
    the same z: the same bits."""
    act = L.ACT_MISH if act_name == "mish" else L.ACT_GELU_TANH
    v = torch.from_numpy(grid_values()[:6016]).reshape(-1, 64).to(cuda)
    M = v.shape[0]
    eye = torch.eye(64, dtype=torch.float32, device=cuda)
    if mode == "bf16x3":
        s = split_ref(L, v, 64)
        z = (s[:, :64].float() + s[:, 64:].float()).contiguous()
        a = split_ref(L, z, 64)
        bt = torch.empty((64, 192), dtype=torch.bfloat16, device=cuda)
        L.check(L.lib.vtd_split_bf16x3(eye.data_ptr(), 64, 64, 64, bt.data_ptr(), 192, 1,
                                       L.stream_ptr()), "split")
        dtype, K, lda, ldo = L.BF16X3, 192, 128, 128
    else:
        # an MFMA accumulator holds neither -0 (0 + -0 * 1 = +0) nor a denormal: z without them
        a = v.to(torch.bfloat16)
        a[a.float().abs() < 1.2e-38] = 0
        a = a.contiguous()
        z = a.float().contiguous()
        bt = eye.to(torch.bfloat16).contiguous()
        dtype, K, lda, ldo = L.BF16, 64, 64, 64
    want = torch.zeros((M, ldo), dtype=torch.bfloat16, device=cuda)
    e = L.VtdEpilogue()
    e.act, e.out, e.ldo, e.out_dtype = act, want.data_ptr(), ldo, dtype
    L.check(L.lib.vtd_gemm(M, 64, K, a.data_ptr(), lda, bt.data_ptr(), K, dtype, ctypes.byref(e),
                           L.stream_ptr()), "vtd_gemm")
    got = torch.zeros((M, ldo), dtype=torch.bfloat16, device=cuda)
    L.check(L.lib.vtd_act_forward(z.data_ptr(), M, 64, 64, act, got.data_ptr(), ldo, dtype,
                                  L.stream_ptr()), "vtd_act_forward")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("T", [25, 40, 400])
def test_head_unscatter_is_the_inverse_reshape(L, cuda, T):
    B = 3
    ldu = -(-T // 64) * 64
    g = torch.Generator(device="cpu").manual_seed(T)
    dU = torch.randn((B * 17, ldu), generator=g).to(cuda)
    ref = dU[:, :T].reshape(B, 17 * T).reshape(B * T, 17).contiguous()
    want = split_ref(L, ref, 64)
    out = torch.full((B * T, 128), 7.0, dtype=torch.bfloat16, device=cuda)
    L.check(L.lib.vtd_head_unscatter(dU.data_ptr(), B, T, ldu, out.data_ptr(), 128, L.BF16X3,
                                     L.stream_ptr()), "vtd_head_unscatter")
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    out16 = torch.full((B * T, 64), 7.0, dtype=torch.bfloat16, device=cuda)
    L.check(L.lib.vtd_head_unscatter(dU.data_ptr(), B, T, ldu, out16.data_ptr(), 64, L.BF16,
                                     L.stream_ptr()), "vtd_head_unscatter")
    assert torch.equal(out16[:, :17], ref.to(torch.bfloat16)) and bool((out16[:, 17:] == 0).all())
