"""vtd_attention_train / vtd_attention_backward / attention_core on the GPU against float64
(tests/attention_grad_oracle.py; the host half is tests/test_attention_grad_kat.py).

Random inputs (q, k, v, dO ~ N(0, sigma), scale = 1 / sqrt(key_dim)), per tensor
max |g - g64| / max |g64| <= 2e-4 (bf16x3) / 5e-2 (bf16), lse within 2e-5 / 2e-2 of
max(1, max |lse64|); designed score patterns (tests/test_gpu_attention_patterns.make_case), whose
gradients nearly cancel, componentwise |g - g64| <= c den with c = 2^-15 / 2^-7; the training
forward's O bit-identical to vtd_attention; two backward runs bit-identical; 0xA5 guards
around dqkv, lse and the workspace; the autograd op against the C call and a float64 torch
autograd.  Every buffer has slack columns, so leading dimensions differ from the widths.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_grad_oracle as A
from tests.test_gpu_attention_patterns import LN2_F32, dkp_of, make_case, pack_qkv

pytestmark = pytest.mark.gpu
MODES = ("x3", "bf16")
SHAPE_IDS = ["x".join(map(str, s)) for s in A.SHAPES]
GUARD = 0xA5


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def _guarded(cuda, nbytes, front, back):
    """A uint8 device buffer of 0xA5 with `front` / `back` guard bytes around nbytes."""
    return torch.full((front + nbytes + back,), GUARD, dtype=torch.uint8, device=cuda)


def _bf16_bits_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def device_backward(L, cuda, mode, qkv, do, B, N, H, dk, scale):
    """One training forward and TWO backward runs of the C entries on qkv fp32 [B*N][ld] and dO
    [B][N][H][dk].  Returns o, lse, dq, dk, dv (float64, [B][N][H][dkp] / [B][H][N]), the raw
    O operand, and what the guard, padding and repeat checks found."""
    dkp = dkp_of(dk)
    inner = H * dkp
    rows = B * N
    x3 = mode == "x3"
    code = L.BF16X3 if x3 else L.BF16
    ld = qkv.shape[1]
    qkv_d = torch.from_numpy(qkv).to(cuda) if x3 else torch.from_numpy(qkv).to(torch.bfloat16).to(cuda)
    # O: bf16 [rows][inner + 16], or split with piece width inner + 64
    opiece = inner + (64 if x3 else 16)
    ldo = 2 * opiece if x3 else opiece
    o_d = torch.full((rows, ldo), -1, dtype=torch.int16, device=cuda)
    lse_buf = _guarded(cuda, B * H * N * 4, 64, 64)
    L.check(L.lib.vtd_attention_train(qkv_d.data_ptr(), B, N, H, dkp, ld, float(scale),
                                      o_d.data_ptr(), ldo, lse_buf.data_ptr() + 64, code,
                                      L.stream_ptr()), "vtd_attention_train")
    # dO: [rows][inner + 8], pad columns zero
    do_np = np.zeros((rows, inner + 8), np.float32)
    for h in range(H):
        do_np[:, h * dkp:h * dkp + dk] = do[:, :, h, :].reshape(rows, dk)
    do_d = torch.from_numpy(do_np).to(cuda)
    if not x3:
        assert (do_d.to(torch.bfloat16).float() == do_d).all()
        do_d = do_d.to(torch.bfloat16)
    piece = 3 * inner + 8
    ldd = 2 * piece if x3 else piece
    n = L.c_size_t(0)
    L.check(L.lib.vtd_attention_backward_workspace_bytes(B, N, H, dkp, code, ctypes.byref(n)))
    raws = []
    guards_ok = True
    for _ in range(2):
        dq_buf = _guarded(cuda, rows * ldd * 2, 2 * ldd * 2, 2 * ldd * 2)
        ws_buf = _guarded(cuda, n.value, 256, 256)
        L.check(L.lib.vtd_attention_backward(
            qkv_d.data_ptr(), o_d.data_ptr(), do_d.data_ptr(), lse_buf.data_ptr() + 64, B, N, H, dkp,
            ld, ldo, inner + 8, float(scale), dq_buf.data_ptr() + 2 * ldd * 2, ldd, code,
            ws_buf.data_ptr() + 256, n.value, L.stream_ptr()), "vtd_attention_backward")
        torch.cuda.synchronize()
        raw = dq_buf.cpu().numpy().view(np.uint16).reshape(rows + 4, ldd)
        wsb = ws_buf.cpu().numpy()
        guards_ok &= bool((raw[:2] == 0xA5A5).all() and (raw[-2:] == 0xA5A5).all())
        guards_ok &= bool((wsb[:256] == GUARD).all() and (wsb[-256:] == GUARD).all())
        for p0 in range(0, ldd, piece):
            guards_ok &= bool((raw[2:-2, p0 + 3 * inner:p0 + piece] == 0xA5A5).all())
        raws.append(raw[2:-2])
    lse_all = lse_buf.cpu().numpy()
    guards_ok &= bool((lse_all[:64] == GUARD).all() and (lse_all[-64:] == GUARD).all())
    lse = lse_all[64:-64].view(np.float32).astype(np.float64).reshape(B, H, N)
    raw = raws[0]
    g = _bf16_bits_to_f64(raw[:, :3 * inner])
    if x3:
        g = g + _bf16_bits_to_f64(raw[:, piece:piece + 3 * inner])
    parts = [g[:, i * inner:(i + 1) * inner].reshape(B, N, H, dkp) for i in range(3)]
    o_raw = o_d.cpu().numpy().view(np.uint16)
    o = _bf16_bits_to_f64(o_raw[:, :inner])
    if x3:
        o = o + _bf16_bits_to_f64(o_raw[:, opiece:opiece + inner])
    return dict(o=o.reshape(B, N, H, dkp), o_raw=o_raw, lse=lse, dq=parts[0], dk=parts[1],
                dv=parts[2], guards_ok=guards_ok, repeat_ok=bool((raws[0] == raws[1]).all()),
                pads_zero=all(bool((p[..., dk:] == 0).all()) for p in parts),
                qkv_d=qkv_d, ld=ld, ldo=ldo, opiece=opiece, code=code)


@pytest.fixture(scope="module")
def random_runs(L, cuda):
    """One device run and one float64 reference per (shape, mode), shared by the tests below."""
    cache = {}

    def get(shape, mode):
        if (shape, mode) not in cache:
            B, H, N, dk = shape
            (q, k, v, do), scale = A.random_case(shape, mode)
            qkv = pack_qkv(*(t.astype(np.float32) for t in (q, k, v)), dkp_of(dk))
            run = device_backward(L, cuda, mode, qkv, do, B, N, H, dk, scale)
            run["errors"] = A.tensor_errors([run[n][..., :dk] for n in ("dq", "dk", "dv")],
                                            q, k, v, do, scale)
            _, lse64, _ = A.forward64(q, k, v, scale)
            run["lse_err"] = float(np.abs(run["lse"] - lse64).max() / max(1.0, np.abs(lse64).max()))
            run["scale"] = scale
            cache[(shape, mode)] = run
        return cache[(shape, mode)]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_random_gradients_and_lse(random_runs, shape, mode):
    run = random_runs(shape, mode)
    print(f"{shape} {mode} sigma {A.SIGMA[shape]}: dQ dK dV errors "
          f"{' '.join(f'{e:.3g}' for e in run['errors'])} (bar {A.BARS[mode]}), "
          f"lse {run['lse_err']:.3g} (bar {A.LSE_TOL[mode]})")
    assert np.isfinite(run["lse"]).all()
    assert all(np.isfinite(run[n]).all() for n in ("dq", "dk", "dv"))
    assert max(run["errors"]) <= A.BARS[mode]
    assert run["lse_err"] <= A.LSE_TOL[mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_training_forward_output_is_vtd_attention_bit_for_bit(L, cuda, random_runs, shape, mode):
    """x3 at the default, bf16 with VTD_KNOB_ATTN_VARIANT 2."""
    run = random_runs(shape, mode)
    B, H, N, dk = shape
    ref = torch.full_like(torch.from_numpy(run["o_raw"].view(np.int16)), -1).to(cuda)
    with L.knob(L.KNOB_ATTN_VARIANT, -1 if mode == "x3" else 2):
        L.check(L.lib.vtd_attention(run["qkv_d"].data_ptr(), B, N, H, dkp_of(dk), run["ld"],
                                    float(run["scale"]), ref.data_ptr(), run["ldo"], run["code"],
                                    L.stream_ptr()), "vtd_attention")
    torch.cuda.synchronize()
    assert (ref.cpu().numpy().view(np.uint16) == run["o_raw"]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_backward_repeats_bit_for_bit_and_respects_guards(random_runs, shape, mode):
    """Two runs into fresh 0xA5 buffers: equal bits; only rows < B N, columns [0, 3 heads dkp) of
    each piece change, pad columns of a head are zero; lse and the workspace keep their guards."""
    run = random_runs(shape, mode)
    assert run["repeat_ok"]
    assert run["guards_ok"]
    assert run["pads_zero"]


DESIGNED = [(p, N, dk) for p in A.DESIGNED_PATTERNS for N, dk in A.DESIGNED_SHAPES]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pattern,N,dk", DESIGNED)
def test_designed_patterns_componentwise(L, cuda, pattern, N, dk, mode):
    """Key identity and ragged tails, invisible in diffuse rows: |g - g64| <= c den with
    den_dQ = A |K|, den_dK = A^T |Q|, den_dV = P^T |dO| (attention_grad_oracle.magnitudes)."""
    from tests.test_gpu_attention_patterns import B, H, tie_positions
    qkv, _, _, _ = make_case(pattern, N, dk)
    q, k, v = A.unpack_qkv(qkv, B, N, H, dk)
    do = A.designed_do(pattern, N, dk)
    scale = float(LN2_F32)
    run = device_backward(L, cuda, mode, qkv, do, B, N, H, dk, LN2_F32)
    g64 = A.backward64(q, k, v, do, scale)
    den = A.magnitudes(q, k, v, do, scale)
    worst = 0.0
    exact_zero = True
    for n, g, d in zip(("dq", "dk", "dv"), g64, den):
        err = np.abs(run[n][..., :dk] - g)
        exact_zero &= bool((err[d == 0] == 0).all())
        worst = max(worst, float((err[d > 0] / d[d > 0]).max()))
    print(f"{pattern} N {N} dk {dk} {mode}: worst |g - g64| / den {worst:.3g} "
          f"(bar {A.C_DESIGNED[mode]:.3g})")
    assert run["guards_ok"] and run["repeat_ok"] and run["pads_zero"]
    assert exact_zero
    assert worst <= A.C_DESIGNED[mode]
    if pattern == "tie":
        # the two tied keys have identical score columns: equal weight in dV = P^T dO (a
        # double-counted clamped key N - 1 would give 1/3 : 2/3)
        for p0, p1 in tie_positions(N):
            if p0 != p1:
                assert (run["dv"][:, p0] == run["dv"][:, p1]).all()


@pytest.mark.parametrize("mode", MODES)
def test_autograd_op(L, cuda, random_runs, mode):
    """attention_core(...).backward() fills qkv.grad: the C call's bits, and within the random
    bars of a float64 torch autograd of the same formula, at (2, 2, 196, 40)."""
    import vision_transformer_detector_amd as vtd
    shape = (2, 2, 196, 40)
    B, H, N, dk = shape
    dkp = dkp_of(dk)
    inner = H * dkp
    (q, k, v, do), scale = A.random_case(shape, mode)
    tdt = torch.float32 if mode == "x3" else torch.bfloat16
    qkv_np = pack_qkv(*(t.astype(np.float32) for t in (q, k, v)), dkp)[:, :3 * inner]
    qkv = torch.from_numpy(np.ascontiguousarray(qkv_np)).to(tdt).to(cuda).reshape(B, N, 3 * inner)
    qkv.requires_grad_(True)
    g = np.zeros((B, N, H, dkp), np.float32)
    g[..., :dk] = do
    out = vtd.attention_core(qkv, H, dk, dtype="bf16x3" if mode == "x3" else "bf16")
    assert out.shape == (B, N, inner) and out.dtype == tdt
    out.backward(torch.from_numpy(g).reshape(B, N, inner).to(tdt).to(cuda))
    assert qkv.grad is not None and qkv.grad.shape == qkv.shape and qkv.grad.dtype == tdt
    grad = qkv.grad.double().cpu().numpy().reshape(B, N, 3, H, dkp)
    run = random_runs(shape, mode)
    # (the plain bf16x3 tensors are float32(hi + lo); in bf16 the cast changes nothing)
    assert (out.detach().double().cpu().numpy().reshape(B, N, H, dkp) ==
            run["o"].astype(np.float32)).all()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert (grad[:, :, i] == run[name].astype(np.float32)).all(), name
    # float64 torch autograd on the CPU
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v)]
    s = torch.einsum("bqhd,bkhd->bhqk", t[0], t[1]) * scale
    o64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), t[2])
    (o64 * torch.tensor(do)).sum().backward()
    for i, name in enumerate(("dq", "dk", "dv")):
        err = A.rel_err(grad[:, :, i][..., :dk], t[i].grad.numpy())
        print(f"autograd {mode} {name}: {err:.3g}")
        assert err <= A.BARS[mode]
