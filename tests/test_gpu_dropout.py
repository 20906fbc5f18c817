"""Dropout on the GPU: the kernels' mask against its numpy restatement, the elementwise DROP
kernels exactly, and vtd_attention_train_dropout / vtd_attention_backward_dropout /
attention_core(dropout=...) against the masked float64 oracle (tests/dropout_oracle.py; the host
half is tests/test_dropout_kat.py).

Random attention inputs are those of tests/test_gpu_attention_backward.py with its measure and
bars (max |g - g64| / max |g64| <= 2e-4 bf16x3 / 5e-2 bf16 per tensor): masking rescales the
device's and the oracle's terms alike.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_grad_oracle as A
from tests import dropout_oracle as D
from tests.test_gpu_attention_patterns import dkp_of, pack_qkv

pytestmark = pytest.mark.gpu
MODES = ("x3", "bf16")
RATES = (0.1, 0.5)
SHAPE_IDS = ["x".join(map(str, s)) for s in A.SHAPES]
GUARD = 0xA5
SEED, STEP, SITE = 0x1234567887654321, 3, 5


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def _drop(L, rate, seed=SEED, step=STEP, site=SITE):
    return L.VtdDropout(seed=seed, step=step, site=site, rate=rate)


def _bits_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _guarded(cuda, nbytes, front, back):
    return torch.full((front + nbytes + back,), GUARD, dtype=torch.uint8, device=cuda)


# ------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("rows,N", [(1, 1), (3, 7), (5, 130)])
@pytest.mark.parametrize("rate", [0.25, 0.5])
def test_mask_entry_is_the_numpy_mask(L, cuda, rows, N, rate):
    ldo = N + 5
    buf = _guarded(cuda, rows * ldo, 64, 64)
    d = _drop(L, rate)
    L.check(L.lib.vtd_dropout_mask(ctypes.byref(d), rows, N, buf.data_ptr() + 64, ldo,
                                   L.stream_ptr()), "vtd_dropout_mask")
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:64] == GUARD).all() and (raw[-64:] == GUARD).all()
    body = raw[64:-64].reshape(rows, ldo)
    assert (body[:, N:] == GUARD).all()
    assert (body[:, :N] == D.mask_rows(rows, N, rate, SEED, STEP, SITE).astype(np.uint8)).all()


@pytest.mark.parametrize("B,H,N", [(1, 1, 1), (2, 2, 33), (1, 2, 130)])
def test_attention_mask_entry_is_the_numpy_mask(L, cuda, B, H, N):
    buf = _guarded(cuda, B * H * N * N, 64, 64)
    d = _drop(L, 0.5)
    L.check(L.lib.vtd_dropout_mask_attention(ctypes.byref(d), B, H, N, buf.data_ptr() + 64,
                                             L.stream_ptr()), "vtd_dropout_mask_attention")
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:64] == GUARD).all() and (raw[-64:] == GUARD).all()
    want = D.mask_attention(B, H, N, 0.5, SEED, STEP, SITE)
    assert (raw[64:-64].reshape(B, H, N, N) == want.astype(np.uint8)).all()


def test_python_dropout_mask(cuda):
    import vision_transformer_detector_amd as vtd
    m = vtd.dropout_mask((5, 130), 0.25, seed=7, step=1, site=2, device=cuda)
    assert m.dtype == torch.bool
    assert (m.cpu().numpy() == D.mask_rows(5, 130, 0.25, 7, 1, 2)).all()
    m = vtd.dropout_mask((2, 2, 33, 33), 0.5, seed=7, device=cuda)
    assert (m.cpu().numpy() == D.mask_attention(2, 2, 33, 0.5, 7)).all()
    assert vtd.dropout_mask((3, 4), 0.0, seed=None, device=cuda).all()
    with pytest.raises(ValueError, match="seed"):
        vtd.dropout_mask((3, 4), 0.5, seed=None, device=cuda)


# ------------------------------------------------------------------------------ elementwise
ACTS = ("none", "mish", "gelu")
EW_SHAPES = [(3, 7), (5, 130), (70, 64)]


def _act_run(L, cuda, z, ga, act, x3, drop):
    """vtd_act_forward[_dropout] (ga None) or vtd_act_grad[_dropout]: the raw uint16 output
    [rows][ld], P = N rounded up to 8 plus 8 slack columns per piece."""
    rows, N = z.shape
    P = (N + 7) // 8 * 8 + 8
    ld = 2 * P if x3 else P
    code = L.BF16X3 if x3 else L.BF16
    out = torch.full((rows, ld), -1, dtype=torch.int16, device=cuda)
    zd = torch.zeros((rows, N + 3), device=cuda)
    zd[:, :N] = torch.from_numpy(z).to(cuda)
    a = {"none": L.ACT_NONE, "mish": L.ACT_MISH, "gelu": L.ACT_GELU_TANH}[act]
    if ga is None:
        if drop is None:
            rc = L.lib.vtd_act_forward(zd.data_ptr(), rows, N, N + 3, a, out.data_ptr(), ld, code,
                                       L.stream_ptr())
        else:
            rc = L.lib.vtd_act_forward_dropout(zd.data_ptr(), rows, N, N + 3, a, out.data_ptr(), ld,
                                               code, L.stream_ptr(), ctypes.byref(drop))
    else:
        gd = torch.zeros((rows, N + 1), device=cuda)
        gd[:, :N] = torch.from_numpy(ga).to(cuda)
        if drop is None:
            rc = L.lib.vtd_act_grad(zd.data_ptr(), N + 3, gd.data_ptr(), N + 1, rows, N, a,
                                    out.data_ptr(), ld, code, L.stream_ptr())
        else:
            rc = L.lib.vtd_act_grad_dropout(zd.data_ptr(), N + 3, gd.data_ptr(), N + 1, rows, N, a,
                                            out.data_ptr(), ld, code, L.stream_ptr(),
                                            ctypes.byref(drop))
    L.check(rc, "act")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16), P


@pytest.mark.parametrize("grad", [False, True], ids=["forward", "grad"])
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows,N", EW_SHAPES)
def test_elementwise_rate_half_is_exactly_twice_or_zero(L, cuda, rows, N, act, x3, grad):
    rng = np.random.default_rng([rows, N])
    z = rng.normal(0, 2, size=(rows, N)).astype(np.float32)
    ga = rng.normal(0, 1, size=(rows, N)).astype(np.float32) if grad else None
    plain, P = _act_run(L, cuda, z, ga, act, x3, None)
    drop, _ = _act_run(L, cuda, z, ga, act, x3, _drop(L, 0.5))
    zero, _ = _act_run(L, cuda, z, ga, act, x3, _drop(L, 0.0))
    assert (zero == plain).all()                       # rate 0: the existing kernel's bits
    keep = D.mask_rows(rows, N, 0.5, SEED, STEP, SITE)
    assert keep.any() and not keep.all() or rows * N < 4
    for p0 in range(0, plain.shape[1], P):             # the bf16 piece, or hi then lo
        a, b = plain[:, p0:p0 + N], drop[:, p0:p0 + N]
        assert (_bits_f64(b)[keep] == 2.0 * _bits_f64(a)[keep]).all()
        assert (b[~keep] == 0).all()                   # +0, not -0
        assert (drop[:, p0 + N:p0 + P] == 0).all()     # pad columns [N, piece width) zero


@pytest.mark.parametrize("rows,N", EW_SHAPES)
def test_dropout_apply_fp32_rate_quarter_is_one_fp32_multiply(L, cuda, rows, N):
    rng = np.random.default_rng([rows, N, 1])
    x = rng.normal(0, 2, size=(rows, N)).astype(np.float32)
    xd = torch.full((rows, N + 3), 7.0, device=cuda)
    xd[:, :N] = torch.from_numpy(x).to(cuda)
    yd = torch.full((rows, N + 2), -3.0, device=cuda)
    d = _drop(L, 0.25)
    L.check(L.lib.vtd_dropout_apply(ctypes.byref(d), xd.data_ptr(), N + 3, rows, N, yd.data_ptr(),
                                    N + 2, L.stream_ptr()), "vtd_dropout_apply")
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    keep = D.mask_rows(rows, N, 0.25, SEED, STEP, SITE)
    want = np.where(keep, x * D.inv_keep(0.25), np.float32(0.0)).astype(np.float32)
    assert (y[:, :N].view(np.uint32) == want.view(np.uint32)).all()
    assert (y[:, N:] == -3.0).all()


def test_dropout_op_forward_and_backward(cuda):
    import vision_transformer_detector_amd as vtd
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(size=(2, 5, 130)).astype(np.float32)).to(cuda).requires_grad_(True)
    g = torch.from_numpy(rng.normal(size=(2, 5, 130)).astype(np.float32)).to(cuda)
    y = vtd.dropout(x, 0.25, seed=7, step=2, site=1)
    y.backward(g)
    keep = D.mask_rows(10, 130, 0.25, 7, 2, 1).reshape(2, 5, 130)
    c = D.inv_keep(0.25)
    assert (y.detach().cpu().numpy() == np.where(keep, x.detach().cpu().numpy() * c, 0)).all()
    assert (x.grad.cpu().numpy() == np.where(keep, g.cpu().numpy() * c, 0)).all()
    assert vtd.dropout(x, None, seed=None) is x and vtd.dropout(x, 0.0, seed=None) is x
    with pytest.raises(ValueError, match="seed"):
        vtd.dropout(x, 0.5, seed=None)
    y2 = vtd.dropout(x, 0.25, seed=7, step=3, site=1)
    assert not torch.equal(y2, y)


# -------------------------------------------------------------------------------- attention
def device_run(L, cuda, mode, qkv, do, B, N, H, dk, scale, drop):
    """The training forward and TWO backward runs with `drop` (a VtdDropout, or None for the
    existing entries) on qkv fp32 [B*N][ld] and dO [B][N][H][dk]; slack columns everywhere."""
    dkp = dkp_of(dk)
    inner, rows, x3 = H * dkp, B * N, mode == "x3"
    code = L.BF16X3 if x3 else L.BF16
    ld = qkv.shape[1]
    qkv_d = torch.from_numpy(qkv).to(cuda) if x3 else torch.from_numpy(qkv).to(torch.bfloat16).to(cuda)
    opiece = inner + (64 if x3 else 16)
    ldo = 2 * opiece if x3 else opiece
    o_d = torch.full((rows, ldo), -1, dtype=torch.int16, device=cuda)
    lse_buf = _guarded(cuda, B * H * N * 4, 64, 64)
    dref = ctypes.byref(drop) if drop is not None else None
    if drop is None:
        L.check(L.lib.vtd_attention_train(qkv_d.data_ptr(), B, N, H, dkp, ld, float(scale),
                                          o_d.data_ptr(), ldo, lse_buf.data_ptr() + 64, code,
                                          L.stream_ptr()), "vtd_attention_train")
    else:
        L.check(L.lib.vtd_attention_train_dropout(
            qkv_d.data_ptr(), B, N, H, dkp, ld, float(scale), o_d.data_ptr(), ldo,
            lse_buf.data_ptr() + 64, code, L.stream_ptr(), dref), "vtd_attention_train_dropout")
    do_np = np.zeros((rows, inner + 8), np.float32)
    for h in range(H):
        do_np[:, h * dkp:h * dkp + dk] = do[:, :, h, :].reshape(rows, dk)
    do_d = torch.from_numpy(do_np).to(cuda)
    if not x3:
        do_d = do_d.to(torch.bfloat16)
    piece = 3 * inner + 8
    ldd = 2 * piece if x3 else piece
    n = L.c_size_t(0)
    L.check(L.lib.vtd_attention_backward_workspace_bytes(B, N, H, dkp, code, ctypes.byref(n)))
    raws, guards_ok = [], True
    for _ in range(2):
        dq_buf = _guarded(cuda, rows * ldd * 2, 2 * ldd * 2, 2 * ldd * 2)
        ws_buf = _guarded(cuda, n.value, 256, 256)
        args = (qkv_d.data_ptr(), o_d.data_ptr(), do_d.data_ptr(), lse_buf.data_ptr() + 64, B, N, H,
                dkp, ld, ldo, inner + 8, float(scale), dq_buf.data_ptr() + 2 * ldd * 2, ldd, code,
                ws_buf.data_ptr() + 256, n.value, L.stream_ptr())
        if drop is None:
            L.check(L.lib.vtd_attention_backward(*args), "vtd_attention_backward")
        else:
            L.check(L.lib.vtd_attention_backward_dropout(*args, dref),
                    "vtd_attention_backward_dropout")
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
    raw = raws[0]
    g = _bits_f64(raw[:, :3 * inner])
    if x3:
        g = g + _bits_f64(raw[:, piece:piece + 3 * inner])
    parts = [g[:, i * inner:(i + 1) * inner].reshape(B, N, H, dkp) for i in range(3)]
    o_raw = o_d.cpu().numpy().view(np.uint16)
    o = _bits_f64(o_raw[:, :inner])
    if x3:
        o = o + _bits_f64(o_raw[:, opiece:opiece + inner])
    # O's slack columns untouched
    for p0 in range(0, ldo, opiece):
        guards_ok &= bool((o_raw[:, p0 + inner:p0 + opiece] == 0xFFFF).all())
    return dict(o=o.reshape(B, N, H, dkp), o_raw=o_raw, raw=raw, lse_bits=lse_all[64:-64].copy(),
                dq=parts[0], dk=parts[1], dv=parts[2], guards_ok=guards_ok,
                repeat_ok=bool((raws[0] == raws[1]).all()),
                pads_zero=all(bool((p[..., dk:] == 0).all()) for p in parts + [o.reshape(B, N, H, dkp)]))


@pytest.fixture(scope="module")
def runs(L, cuda):
    """One device run per (shape, mode, rate), rate None = the existing entries; inputs shared."""
    cache = {}

    def get(shape, mode, rate):
        key = (shape, mode, rate)
        if key not in cache:
            B, H, N, dk = shape
            (q, k, v, do), scale = A.random_case(shape, mode)
            qkv = pack_qkv(*(t.astype(np.float32) for t in (q, k, v)), dkp_of(dk))
            drop = None if rate is None else _drop(L, rate)
            cache[key] = device_run(L, cuda, mode, qkv, do, B, N, H, dk, scale, drop)
        return cache[key]
    return get


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_random_attention_against_masked_float64(runs, shape, mode, rate):
    B, H, N, dk = shape
    run = runs(shape, mode, rate)
    (q, k, v, do), scale = A.random_case(shape, mode)
    mask = D.mask_attention(B, H, N, rate, SEED, STEP, SITE)
    c = D.inv_keep(rate)
    o64, _, _ = D.forward64(q, k, v, scale, mask, c)
    g64 = D.backward64(q, k, v, do, scale, mask, c)
    got = [run[n][..., :dk] for n in ("o", "dq", "dk", "dv")]
    assert all(np.isfinite(g).all() for g in got)
    if N > 1:
        errs = [A.rel_err(g, r) for g, r in zip(got, [o64] + list(g64))]
    else:
        # one key: P = 1, dS cancels completely (attention_grad_oracle.tensor_errors); a dropped
        # (b, h, i) has O, dV exactly zero and no denominator at all
        den = [np.abs(o64)] + list(D.magnitudes(q, k, v, do, scale, mask, c))
        errs = []
        for g, r, d_ in zip(got, [o64] + list(g64), den):
            errs.append(float(np.abs(g - r).max() / d_.max()) if d_.max() > 0
                        else float(np.abs(g).max()))
        dropped = ~mask[:, :, :, 0]                               # [B][H][N]
        assert (np.moveaxis(run["o"], 2, 1)[dropped] == 0).all()
    print(f"{shape} {mode} rate {rate}: O dQ dK dV errors {' '.join(f'{e:.3g}' for e in errs)} "
          f"(bar {A.BARS[mode]})")
    assert max(errs) <= A.BARS[mode]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_lse_bits_repeats_guards_and_pads(runs, shape, mode, rate):
    run, plain = runs(shape, mode, rate), runs(shape, mode, None)
    assert (run["lse_bits"] == plain["lse_bits"]).all()      # the undropped softmax's LSE
    assert run["repeat_ok"] and run["guards_ok"] and run["pads_zero"]
    if shape[2] > 1:
        assert not (run["o_raw"] == plain["o_raw"]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_rate_zero_is_the_existing_entries_bit_for_bit(runs, shape, mode):
    zero, plain = runs(shape, mode, 0.0), runs(shape, mode, None)
    assert (zero["o_raw"] == plain["o_raw"]).all() and (zero["raw"] == plain["raw"]).all()
    assert (zero["lse_bits"] == plain["lse_bits"]).all()


def _designed(L, cuda, mode, N, B=2, H=2, dk=32):
    """q = k = 0 (uniform P = 1 / N), v[j] = e_(j mod 32), rate 0.5:
    O[i][d] = (2 / N) sum_k m[i][d + 32 k] exactly -- the kernel's own mask read back."""
    dkp = 32
    z = np.zeros((B, N, H, dk), np.float32)
    v = np.zeros((B, N, H, dk), np.float32)
    for j in range(N):
        v[:, j, :, j % 32] = 1.0
    qkv = pack_qkv(z, z, v, dkp)
    run = device_run(L, cuda, mode, qkv, np.zeros((B, N, H, dk)), B, N, H, dk, 1.0 / np.sqrt(dk),
                     _drop(L, 0.5))
    mask = D.mask_attention(B, H, N, 0.5, SEED, STEP, SITE).astype(np.float64)    # [B][H][i][j]
    want = (2.0 / N) * mask.reshape(B, H, N, N // 32, 32).sum(axis=3)             # [B][H][i][d]
    return run, np.moveaxis(want, 1, 2)


@pytest.mark.parametrize("mode,N", [("x3", 64), ("bf16", 64), ("bf16", 256)])
def test_designed_forward_reads_the_kernels_mask_back(L, cuda, mode, N):
    run, want = _designed(L, cuda, mode, N)
    assert (run["o"] == want).all()
    assert run["guards_ok"]


def test_mask_does_not_depend_on_batch_or_padding(L, cuda):
    """Image 0 of a batch of two is the batch-of-one run, with other leading dimensions."""
    shape, mode = (2, 2, 77, 24), "x3"
    B, H, N, dk = shape
    (q, k, v, do), scale = A.random_case(shape, mode)
    two = device_run(L, cuda, mode, pack_qkv(*(t.astype(np.float32) for t in (q, k, v)), 32), do,
                     B, N, H, dk, scale, _drop(L, 0.5))
    qkv1 = pack_qkv(*(t[:1].astype(np.float32) for t in (q, k, v)), 32)
    qkv1 = np.ascontiguousarray(np.pad(qkv1, ((0, 0), (0, 24))))
    one = device_run(L, cuda, mode, qkv1, do[:1], 1, N, H, dk, scale, _drop(L, 0.5))
    assert (one["o"] == two["o"][:1]).all()
    for n in ("dq", "dk", "dv"):
        assert (one[n] == two[n][:1]).all(), n


@pytest.mark.parametrize("mode", MODES)
def test_attention_core_with_dropout(L, cuda, runs, mode):
    """The autograd op gives the C entries' bits; dropout None / 0 is the op without dropout; a
    rate without a seed raises; another step gives another result."""
    import vision_transformer_detector_amd as vtd
    shape = (2, 2, 77, 24)
    B, H, N, dk = shape
    dkp, inner = 32, H * 32
    (q, k, v, do), scale = A.random_case(shape, mode)
    tdt = torch.float32 if mode == "x3" else torch.bfloat16
    dtype = "bf16x3" if mode == "x3" else "bf16"
    qkv_np = pack_qkv(*(t.astype(np.float32) for t in (q, k, v)), dkp)[:, :3 * inner]
    base = torch.from_numpy(np.ascontiguousarray(qkv_np)).to(tdt).to(cuda).reshape(B, N, 3 * inner)
    g = np.zeros((B, N, H, dkp), np.float32)
    g[..., :dk] = do
    gt = torch.from_numpy(g).reshape(B, N, inner).to(tdt).to(cuda)

    def go(**kw):
        x = base.clone().requires_grad_(True)
        out = vtd.attention_core(x, H, dk, dtype=dtype, **kw)
        out.backward(gt)
        return out.detach(), x.grad

    out, grad = go(dropout=0.5, seed=SEED, step=STEP, site=SITE)
    run = runs(shape, mode, 0.5)
    assert (out.double().cpu().numpy().reshape(B, N, H, dkp) == run["o"].astype(np.float32)).all()
    gr = grad.double().cpu().numpy().reshape(B, N, 3, H, dkp)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert (gr[:, :, i] == run[name].astype(np.float32)).all(), name
    o_plain, g_plain = go()
    for kw in (dict(dropout=None, seed=None), dict(dropout=0.0, seed=None), dict(dropout=0, seed=4)):
        o2, g2 = go(**kw)
        assert torch.equal(o2, o_plain) and torch.equal(g2, g_plain)
    o3, _ = go(dropout=0.5, seed=SEED, step=STEP + 1, site=SITE)
    assert not torch.equal(o3, out)
    with pytest.raises(ValueError, match="seed"):
        vtd.attention_core(base, H, dk, dtype=dtype, dropout=0.5, seed=None)
    with pytest.raises(ValueError, match="rate"):
        vtd.attention_core(base, H, dk, dtype=dtype, dropout=1.0, seed=1)
