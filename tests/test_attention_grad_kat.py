"""The yardstick of the attention backward, no GPU: the float64 oracle
(tests/attention_grad_oracle.py) against central differences, the CPU emulation of each
mode's roundings against HALF of every bar tests/test_gpu_attention_backward.py holds the device
to -- on exactly the seeded inputs that test uses -- the new symbols, and every argument and
workspace check through ctypes, all of which must answer before any device call."""
import ctypes
import functools

import numpy as np
import pytest

from tests import attention_grad_oracle as A

NEW_SYMBOLS = ["vtd_attention_train", "vtd_attention_backward",
               "vtd_attention_backward_workspace_bytes"]


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def test_oracle_gradients_match_central_differences():
    """float64, step 1e-6, 8 seeded coordinates of q, k and v at (2, 2, 9, 5): within 1e-7 of
    the tensor's largest |gradient|."""
    rng = np.random.default_rng(3)
    q, k, v, do = (rng.normal(0, 1.0, size=(2, 9, 2, 5)) for _ in range(4))
    scale = 5 ** -0.5
    grads = A.backward64(q, k, v, do, scale)
    worst = 0.0
    for which, g in enumerate(grads):
        for _ in range(8):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1.0, -1.0):
                t = [q.copy(), k.copy(), v.copy()]
                t[which][idx] += sign * 1e-6
                vals.append(float((A.forward64(*t, scale)[0] * do).sum()))
            worst = max(worst, abs((vals[0] - vals[1]) / 2e-6 - g[idx]) / np.abs(g).max())
    print(f"worst finite-difference error / tensor maximum {worst:.3g}")
    assert worst <= 1e-7


def test_oracle_lse_and_rows():
    (q, k, v, do), scale = A.random_case((2, 2, 31, 24), "x3")
    o, lse, p = A.forward64(q, k, v, scale)
    assert np.allclose(p.sum(axis=-1), 1.0, atol=1e-13)
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * scale
    assert np.allclose(np.exp(s - lse[..., None]), p, atol=1e-13)


@pytest.mark.parametrize("mode", ["x3", "bf16"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_random_is_under_half_the_bars(shape, mode):
    """The roundings alone, on the GPU test's own inputs: at most half of the per-tensor bar
    (2e-4 / 5e-2) and of the lse tolerance (2e-5 / 2e-2)."""
    (q, k, v, do), scale = A.random_case(shape, mode)
    _, lse64, _ = A.forward64(q, k, v, scale)
    e = A.emulate(q, k, v, do, scale, mode)
    worst = max(A.tensor_errors([e["dq"], e["dk"], e["dv"]], q, k, v, do, scale))
    lse_err = np.abs(e["lse"] - lse64).max() / max(1.0, np.abs(lse64).max())
    print(f"{shape} {mode} sigma {A.SIGMA[shape]}: emulated worst {worst:.3g}, lse {lse_err:.3g}")
    assert worst <= 0.5 * A.BARS[mode]
    assert lse_err <= 0.5 * A.LSE_TOL[mode]


@functools.lru_cache(maxsize=None)
def _patterns():
    from tests import test_gpu_attention_patterns as P
    return P


@pytest.mark.parametrize("mode", ["x3", "bf16"])
@pytest.mark.parametrize("N,dk", A.DESIGNED_SHAPES)
@pytest.mark.parametrize("pattern", A.DESIGNED_PATTERNS)
def test_emulated_designed_is_under_half_the_bars(pattern, N, dk, mode):
    """Componentwise |g - g64| <= c den with c = 2^-15 / 2^-7: the emulation stays under c / 2."""
    P = _patterns()
    qkv, _, _, _ = P.make_case(pattern, N, dk)
    q, k, v = A.unpack_qkv(qkv, P.B, N, P.H, dk)
    do = A.designed_do(pattern, N, dk)
    scale = float(P.LN2_F32)
    g64 = A.backward64(q, k, v, do, scale)
    den = A.magnitudes(q, k, v, do, scale)
    e = A.emulate(q, k, v, do, scale, mode)
    worst = 0.0
    for n, g, d in zip(("dq", "dk", "dv"), g64, den):
        err = np.abs(e[n] - g)
        assert (err[d == 0] == 0).all()
        worst = max(worst, float((err[d > 0] / d[d > 0]).max()))
    print(f"{pattern} N {N} dk {dk} {mode}: emulated worst ratio {worst:.3g}")
    assert worst <= 0.5 * A.C_DESIGNED[mode]


def test_new_symbols_and_abi(L):
    assert L.lib.vtd_abi_version() == 17 == L.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    import vision_transformer_detector_amd as vtd
    assert callable(vtd.attention_core) and "attention_core" in vtd.__all__


# ---- argument checks: fake device addresses, never dereferenced
QKV, O, DO, LSE, DQKV, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def bwd(L, qkv=QKV, o=O, do=DO, lse=LSE, B=2, N=40, heads=2, dkp=64, ldqkv=384, ldo=128,
        lddo=128, scale=0.125, dqkv=DQKV, lddqkv=384, dtype=1, ws=WS, ws_bytes=1 << 20):
    return L.lib.vtd_attention_backward(qkv, o, do, lse, B, N, heads, dkp, ldqkv, ldo, lddo, scale,
                                        dqkv, lddqkv, dtype, ws, ws_bytes, None)


def train(L, qkv=QKV, B=2, N=40, heads=2, dkp=64, ldqkv=384, scale=0.125, o=O, ldo=128, lse=LSE,
          dtype=1):
    return L.lib.vtd_attention_train(qkv, B, N, heads, dkp, ldqkv, scale, o, ldo, lse, dtype, None)


def test_backward_argument_errors(L):
    for name in ("qkv", "o", "do", "lse", "dqkv", "ws"):
        assert bwd(L, **{name: None}) == -1
    assert bwd(L, B=0) == -1 and bwd(L, N=0) == -1 and bwd(L, heads=-1) == -1
    assert bwd(L, dkp=48) == -1 and bwd(L, dkp=0) == -1 and bwd(L, dkp=256) == -1
    for scale in (0.0, -0.125, float("inf"), float("nan")):
        assert bwd(L, scale=scale) == -1
    assert bwd(L, ldqkv=376) == -1                      # < 3 heads dkp
    assert bwd(L, ldqkv=388) == -1                      # % 8
    assert bwd(L, lddo=120) == -1 and bwd(L, lddo=132) == -1
    assert bwd(L, ldo=120) == -1 and bwd(L, ldo=132) == -1
    assert bwd(L, lddqkv=376) == -1 and bwd(L, lddqkv=388) == -1
    assert bwd(L, qkv=QKV + 2) == -1 and bwd(L, dqkv=DQKV + 8) == -1 and bwd(L, do=DO + 4) == -1
    # VTD_BF16X3: split O and dqkv, piece width ld / 2, ld % 16
    x3 = dict(dtype=3, ldo=256, lddqkv=768)
    assert bwd(L, **{**x3, "ldo": 128}) == -1           # piece 64 < heads dkp
    assert bwd(L, **{**x3, "ldo": 264}) == -1           # % 16
    assert bwd(L, **{**x3, "lddqkv": 384}) == -1
    assert bwd(L, **{**x3, "lddqkv": 776}) == -1
    assert bwd(L, dtype=0) == -2 and bwd(L, dtype=2) == -2 and bwd(L, dtype=7) == -2
    # the workspace: delta, fp32 [B][heads][N]; VTD_BF16X3 also the row sums' reciprocals
    n = ctypes.c_size_t(0)
    for dtype, planes in ((1, 1), (3, 2)):
        assert L.lib.vtd_attention_backward_workspace_bytes(2, 40, 2, 64, dtype, ctypes.byref(n)) == 0
        assert n.value == planes * 2 * 2 * 40 * 4
        mode = x3 if dtype == 3 else {}
        assert bwd(L, **mode, ws_bytes=n.value - 1) == -4
        assert b"workspace" in L.lib.vtd_last_error()
    assert L.lib.vtd_attention_backward_workspace_bytes(2, 40, 2, 64, 1, None) == -1
    assert L.lib.vtd_attention_backward_workspace_bytes(2, 0, 2, 64, 1, ctypes.byref(n)) == -1
    assert L.lib.vtd_attention_backward_workspace_bytes(2, 40, 2, 48, 1, ctypes.byref(n)) == -1
    assert L.lib.vtd_attention_backward_workspace_bytes(2, 40, 2, 64, 0, ctypes.byref(n)) == -2


def test_train_argument_errors(L):
    assert train(L, qkv=None) == -1 and train(L, o=None) == -1 and train(L, lse=None) == -1
    assert train(L, B=0) == -1 and train(L, N=-1) == -1 and train(L, heads=0) == -1
    assert train(L, dkp=48) == -1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert train(L, scale=scale) == -1
    assert train(L, ldqkv=376) == -1 and train(L, ldqkv=388) == -1
    assert train(L, ldo=120) == -1 and train(L, ldo=132) == -1
    assert train(L, dtype=3, ldo=255) == -1 and train(L, dtype=3, ldo=128) == -1
    assert train(L, dtype=0) == -2 and train(L, dtype=2) == -2
