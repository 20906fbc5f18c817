"""The yardstick of the encoder block backward, no GPU: the float64 block oracle
(tests/block_grad_oracle.py) against central differences, the CPU emulation of the device's
roundings against half the bars the GPU test holds the device to, the new symbols, every
argument check of the two new entries through ctypes -- all of which must answer before any
device call -- and the workspace size."""
import ctypes

import numpy as np
import pytest
import torch

from tests import block_grad_oracle as K

NEW_SYMBOLS = ["vtd_encoder_block_backward", "vtd_encoder_block_backward_workspace_bytes"]
FD_CASES = [K.CASES[0], (2, 5, 8, 2, 4, 2, False)]


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.mark.parametrize("case", FD_CASES, ids=K.case_id)
def test_oracle_gradients_match_central_differences(case):
    """float64, step 1e-6, 6 seeded coordinates of every tensor: within 1e-6 of the tensor's
    largest |gradient| (key/bias, whose gradient is identically zero: of the magnitude
    block_grad_oracle._denominators gives it)."""
    use_mish = case[6]
    w = K.seeded_weights(case)
    x, dy = K.seeded_inputs(case)
    _, grads, dx, den = K.block_grads(w, x, dy, use_mish)
    dyt = torch.tensor(dy, dtype=torch.float64)

    def value(ws, xt):
        return float((K.block_forward(ws, xt, use_mish) * dyt).sum())

    rng = np.random.default_rng(7)
    h = 1e-6
    worst = 0.0
    for i, g in enumerate(grads + [dx]):
        top = den[i]
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1.0, -1.0):
                ws = [torch.tensor(t, dtype=torch.float64) for t in w]
                xt = torch.tensor(x, dtype=torch.float64)
                target = xt if i == len(grads) else ws[i]
                target[idx] += sign * h
                vals.append(value(ws, xt))
            fd = (vals[0] - vals[1]) / (2 * h)
            worst = max(worst, abs(fd - g[idx]) / top)
    print(f"{K.case_id(case)}: worst finite-difference error / tensor maximum {worst:.3g}")
    assert worst <= 1e-6


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_emulated_backward_is_under_half_the_bars(case, mode):
    """The device's chain of roundings emulated on the CPU stays at or under half the bar of
    tests/test_gpu_encoder_block.py for every tensor (2e-4 bf16x3, 5e-2 bfloat16)."""
    B, N, d, heads, dk, q, use_mish = case
    w = K.seeded_weights(case)
    x, dy = K.seeded_inputs(case)
    y64, g64, dx64, den = K.block_grads(w, x, dy, use_mish)
    y, g, dx = K.emulated_block_backward(w, x, dy, heads, dk, use_mish, mode)
    errs = K.rel_errors(g, dx, g64, dx64, den, q)
    top = max(errs, key=errs.get)
    print(f"{K.case_id(case)} {mode}: emulation worst {errs[top]:.3g} ({top}); "
          + ", ".join(f"{n} {v:.2g}" for n, v in errs.items()))
    assert [t.shape for t in g] == [t.shape for t in g64] and dx.shape == dx64.shape
    assert errs[top] <= 0.5 * K.BARS[mode], f"{top}: {errs[top]:.3g} > half of {K.BARS[mode]}"


def test_new_symbols_and_abi(L):
    assert L.lib.vtd_abi_version() == 17 == L.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    import vision_transformer_detector_amd as m
    assert callable(m.encoder_block) and hasattr(m.Model, "encoder_block_weights")


# ---- argument checks: fake device addresses, never dereferenced
X, DY, Y, W, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000


def dims(L, **change):
    kw = dict(batch=3, tokens=25, d=24, num_heads=3, key_dim=10, mlp_quantities=3, use_mish=1,
              dtype=3)
    kw.update(change)
    return L.VtdBlockDims(**kw)


def structs(L, q=3):
    P, G = L.VtdBlockParams(), L.VtdBlockGrads()
    for S in (P, G):
        for n, _ in L.VtdBlockParams._fields_[:12]:
            setattr(S, n, W)
        for j in range(q):
            S.w_mlp[j] = S.b_mlp[j] = W
    G.dx = W
    return P, G


def ws_bytes(L, d):
    n = ctypes.c_size_t(0)
    return L.lib.vtd_encoder_block_backward_workspace_bytes(ctypes.byref(d), ctypes.byref(n)), n.value


def test_workspace_bytes_argument_errors(L):
    rc, need = ws_bytes(L, dims(L))
    assert rc == 0 and need > 0
    rc, bf16 = ws_bytes(L, dims(L, dtype=1))
    assert rc == 0 and 0 < bf16 < need
    f = L.lib.vtd_encoder_block_backward_workspace_bytes
    n = ctypes.c_size_t()
    assert f(None, ctypes.byref(n)) == -1
    assert f(ctypes.byref(dims(L)), None) == -1
    for field in ("batch", "tokens", "d", "num_heads", "key_dim", "mlp_quantities"):
        assert ws_bytes(L, dims(L, **{field: 0}))[0] == -1, field
        assert ws_bytes(L, dims(L, **{field: -2}))[0] == -1, field
    assert ws_bytes(L, dims(L, mlp_quantities=L.MAX_MLP + 1))[0] == -1
    assert ws_bytes(L, dims(L, mlp_quantities=L.MAX_MLP))[0] == 0
    assert ws_bytes(L, dims(L, key_dim=129))[0] == -1
    assert ws_bytes(L, dims(L, key_dim=128))[0] == 0
    assert ws_bytes(L, dims(L, batch=1 << 16, tokens=1 << 15))[0] == -1       # rows = 2^31
    assert b"too large" in L.lib.vtd_last_error()
    assert ws_bytes(L, dims(L, batch=(1 << 16) - 1, tokens=1 << 15))[0] == 0
    assert ws_bytes(L, dims(L, d=1 << 22, mlp_quantities=3))[0] == -1         # width 2^24
    for dtype in (0, 2, 4, -1):
        assert ws_bytes(L, dims(L, dtype=dtype))[0] == -2
        assert b"VTD_BF16X3" in L.lib.vtd_last_error()


def test_block_backward_argument_errors(L):
    d = dims(L)
    _, need = ws_bytes(L, d)
    P, G = structs(L)
    f = L.lib.vtd_encoder_block_backward
    ok = (ctypes.byref(d), ctypes.byref(P), X, DY, Y, ctypes.byref(G), WS, need, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return f(*args)
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a2=None) == -1
    assert call(a5=None) == -1 and call(a6=None) == -1
    assert call(a3=None, a4=None) == -1             # no dy and no y: nothing to do
    assert call(a7=need - 1) == -4
    assert str(need).encode() in L.lib.vtd_last_error()
    assert call(a7=0) == -4
    for field in ("batch", "tokens", "d", "num_heads", "key_dim", "mlp_quantities"):
        assert call(a0=ctypes.byref(dims(L, **{field: 0}))) == -1, field
    assert call(a0=ctypes.byref(dims(L, mlp_quantities=L.MAX_MLP + 1))) == -1
    assert call(a0=ctypes.byref(dims(L, key_dim=129))) == -1
    assert call(a0=ctypes.byref(dims(L, batch=1 << 16, tokens=1 << 15))) == -1
    for dtype in (0, 2):
        assert call(a0=ctypes.byref(dims(L, dtype=dtype))) == -2
    for n, _ in L.VtdBlockParams._fields_[:12]:
        P2, G2 = structs(L)
        setattr(P2, n, None)
        assert call(a1=ctypes.byref(P2)) == -1, n
        assert b"weight" in L.lib.vtd_last_error()
        setattr(G2, n, None)
        assert call(a5=ctypes.byref(G2)) == -1, n
        assert b"gradient" in L.lib.vtd_last_error()
    for arr in ("w_mlp", "b_mlp"):
        P2, G2 = structs(L)
        getattr(P2, arr)[2] = None
        getattr(G2, arr)[1] = None
        assert call(a1=ctypes.byref(P2)) == -1 and call(a5=ctypes.byref(G2)) == -1


def test_workspace_is_monotone_in_batch_and_granular(L):
    for shape in (dict(tokens=25, d=24, num_heads=3, key_dim=10, mlp_quantities=3),
                  dict(tokens=196, d=768, num_heads=12, key_dim=64, mlp_quantities=3),
                  dict(tokens=1, d=768, num_heads=12, key_dim=64, mlp_quantities=2)):
        for dtype in (3, 1):
            prev = 0
            for batch in list(range(1, 40)) + [48, 64, 96, 128, 192, 256, 300, 512, 1024, 4096]:
                rc, n = ws_bytes(L, dims(L, batch=batch, dtype=dtype, **shape))
                assert rc == 0 and n % 256 == 0
                assert n >= prev, (shape, dtype, batch, n, prev)
                prev = n
