"""The yardstick of the whole-model gradients, no GPU: the float64 oracle of the stem and of the
whole model (tests/model_grad_oracle.py) against central differences, the CPU emulation of the
device's whole chain of roundings against half the bars the GPU test holds the device to, the
new symbols, every argument check of the two new entries through ctypes -- all of which must
answer before any device call -- the workspace size, and the ValueErrors of patch_embedding that
need no device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import model_grad_oracle as M

NEW_SYMBOLS = ["vtd_stem_backward", "vtd_stem_backward_workspace_bytes"]


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def test_stem_oracle_matches_central_differences():
    """float64, step 1e-6, 6 seeded coordinates of each of the three tensors at tiny_mish's
    stem: within 1e-6 of the tensor's largest |gradient|."""
    case = M.STEM_CASES[0]
    images, sw, dx0 = M.seeded_stem(case)
    p = case[3]
    _, grads = M.stem_grads(sw, images, p, dx0)
    pt = torch.tensor(M.patches_of(images, p))
    r = torch.tensor(dx0, dtype=torch.float64)
    rng = np.random.default_rng(7)
    h, worst = 1e-6, 0.0
    for i, g in enumerate(grads):
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1.0, -1.0):
                t = [torch.tensor(a, dtype=torch.float64) for a in sw]
                t[i][idx] += sign * h
                vals.append(float((M.stem_forward(t, pt) * r).sum()))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g[idx]) / np.abs(g).max())
    print(f"stem: worst finite-difference error / tensor maximum {worst:.3g}")
    assert worst <= 1e-6


def test_model_oracle_matches_central_differences():
    """The whole model at tiny_mish with the smooth stand-in loss sum(logits * r): float64, step
    1e-6, 6 seeded coordinates of every weight tensor, within 1e-6 of the tensor's denominator
    (max |gradient|; key/bias, whose gradient is identically zero: model_grads' magnitude)."""
    kw, w, x, r = M.load_case("tiny_mish", 2)
    _, grads, dxs, den = M.model_grads(kw, w, x, r)
    assert list(grads) == list(V.weight_shapes(**kw)) and len(dxs) == 3
    pt = torch.tensor(M.patches_of(x, kw["patch_size"]))
    rt = torch.tensor(r, dtype=torch.float64)
    rng = np.random.default_rng(7)
    h, worst = 1e-6, 0.0
    for n, g in grads.items():
        assert g.shape == np.asarray(w[n]).shape
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1.0, -1.0):
                wt = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
                wt[n][idx] += sign * h
                vals.append(float((M.model_forward(kw, wt, pt) * rt).sum()))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g[idx]) / den[n])
    print(f"tiny_mish: worst finite-difference error / tensor denominator {worst:.3g}")
    assert worst <= 1e-6


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c[0])
def test_emulated_chain_is_under_half_the_bars(case, mode):
    """The device's whole chain of roundings emulated on the CPU stays at or under half the bar
    of every tensor: the project's (2e-4 bf16x3, 5e-2 bfloat16), or the tensor's own from
    model_grad_oracle.OWN_BARS."""
    kw, w, x, dl = M.load_case(*case)
    logits64, g64, _, den = M.model_grads(kw, w, x, dl)
    logits, g = M.emulated_model_backward(kw, w, x, dl, mode)
    assert list(g) == list(g64) and all(g[n].shape == g64[n].shape for n in g64)
    errs = M.rel_errors(g, g64, den)
    top = max(errs, key=errs.get)
    own = {n: f"{errs[n]:.3g}" for n in M.OWN_BARS[mode] if n in errs}
    print(f"{case[0]} {mode}: emulation worst {errs[top]:.3g} ({top}); own bars: {own}")
    for n, v in errs.items():
        assert v <= 0.5 * M.bar(mode, n), f"{n}: {v:.3g} > half of {M.bar(mode, n)}"
    tol = {"bf16x3": 1e-4, "bfloat16": 3e-2}[mode]
    assert np.all(np.abs(logits - logits64) <= tol * np.abs(logits64) + tol * np.abs(logits64).max())


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("case", M.STEM_CASES, ids=M.stem_case_id)
def test_emulated_stem_is_under_half_the_bars(case, mode):
    """The stem alone at the cases of tests/test_gpu_stem_backward.py: the emulated dW and db
    under half the project's bars, the emulated x0 within the forward tolerance."""
    images, sw, dx0 = M.seeded_stem(case)
    x64, g64 = M.stem_grads(sw, images, case[3], dx0)
    g = M.emulated_stem_backward(images, case[3], dx0, mode)
    errs = [float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(g, g64)]
    print(f"{M.stem_case_id(case)} {mode}: dpos {errs[0]:.3g}, dW {errs[1]:.3g}, db {errs[2]:.3g}")
    assert max(errs[1:]) <= 0.5 * M.BARS[mode]
    x0 = M.emulated_stem_forward(sw, images, case[3], mode)
    tol = {"bf16x3": 1e-4, "bfloat16": 3e-2}[mode]
    assert np.all(np.abs(x0 - x64) <= tol * np.abs(x64) + tol * np.abs(x64).max())
    # dpos: the bound the GPU test holds the device to also holds the float32 emulation
    c = M.dpos_roundings(case[0], case[4])
    bound = c * 2.0 ** -24 * np.abs(dx0.astype(np.float64)).sum(axis=(0, 2))
    assert np.all(np.abs(g[0].astype(np.float64) - g64[0])[:, 0] <= bound)


def test_new_symbols_and_abi(L):
    assert L.lib.vtd_abi_version() == 17 == L.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    import vision_transformer_detector_amd as m
    assert callable(m.patch_embedding) and "patch_embedding" in m.__all__
    assert hasattr(m.Model, "stem_weights") and hasattr(m.Model, "gradients")


# ---- argument checks: fake device addresses, never dereferenced
IMG, DX, X0, W, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000


def dims(L, **change):
    kw = dict(batch=3, H=40, W=36, C=3, patch=8, d=24, dtype=3)
    kw.update(change)
    return L.VtdStemDims(**kw)


def structs(L):
    P, G = L.VtdStemParams(), L.VtdStemParams()
    for S in (P, G):
        S.pos = S.w = S.b = W
    return P, G


def ws_bytes(L, d):
    n = ctypes.c_size_t(0)
    return L.lib.vtd_stem_backward_workspace_bytes(ctypes.byref(d), ctypes.byref(n)), n.value


def test_workspace_bytes_argument_errors(L):
    rc, need = ws_bytes(L, dims(L))
    assert rc == 0 and need > 0
    rc, bf16 = ws_bytes(L, dims(L, dtype=1))
    assert rc == 0 and 0 < bf16 < need
    f = L.lib.vtd_stem_backward_workspace_bytes
    n = ctypes.c_size_t()
    assert f(None, ctypes.byref(n)) == -1
    assert f(ctypes.byref(dims(L)), None) == -1
    for field in ("batch", "H", "W", "C", "patch", "d"):
        assert ws_bytes(L, dims(L, **{field: 0}))[0] == -1, field
        assert ws_bytes(L, dims(L, **{field: -2}))[0] == -1, field
    big = dict(H=256, W=128, patch=1)                                     # 2^15 tokens
    assert ws_bytes(L, dims(L, batch=1 << 16, **big))[0] == -1            # rows = 2^31
    assert b"too large" in L.lib.vtd_last_error()
    assert ws_bytes(L, dims(L, batch=(1 << 16) - 1, **big))[0] == 0
    assert ws_bytes(L, dims(L, d=1 << 24))[0] == -1
    assert ws_bytes(L, dims(L, patch=4096, C=1))[0] == -1                 # patch_dim 2^24
    for dtype in (0, 2, 4, -1):
        assert ws_bytes(L, dims(L, dtype=dtype))[0] == -2
        assert b"VTD_BF16X3" in L.lib.vtd_last_error()


def test_stem_backward_argument_errors(L):
    d = dims(L)
    _, need = ws_bytes(L, d)
    P, G = structs(L)
    f = L.lib.vtd_stem_backward
    ok = (ctypes.byref(d), ctypes.byref(P), IMG, DX, X0, ctypes.byref(G), WS, need, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return f(*args)
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a2=None) == -1
    assert call(a5=None) == -1 and call(a6=None) == -1
    assert b"null pointer" in L.lib.vtd_last_error()
    assert call(a3=None, a4=None) == -1             # no dx0 and no x0: nothing to do
    assert call(a7=need - 1) == -4
    assert str(need).encode() in L.lib.vtd_last_error()
    assert call(a7=0) == -4
    assert call(a3=None, a5=None, a7=0) == -4       # forward only: grads ignored
    for field in ("batch", "H", "W", "C", "patch", "d"):
        assert call(a0=ctypes.byref(dims(L, **{field: 0}))) == -1, field
    assert call(a0=ctypes.byref(dims(L, batch=1 << 16, H=256, W=128, patch=1))) == -1
    for dtype in (0, 2):
        assert call(a0=ctypes.byref(dims(L, dtype=dtype))) == -2
    for n in ("pos", "w", "b"):
        P2, G2 = structs(L)
        setattr(P2, n, None)
        assert call(a1=ctypes.byref(P2)) == -1, n
        assert b"weight" in L.lib.vtd_last_error()
        setattr(G2, n, None)
        assert call(a5=ctypes.byref(G2)) == -1, n
        assert b"gradient" in L.lib.vtd_last_error()
        assert call(a3=None, a5=ctypes.byref(G2), a7=0) == -4         # not looked at without dx0
    # misaligned bases
    for change in (dict(a6=WS + 8), dict(a4=X0 + 4), dict(a2=IMG + 2), dict(a3=DX + 1)):
        assert call(**change) == -1, change
        assert b"misaligned" in L.lib.vtd_last_error()
    assert call(a3=DX + 4, a7=0) == -4              # dx0 off a 16-B boundary: the generic path
    for n, off in (("w", 4), ("b", 8), ("pos", 2)):
        P2, G2 = structs(L)
        setattr(P2, n, W + off)
        assert call(a1=ctypes.byref(P2)) == -1, n
        setattr(G2, n, W + 2)
        assert call(a5=ctypes.byref(G2)) == -1, n


def test_workspace_is_monotone_in_batch_and_granular(L):
    for shape in (dict(H=40, W=36, patch=8, d=24), dict(H=224, W=224, patch=16, d=768),
                  dict(H=33, W=50, patch=7, d=6)):
        for dtype in (3, 1):
            prev = 0
            for batch in list(range(1, 40)) + [48, 64, 96, 128, 192, 256, 300, 512, 1024, 4096]:
                rc, n = ws_bytes(L, dims(L, batch=batch, dtype=dtype, **shape))
                assert rc == 0 and n % 256 == 0
                assert n >= prev, (shape, dtype, batch, n, prev)
                prev = n


def test_patch_embedding_value_errors_without_a_device():
    import vision_transformer_detector_amd as m
    img = torch.zeros((2, 40, 36, 3))
    ws = [torch.zeros((25, 1)), torch.zeros((192, 24)), torch.zeros((24,))]
    for dtype in ("float32", "float8"):
        with pytest.raises(ValueError, match="patch_embedding: dtype .* no backward"):
            m.patch_embedding(img, ws, patch_size=8, dtype=dtype)
    with pytest.raises(ValueError, match="unsupported dtype"):
        m.patch_embedding(img, ws, patch_size=8, dtype="int8")
    with pytest.raises(ValueError, match="weights must hold 3 tensors.*got 2"):
        m.patch_embedding(img, ws[:2], patch_size=8)
    with pytest.raises(ValueError, match="weights must hold 3 tensors.*got 4"):
        m.patch_embedding(img, dict(a=ws[0], b=ws[1], c=ws[2], d=ws[2]), patch_size=8)
    with pytest.raises(ValueError, match="patch_size must be positive"):
        m.patch_embedding(img, ws, patch_size=0)
    with pytest.raises(ValueError, match="images must be a device tensor"):
        m.patch_embedding(img, ws, patch_size=8)
    with pytest.raises(ValueError, match="images must be a device tensor"):
        m.patch_embedding(img.numpy(), ws, patch_size=8)
