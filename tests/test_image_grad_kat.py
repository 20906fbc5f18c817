"""The yardstick of the image gradient, no GPU: the float64 oracle of tests/image_grad_oracle.py
against central differences (the stem alone, and tiny_mish end to end), the adjoint identity of
its un-patch, the CPU emulation of the device's roundings against half the bars the GPU tests
hold the device to -- at every case those tests run --, the new symbols, every argument check of
the two new entries through ctypes, all of which must answer before any device call, the
workspace size, and vtd_stem_backward's recorded workspace sizes."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import image_grad_oracle as G
from tests import model_grad_oracle as M

NEW_SYMBOLS = ["vtd_stem_image_grad", "vtd_stem_image_grad_workspace_bytes"]
MODES = ["bf16x3", "bfloat16"]


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


# ---- the float64 oracle
@pytest.mark.parametrize("case", [G.STEM_CASES[1], G.STEM_CASES[8], G.STEM_CASES[9]],
                         ids=G.stem_case_id)
def test_stem_oracle_matches_central_differences(case):
    """float64, step 1e-6, 12 seeded image coordinates, the loss sum(x0 * dx0): within 1e-6 of
    the largest |gradient| (the stem is linear in the images: only rounding is left)."""
    B, Hh, Ww, p, d, C = G.parse(case)
    w, dx0 = G.seeded(case)
    rng = np.random.default_rng(5)
    images = rng.uniform(0.0, 1.0, (B, Hh, Ww, C))
    g64 = G.stem_image_grad64(w, dx0, (Hh, Ww, C), p)
    assert g64.shape == images.shape

    def loss(x):
        return float((V.extract_patches_same(x, p) @ w.astype(np.float64) * dx0).sum())
    h, worst = 1e-6, 0.0
    for _ in range(12):
        idx = tuple(int(rng.integers(0, s)) for s in images.shape)
        vals = []
        for sign in (1.0, -1.0):
            x = images.copy()
            x[idx] += sign * h
            vals.append(loss(x))
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g64[idx]) / np.abs(g64).max())
    print(f"{G.stem_case_id(case)}: worst finite-difference error / maximum {worst:.3g}")
    assert worst <= 1e-6


def test_model_oracle_matches_central_differences():
    """tiny_mish end to end with the smooth stand-in loss sum(logits * r): float64, step 1e-6,
    12 seeded image coordinates, within 1e-6 of the largest |gradient|."""
    kw, w, x, r = M.load_case("tiny_mish", 2)
    _, g64, dx0 = G.model_image_grad64(kw, w, x, r)
    assert g64.shape == x.shape and dx0.shape[:2] == (2, 25)
    rng = np.random.default_rng(7)
    h, worst = 1e-6, 0.0
    for _ in range(12):
        idx = tuple(int(rng.integers(0, s)) for s in x.shape)
        vals = []
        for sign in (1.0, -1.0):
            xp = np.asarray(x, np.float64).copy()
            xp[idx] += sign * h
            vals.append(float((G.model_forward64(kw, w, xp) * r).sum()))
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g64[idx]) / np.abs(g64).max())
    print(f"tiny_mish: worst finite-difference error / maximum {worst:.3g}")
    assert worst <= 1e-6


@pytest.mark.parametrize("case", G.STEM_CASES, ids=G.stem_case_id)
def test_unpatch_is_the_adjoint_of_the_extraction(case):
    """<extract(u), v> == <u, unpatch(v)> on random u, v in float64, to rounding; every image
    element has exactly one source (unpatch asserts it) and the pads have none."""
    B, Hh, Ww, p, d, C = G.parse(case)
    rng = np.random.default_rng([Hh, Ww, p, C])
    u = rng.standard_normal((B, Hh, Ww, C))
    pu = V.extract_patches_same(u, p)
    v = rng.standard_normal(pu.shape)
    lhs, rhs = float((pu * v).sum()), float((u * G.unpatch(v, (Hh, Ww, C), p)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(np.abs(pu * v).sum())
    idx = G.source_index((Hh, Ww, C), p)
    gh, gw = V.token_grid(Hh, Ww, p)
    assert int((idx == 0).sum()) == gh * gw * p * p * C - Hh * Ww * C


# ---- the emulation fixes the bars
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", G.STEM_CASES, ids=G.stem_case_id)
def test_emulated_stem_is_under_half_the_bar(case, mode):
    B, Hh, Ww, p, d, C = G.parse(case)
    w, dx0 = G.seeded(case)
    g64 = G.stem_image_grad64(w, dx0, (Hh, Ww, C), p)
    g = G.emulated_stem_image_grad(w, dx0, (Hh, Ww, C), p, mode)
    assert g.shape == g64.shape and g.dtype == np.float32
    err = G.rel_err(g, g64)
    print(f"{G.stem_case_id(case)} {mode}: emulation {err:.3g}")
    assert err <= 0.5 * G.bar(mode, G.stem_case_id(case))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", G.MODEL_CASES, ids=lambda c: c[0])
def test_emulated_model_is_under_half_the_bar(case, mode):
    kw, w, x, dl = M.load_case(*case)
    _, g64, _ = G.model_image_grad64(kw, w, x, dl)
    g = G.emulated_model_image_grad(kw, w, x, dl, mode)
    err = G.rel_err(g, g64)
    print(f"{case[0]} {mode}: emulation {err:.3g}")
    assert err <= 0.5 * G.bar(mode, case[0])


def test_own_bars_follow_the_rule():
    """An own bar exists only above the project's, for a known case."""
    ids = [G.stem_case_id(c) for c in G.STEM_CASES] + [c[0] for c in G.MODEL_CASES]
    for mode in MODES:
        for name, v in G.OWN_BARS[mode].items():
            assert name in ids and v > G.BARS[mode]


# ---- symbols
def test_new_symbols_and_abi(L):
    assert L.lib.vtd_abi_version() == 17 == L.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    import inspect

    import vision_transformer_detector_amd as m
    from vision_transformer_detector_amd import stem
    assert callable(stem.image_grad) and callable(stem.image_grad_workspace_bytes)
    assert inspect.signature(m.patch_embedding).parameters["image_gradient"].default is False
    assert inspect.signature(m.Model.gradients).parameters["image_gradient"].default is False
    assert callable(m.Model.image_gradient)


# ---- argument checks: fake device addresses, never dereferenced
W, DX, IMG, WS = 0x40000, 0x20000, 0x10000, 0x100000


def dims(L, **change):
    kw = dict(batch=3, H=40, W=36, C=3, patch=8, d=24, dtype=3)
    kw.update(change)
    return L.VtdStemDims(**kw)


def ws_bytes(L, d):
    n = ctypes.c_size_t(0)
    return L.lib.vtd_stem_image_grad_workspace_bytes(ctypes.byref(d), ctypes.byref(n)), n.value


def test_workspace_bytes_argument_errors(L):
    rc, need = ws_bytes(L, dims(L))
    assert rc == 0 and need > 0
    rc, bf16 = ws_bytes(L, dims(L, dtype=1))
    assert rc == 0 and 0 < bf16 < need
    f = L.lib.vtd_stem_image_grad_workspace_bytes
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


def test_workspace_layout(L):
    """The plan as the header describes it: dx0 in operand form, the row-sum scratch, the
    kernel as stored, fp32 dP -- each rounded up to 256 bytes."""
    def up(n, m):
        return -(-n // m) * m
    for case in G.STEM_CASES:
        B, Hh, Ww, p, d, C = G.parse(case)
        gh, gw = V.token_grid(Hh, Ww, p)
        R, Pp, Dp = B * gh * gw, up(p * p * C, 64), up(d, 64)
        for dtype, eop, kk in ((3, 4, 3), (1, 2, 1)):
            want = (up(R * Dp * eop, 256) + up(R * 4, 256) + up(Pp * kk * Dp * 2, 256)
                    + up(R * Pp * 4, 256))
            assert ws_bytes(L, dims(L, batch=B, H=Hh, W=Ww, C=C, patch=p, d=d,
                                    dtype=dtype)) == (0, want), case


def test_stem_image_grad_argument_errors(L):
    d = dims(L)
    _, need = ws_bytes(L, d)
    f = L.lib.vtd_stem_image_grad
    ok = (ctypes.byref(d), W, DX, IMG, WS, need, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return f(*args)
    for i in range(5):
        assert call(**{f"a{i}": None}) == -1, i
    assert b"null" in L.lib.vtd_last_error()
    assert call(a5=need - 1) == -4
    assert str(need).encode() in L.lib.vtd_last_error()
    assert call(a5=0) == -4
    for field in ("batch", "H", "W", "C", "patch", "d"):
        assert call(a0=ctypes.byref(dims(L, **{field: 0}))) == -1, field
        assert call(a0=ctypes.byref(dims(L, **{field: -1}))) == -1, field
    assert call(a0=ctypes.byref(dims(L, batch=1 << 16, H=256, W=128, patch=1))) == -1
    assert b"too large" in L.lib.vtd_last_error()
    assert call(a0=ctypes.byref(dims(L, d=1 << 24))) == -1
    assert call(a0=ctypes.byref(dims(L, patch=4096, C=1))) == -1
    for dtype in (0, 2, 4, -1):
        assert call(a0=ctypes.byref(dims(L, dtype=dtype))) == -2
        assert b"VTD_BF16X3" in L.lib.vtd_last_error()
    # misaligned bases: the workspace and w on 16 bytes, dx0 and dimages on 4
    for change in (dict(a4=WS + 8), dict(a1=W + 4), dict(a1=W + 8), dict(a2=DX + 2),
                   dict(a3=IMG + 1), dict(a3=IMG + 2)):
        assert call(**change) == -1, change
        assert b"misaligned" in L.lib.vtd_last_error()
    # dx0 and dimages off a 16-B boundary are accepted (the generic paths): the next check answers
    assert call(a2=DX + 4, a5=0) == -4
    assert call(a3=IMG + 4, a5=0) == -4
    assert call(a3=IMG + 12, a5=0) == -4


def test_workspace_is_monotone_in_batch_and_granular(L):
    for shape in (dict(H=40, W=36, patch=8, d=24), dict(H=224, W=224, patch=16, d=768),
                  dict(H=33, W=50, patch=7, d=6), dict(H=34, W=34, patch=17, d=28)):
        for dtype in (3, 1):
            prev = 0
            for batch in list(range(1, 40)) + [48, 64, 96, 128, 192, 256, 300, 512, 1024, 4096]:
                rc, n = ws_bytes(L, dims(L, batch=batch, dtype=dtype, **shape))
                assert rc == 0 and n % 256 == 0
                assert n >= prev, (shape, dtype, batch, n, prev)
                prev = n


def test_stem_backward_workspace_sizes_unchanged(L):
    """vtd_stem_backward_workspace_bytes still answers the recorded table."""
    from tests.test_train_plan_host import GOLDEN, train_workspace_table
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    table = train_workspace_table(L)
    stem = {k: v for k, v in table.items() if k.startswith("stem/")}
    assert len(stem) == 2 * len(M.STEM_CASES)
    for k, v in stem.items():
        assert golden[k] == v, k


def test_patch_embedding_keyword_needs_no_device_to_validate():
    """The new keyword changes no validation: the same errors, before any device call."""
    import vision_transformer_detector_amd as m
    img = torch.zeros((2, 40, 36, 3), requires_grad=True)
    ws = [torch.zeros((25, 1)), torch.zeros((192, 24)), torch.zeros((24,))]
    with pytest.raises(ValueError, match="patch_embedding: dtype .* no backward"):
        m.patch_embedding(img, ws, patch_size=8, dtype="float32", image_gradient=True)
    with pytest.raises(ValueError, match="images must be a device tensor"):
        m.patch_embedding(img, ws, patch_size=8, image_gradient=True)
