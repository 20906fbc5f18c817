"""The yardstick of the head backward, no GPU: the float64 oracle (tests/head_grad_oracle.py)
against central differences, the CPU emulation of the device's operand formats against the
bars the GPU test holds the device to, the new symbols, and every argument check through
ctypes -- all of which must answer before any device call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import head_grad_oracle as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ["vtd_gemm_wgrad", "vtd_gemm_wgrad_choice", "vtd_act_forward", "vtd_act_grad",
               "vtd_head_unscatter", "vtd_forward_encoded", "vtd_head_backward",
               "vtd_head_backward_workspace_bytes"]


def load_case(name, batch):
    """(kwargs, weights, encoded (B, N, d), dlogits (B, 17, 6)) -- seeded stand-ins for the
    encoder's output and the loss gradient, of their usual sizes."""
    if name == "multi_tile":
        kw = dict(H.MULTI_TILE)
        w = V.init_weights(seed=11, **kw)
    else:
        z = np.load(os.path.join(GOLD, f"{name}.npz"))
        kw = json.loads(str(z["kwargs"]))
        kw["input_shape"] = tuple(kw["input_shape"])
        w = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    n_tok = w["position_encoding/position_embedding/embeddings"].shape[0]
    rng = np.random.default_rng(len(name) + batch)
    encoded = rng.normal(0.0, 1.0, (batch, n_tok, kw["embedding_dim"])).astype(np.float32)
    dlogits = (rng.normal(0.0, 1.0, (batch, 17, 6)) / (batch * 17)).astype(np.float32)
    return kw, w, encoded, dlogits


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


@pytest.mark.parametrize("name", ["tiny_mish", "tiny_gelu"])
def test_oracle_gradients_match_central_differences(name):
    """float64, step 1e-6, 6 seeded coordinates of every tensor: within 1e-6 of the tensor's
    largest |gradient|."""
    kw, w, encoded, dlogits = load_case(name, 2)
    use_mish = kw.get("use_mish", True)
    _, grads = H.head_grads(w, encoded, dlogits, use_mish)
    dl = torch.tensor(dlogits, dtype=torch.float64)

    def value(hw, enc):
        return float((H.head_forward(hw, enc, use_mish) * dl).sum())

    rng = np.random.default_rng(7)
    h = 1e-6
    worst = 0.0
    for n, g in grads.items():
        top = np.abs(g).max()
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sign in (1.0, -1.0):
                hw = H.head_weights(w)
                enc = torch.tensor(encoded, dtype=torch.float64)
                target = enc if n == "encoded_images" else hw[n]
                target[idx] += sign * h
                vals.append(value(hw, enc))
            fd = (vals[0] - vals[1]) / (2 * h)
            worst = max(worst, abs(fd - g[idx]) / top)
    print(f"{name}: worst finite-difference error / tensor maximum {worst:.3g}")
    assert worst <= 1e-6


CASES = [("tiny_mish", 3), ("tiny_gelu", 2), ("tiny_seq400", 2), ("multi_tile", 16)]


@pytest.mark.parametrize("mode", ["bf16x3", "bfloat16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_emulated_backward_is_under_the_bars(case, mode):
    """The device's chain of products emulated on the CPU leaves room under the bars of
    tests/test_gpu_head_backward.py (2e-4 bf16x3, 5e-2 bfloat16)."""
    kw, w, encoded, dlogits = load_case(*case)
    use_mish = kw.get("use_mish", True)
    _, g64 = H.head_grads(w, encoded, dlogits, use_mish)
    _, emu = H.emulated_head_backward(w, encoded, dlogits, use_mish, mode)
    assert list(emu) == list(g64)
    worst = max(H.rel_err(emu[n], g64[n]) for n in g64)
    print(f"{case[0]} {mode}: emulation worst {worst:.3g}")
    assert worst <= H.BARS[mode]


def test_new_symbols_and_abi(L):
    assert L.lib.vtd_abi_version() == 17 == L.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib, name)


# ---- argument checks: fake device addresses, never dereferenced
X, G, W, PART = 0x10000, 0x20000, 0x30000, 0x40000


def wgrad(L, M=64, K=64, N=17, x=X, ldx=64, g=G, ldg=64, dtype=1, dw=W, ldw=17, db=None,
          part=PART, part_bytes=1 << 30, msplit=1):
    return L.lib.vtd_gemm_wgrad(M, K, N, x, ldx, g, ldg, dtype, dw, ldw, db, part, part_bytes,
                                msplit, None)


def test_wgrad_argument_errors(L):
    assert wgrad(L, x=None) == -1 and wgrad(L, g=None) == -1 and wgrad(L, dw=None) == -1
    assert wgrad(L, M=0) == -1 and wgrad(L, K=0) == -1 and wgrad(L, N=-1) == -1
    assert wgrad(L, ldx=60) == -1                       # ld % 8
    assert wgrad(L, ldx=56) == -1                       # ld < K
    assert wgrad(L, dtype=3, ldx=72) == -1              # VTD_BF16X3: ld % 16
    assert wgrad(L, dtype=3, ldx=64, ldg=64) == -1      # piece width ld / 2 < K
    assert wgrad(L, ldg=16) == -1 and wgrad(L, ldw=16) == -1
    assert wgrad(L, x=X + 2) == -1                      # alignment
    assert wgrad(L, msplit=0) == -1 and wgrad(L, msplit=3) == -1      # ceil(64 / 32) = 2
    assert wgrad(L, M=100000, msplit=257) == -1
    assert wgrad(L, msplit=2, part=None) == -1
    assert wgrad(L, msplit=2, part_bytes=2 * 65 * 17 * 4 - 1) == -1
    assert b"part_bytes" in L.lib.vtd_last_error()
    assert wgrad(L, dtype=0) == -2 and wgrad(L, dtype=2) == -2
    for M, K, N in ((4352, 8704, 4352), (50176, 768, 17), (17, 64, 6)):
        for dtype in (1, 3):
            c = L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype)
            assert 1 <= c <= min(-(-M // 32), 256)
    assert L.lib.vtd_gemm_wgrad_choice(4352, 8704, 4352, 1) == 1
    assert L.lib.vtd_gemm_wgrad_choice(50176, 768, 17, 1) > 8


def test_elementwise_argument_errors(L):
    f = L.lib.vtd_act_forward
    assert f(None, 4, 64, 64, 1, W, 64, 1, None) == -1
    assert f(X, 4, 64, 64, 1, None, 64, 1, None) == -1
    assert f(X, 0, 64, 64, 1, W, 64, 1, None) == -1
    assert f(X, 4, 64, 60, 1, W, 64, 1, None) == -1          # ldz < N
    assert f(X, 4, 64, 64, 7, W, 64, 1, None) == -1          # activation
    assert f(X, 4, 64, 64, 1, W, 60, 1, None) == -1          # lda % 8
    assert f(X, 4, 64, 64, 1, W, 64, 3, None) == -1          # piece width 32 < N
    assert f(X, 4, 64, 64, 1, W + 4, 64, 1, None) == -1      # alignment
    assert f(X, 4, 64, 64, 1, W, 64, 0, None) == -2
    g = L.lib.vtd_act_grad
    assert g(None, 64, G, 64, 4, 64, 2, W, 128, 3, None) == -1
    assert g(X, 64, None, 64, 4, 64, 2, W, 128, 3, None) == -1
    assert g(X, 64, G, 64, 4, 64, 2, None, 128, 3, None) == -1
    assert g(X, 64, G, 32, 4, 64, 2, W, 128, 3, None) == -1   # ldga < N
    assert g(X, 64, G, 64, 4, 64, 2, W, 120, 3, None) == -1   # ld % 16
    assert g(X, 64, G, 64, 4, 64, 2, W, 128, 2, None) == -2
    u = L.lib.vtd_head_unscatter
    assert u(None, 2, 25, 64, W, 128, 3, None) == -1
    assert u(X, 2, 25, 64, None, 128, 3, None) == -1
    assert u(X, 0, 25, 64, W, 128, 3, None) == -1
    assert u(X, 2, 25, 24, W, 128, 3, None) == -1             # ldu < T
    assert u(X, 2, 25, 64, W, 16, 3, None) == -1              # piece width 8 < 17
    assert u(X, 2, 25, 64, W, 64, 0, None) == -2


def config(L, dtype=3, batch=2):
    return L.VtdConfig(batch=batch, image_h=40, image_w=36, channels=3, patch_size=8,
                       embedding_dim=24, num_heads=3, key_dim=10, mlp_quantities=3,
                       repeat_times=2, head_last_units=8, head_layers=3, head_repeats=1,
                       use_mish=1, dtype=dtype)


def head_structs(L, n_head=3):
    P, Gr = L.VtdHeadParams(), L.VtdHeadGrads()
    for S in (P, Gr):
        S.w_det = S.b_det = S.w_final = S.b_final = X
        for j in range(n_head):
            S.w_head[j] = S.b_head[j] = X
    return P, Gr


def test_runtime_argument_errors(L):
    need = ctypes.c_size_t()
    wsb = L.lib.vtd_head_backward_workspace_bytes
    assert wsb(ctypes.byref(config(L)), ctypes.byref(need)) == 0 and need.value > 0
    bf16 = ctypes.c_size_t()
    assert wsb(ctypes.byref(config(L, dtype=1)), ctypes.byref(bf16)) == 0
    assert 0 < bf16.value < need.value
    assert wsb(ctypes.byref(config(L)), None) == -1
    assert wsb(None, ctypes.byref(need)) == -1
    for dtype in (0, 2):
        assert wsb(ctypes.byref(config(L, dtype=dtype)), ctypes.byref(need)) == -2
        assert b"VTD_BF16X3" in L.lib.vtd_last_error()
    wsb(ctypes.byref(config(L)), ctypes.byref(need))
    hb = L.lib.vtd_head_backward
    cfg, (P, Gr) = config(L), head_structs(L)
    ok = (ctypes.byref(cfg), ctypes.byref(P), X, G, None, ctypes.byref(Gr), W, need.value, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return hb(*args)
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a2=None) == -1
    assert call(a5=None) == -1 and call(a6=None) == -1
    assert call(a3=None) == -1                      # no dlogits and no logits: nothing to do
    assert call(a7=need.value - 1) == -4
    for dtype in (0, 2):
        c2 = config(L, dtype=dtype)
        assert call(a0=ctypes.byref(c2)) == -2
    P2, _ = head_structs(L)
    P2.w_head[1] = None
    assert call(a1=ctypes.byref(P2)) == -1
    _, G2 = head_structs(L)
    G2.b_final = None
    assert call(a5=ctypes.byref(G2)) == -1
    fe = L.lib.vtd_forward_encoded
    wts = L.VtdWeights()
    assert fe(ctypes.byref(cfg), ctypes.byref(wts), X, None, W, 1 << 40, None) == -1
    assert fe(ctypes.byref(cfg), None, X, G, W, 1 << 40, None) == -1
    assert fe(None, ctypes.byref(wts), X, G, W, 1 << 40, None) == -1
    assert fe(ctypes.byref(cfg), ctypes.byref(wts), X, G, W, 16, None) in (-1, -4)
