"""Dropout without a GPU: the Philox known answers, the numpy mask's statistics, the float64
masked attention gradients against central differences, and the C ABI of the dropout entries
(symbols, struct layout against a gcc probe, argument checks that return before any device call).
"""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import dropout_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vtd.h")
SYMBOLS = ("vtd_dropout_mask", "vtd_dropout_mask_attention", "vtd_dropout_apply",
           "vtd_act_forward_dropout", "vtd_act_grad_dropout", "vtd_attention_train_dropout",
           "vtd_attention_backward_dropout", "vtd_encoder_block_backward_dropout")


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = D.philox4x32_10([np.uint32(c) for c in ctr], key)
    assert tuple(int(g) for g in got) == want


def test_philox_is_vectorised_consistently():
    """An array of counters gives what each counter gives alone."""
    c0 = np.arange(5, dtype=np.uint32)
    many = D.philox4x32_10([c0, np.uint32(7), np.uint32(8), np.uint32(9)], (1, 2))
    for i in range(5):
        one = D.philox4x32_10([np.uint32(i), np.uint32(7), np.uint32(8), np.uint32(9)], (1, 2))
        assert [int(w[i]) for w in many] == [int(w) for w in one]


@pytest.mark.parametrize("seed", [1, 0x0123456789ABCDEF])
@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_kept_count_is_binomial(rate, seed):
    """2^20 elements: the kept count within 6 standard deviations of n (1 - realised rate), at an
    elementwise site and at an attention site."""
    n = 1 << 20
    keep_p = 1.0 - D.threshold(rate) / 65536.0
    assert abs((1.0 - keep_p) - rate) <= 2.0 ** -16
    sd = math.sqrt(n * keep_p * (1.0 - keep_p))
    for m in (D.mask_rows(1024, 1024, rate, seed), D.mask_attention(2, 2, 512, rate, seed)):
        assert m.size == n and m.dtype == np.bool_
        print(f"rate {rate} seed {seed:#x}: kept {int(m.sum())}, expected {n * keep_p:.0f}, sd {sd:.0f}")
        assert abs(int(m.sum()) - n * keep_p) <= 6.0 * sd


def test_inv_keep():
    assert D.inv_keep(0.5) == np.float32(2.0)
    assert D.inv_keep(0.25) == np.float32(1.0 / 0.75)
    assert D.threshold(0.999999) == 65535 and D.threshold(0.0) == 0


def test_masks_differ_by_site_step_and_seed():
    base = D.mask_rows(64, 64, 0.5, 11, step=3, site=2)
    assert (base == D.mask_rows(64, 64, 0.5, 11, step=3, site=2)).all()
    for other in (D.mask_rows(64, 64, 0.5, 11, step=3, site=3),
                  D.mask_rows(64, 64, 0.5, 11, step=4, site=2),
                  D.mask_rows(64, 64, 0.5, 12, step=3, site=2),
                  D.mask_rows(64, 64, 0.5, 11 + (1 << 32), step=3, site=2),
                  D.mask_rows(64, 64, 0.5, 11, step=3 + (1 << 32), site=2)):
        frac = float((base != other).mean())
        assert 0.4 < frac < 0.6, frac
    a = D.mask_attention(2, 2, 32, 0.5, 11)
    # images and heads draw different bits; a sub-block of a longer sequence is the same mask
    assert 0.4 < float((a[0, 0] != a[1, 0]).mean()) < 0.6
    assert 0.4 < float((a[0, 0] != a[0, 1]).mean()) < 0.6
    assert (D.mask_attention(1, 2, 20, 0.5, 11)[0] == a[0, :, :20, :20]).all()
    # rows of an elementwise site do not depend on how many there are or where a view starts
    assert (D.mask_rows(7, 13, 0.5, 11, row0=5) == D.mask_rows(64, 64, 0.5, 11)[5:12, :13]).all()


def test_masked_attention_gradients_match_central_differences():
    B, H, N, dk = 1, 2, 5, 4
    rng = np.random.default_rng(5)
    q, k, v, do = (rng.normal(size=(B, N, H, dk)) for _ in range(4))
    mask = D.mask_attention(B, H, N, 0.5, seed=9)
    assert mask.any() and not mask.all()
    c, scale = 2.0, 0.5
    grads = D.backward64(q, k, v, do, scale, mask, c)

    def loss(q_, k_, v_):
        return float((D.forward64(q_, k_, v_, scale, mask, c)[0] * do).sum())
    eps = 1e-6
    for which, g in enumerate(grads):
        num = np.zeros_like(g)
        for idx in np.ndindex(g.shape):
            t = [q.copy(), k.copy(), v.copy()]
            t[which][idx] += eps
            up = loss(*t)
            t[which][idx] -= 2 * eps
            num[idx] = (up - loss(*t)) / (2 * eps)
        assert np.abs(num - g).max() <= 1e-8 * max(1.0, np.abs(g).max()), which
    # lse and P are the undropped softmax's
    o, lse, p = D.forward64(q, k, v, scale, mask, c)
    assert np.allclose(p.sum(-1), 1.0)


def test_symbols_and_abi(L):
    for n in SYMBOLS:
        assert hasattr(L.lib, n) and n in L.SIGNATURES, n
    assert L.lib.vtd_abi_version() == 17 and L.ABI_VERSION == 17
    import vision_transformer_detector_amd as vtd
    assert callable(vtd.dropout) and callable(vtd.dropout_mask)


def test_struct_layout_matches_c(L):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "vtd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(vtd_dropout), offsetof(vtd_dropout, seed),
         offsetof(vtd_dropout, step), offsetof(vtd_dropout, site), offsetof(vtd_dropout, rate));
  printf("%zu %zu %zu %zu %zu\n", sizeof(vtd_block_dropout), offsetof(vtd_block_dropout, seed),
         offsetof(vtd_block_dropout, step), offsetof(vtd_block_dropout, site_base),
         offsetof(vtd_block_dropout, rate));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    S, T = L.VtdDropout, L.VtdBlockDropout
    assert [int(x) for x in out] == [ctypes.sizeof(S), S.seed.offset, S.step.offset, S.site.offset,
                                     S.rate.offset, ctypes.sizeof(T), T.seed.offset, T.step.offset,
                                     T.site_base.offset, T.rate.offset]


def _calls(L, drop):
    """Every dropout entry with plausible (never dereferenced) pointers and the given vtd_dropout."""
    p = 4096
    return {
        "vtd_dropout_mask": lambda: L.lib.vtd_dropout_mask(drop, 4, 8, p, 8, None),
        "vtd_dropout_mask_attention": lambda: L.lib.vtd_dropout_mask_attention(drop, 1, 1, 8, p, None),
        "vtd_dropout_apply": lambda: L.lib.vtd_dropout_apply(drop, p, 8, 4, 8, p, 8, None),
        "vtd_act_forward_dropout": lambda: L.lib.vtd_act_forward_dropout(
            p, 4, 8, 8, L.ACT_MISH, p, 8, L.BF16, None, drop),
        "vtd_act_grad_dropout": lambda: L.lib.vtd_act_grad_dropout(
            p, 8, p, 8, 4, 8, L.ACT_MISH, p, 8, L.BF16, None, drop),
        "vtd_attention_train_dropout": lambda: L.lib.vtd_attention_train_dropout(
            p, 1, 8, 1, 32, 96, 0.5, p, 32, p, L.BF16, None, drop),
        "vtd_attention_backward_dropout": lambda: L.lib.vtd_attention_backward_dropout(
            p, p, p, p, 1, 8, 1, 32, 96, 32, 32, 0.5, p, 96, L.BF16, p, 1 << 20, None, drop),
    }


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_bad_rates_are_refused_before_any_device_call(L, rate):
    drop = ctypes.byref(L.VtdDropout(seed=1, step=0, site=0, rate=rate))
    for name, call in _calls(L, drop).items():
        assert call() == -1, name
        assert b"rate" in L.lib.vtd_last_error(), name


def test_null_struct_and_bad_arguments_are_refused(L):
    for name, call in _calls(L, None).items():
        assert call() == -1, name
        assert b"null dropout" in L.lib.vtd_last_error(), name
    ok = ctypes.byref(L.VtdDropout(seed=1, step=0, site=0, rate=0.5))
    lib = L.lib
    assert lib.vtd_dropout_mask(ok, 4, 8, None, 8, None) == -1
    assert lib.vtd_dropout_mask(ok, 4, 8, 4096, 7, None) == -1            # ldo < N
    assert lib.vtd_dropout_mask(ok, 0, 8, 4096, 8, None) == -1
    assert lib.vtd_dropout_mask_attention(ok, 1, 0, 8, 4096, None) == -1
    assert lib.vtd_dropout_apply(ok, 4096, 7, 4, 8, 4096, 8, None) == -1
    assert lib.vtd_dropout_apply(ok, None, 8, 4, 8, 4096, 8, None) == -1
    # the wrapped entries' own checks still hold with a valid dropout
    assert lib.vtd_act_forward_dropout(4096, 4, 8, 8, 9, 4096, 8, L.BF16, None, ok) == -1
    assert lib.vtd_act_grad_dropout(4096, 8, None, 8, 4, 8, 0, 4096, 8, L.BF16, None, ok) == -1
    assert lib.vtd_attention_train_dropout(4096, 1, 8, 1, 48, 144, 0.5, 4096, 48, 4096, L.BF16,
                                           None, ok) == -1
    assert lib.vtd_attention_train_dropout(4096, 1, 8, 1, 32, 96, 0.5, 4096, 32, 4096, L.F32,
                                           None, ok) == -2
    assert lib.vtd_attention_backward_dropout(4096, 4096, 4096, 4096, 1, 8, 1, 32, 96, 32, 32, 0.5,
                                              4096, 96, L.BF16, 4096, 0, None, ok) == -4


def test_block_entry_checks_its_dropout_before_anything_else(L):
    dims = L.VtdBlockDims(batch=1, tokens=3, d=8, num_heads=1, key_dim=4, mlp_quantities=1,
                          use_mish=1, dtype=L.BF16X3)
    params, grads = L.VtdBlockParams(), L.VtdBlockGrads()

    def call(drop):
        return L.lib.vtd_encoder_block_backward_dropout(
            ctypes.byref(dims), ctypes.byref(params), 4096, 4096, 4096, ctypes.byref(grads), 4096,
            1 << 30, None, drop)
    assert call(None) == -1 and b"null dropout" in L.lib.vtd_last_error()
    for rate in (-0.5, 1.0, float("nan")):
        d = L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=rate)
        assert call(ctypes.byref(d)) == -1 and b"rate" in L.lib.vtd_last_error()
    d = L.VtdBlockDropout(seed=1, step=0, site_base=0xFFFFFFFF, rate=0.5)
    assert call(ctypes.byref(d)) == -1 and b"site_base" in L.lib.vtd_last_error()
    # a valid dropout: the block entry's own checks (null weight pointers here)
    d = L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=0.5)
    assert call(ctypes.byref(d)) == -1 and b"null weight" in L.lib.vtd_last_error()


def test_python_argument_rules():
    from vision_transformer_detector_amd.dropout import inv_keep, spec
    assert spec("t", None, None) is None and spec("t", 0.0, None) is None
    with pytest.raises(ValueError, match="seed"):
        spec("t", 0.5, None)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="rate"):
            spec("t", bad, 1)
    d = spec("t", 0.25, (1 << 64) - 1, step=5, site=7)
    assert (d.seed, d.step, d.site) == ((1 << 64) - 1, 5, 7) and d.rate == 0.25
    with pytest.raises(ValueError):
        spec("t", 0.25, 1 << 64)
    assert inv_keep(0.5) == 2.0 and np.float32(inv_keep(0.25)) == D.inv_keep(0.25)
