"""Dropout at model level without a GPU: the oracle of tests/model_dropout_oracle.py against the
undropped oracles, the site numbering, the condition on the head masks the GPU tests rely on, and
the argument checks of vtd_head_backward_dropout that return before any device call.
"""
import ctypes

import numpy as np
import pytest

from tests import dropout_oracle as D
from tests import head_grad_oracle as H
from tests import model_dropout_oracle as R
from tests import model_grad_oracle as M

CASES = pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])


def _dlogits(name, batch):
    rng = np.random.default_rng(len(name) + batch)
    return (rng.normal(0.0, 1.0, (batch, 17, 6)) / (batch * 17)).astype(np.float32)


def test_the_cases_are_the_issues():
    assert R.CASES == [("tiny_mish", 3), ("tiny_gelu", 2), ("multi_tile", 16), ("ragged_head", 3)]
    kw = R.load_case("ragged_head", 3)[0]
    assert R.shape_of(kw)[7] == [24, 12, 6] and kw["mlp_head_last_units"] == 6
    tiny = R.load_case("tiny_mish", 3)[0]
    assert {k: v for k, v in kw.items() if k != "mlp_head_last_units"} == \
        {k: v for k, v in tiny.items() if k != "mlp_head_last_units"}
    # every other case has head units divisible by the mask's 4-column patch
    for name, b in R.CASES[:3]:
        assert all(u % 4 == 0 for u in R.shape_of(R.load_case(name, b)[0])[7]), name


@CASES
def test_all_ones_head_masks_reproduce_the_undropped_head(case):
    name, b = case
    kw, w, _, _ = R.load_case(name, b)
    N, d, _, _, _, _, use_mish, _ = R.shape_of(kw)
    rng = np.random.default_rng(5)
    enc = rng.standard_normal((b, N, d))
    dl = _dlogits(name, b)
    ones = [np.ones_like(m) for m in R.head_masks(kw, b, 0.5, R.SEED, 0)]
    logits, grads = R.head_grads(w, enc, dl, use_mish, ones, 1.0)
    logits0, grads0 = H.head_grads(w, enc, dl, use_mish)
    assert np.array_equal(logits, logits0) and list(grads) == list(grads0)
    for n in grads0:
        assert np.array_equal(grads[n], grads0[n]), n


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[1], R.CASES[3]], ids=lambda c: c[0])
def test_all_ones_model_masks_reproduce_the_undropped_model(case):
    name, b = case
    kw, w, x, _ = R.load_case(name, b)
    dl = _dlogits(name, b)
    ones = R.ones_like_masks(R.model_masks(kw, b, 0.5, R.SEED, 0))
    logits, grads, dxs, den = R.model_grads(kw, w, x, dl, ones, 1.0)
    logits0, grads0, dxs0, den0 = M.model_grads(kw, w, x, dl)
    assert np.array_equal(logits, logits0) and list(grads) == list(grads0) and den == den0
    for n in grads0:
        assert np.array_equal(grads[n], grads0[n]), n
    assert all(np.array_equal(a, c) for a, c in zip(dxs, dxs0))


def test_masks_change_the_head_and_its_gradients():
    kw, w, _, _ = R.load_case("ragged_head", 3)
    N, d, _, _, _, _, use_mish, _ = R.shape_of(kw)
    enc = np.random.default_rng(6).standard_normal((3, N, d))
    dl = _dlogits("ragged_head", 3)
    masks = R.head_masks(kw, 3, 0.5, R.SEED, 0)
    logits, grads = R.head_grads(w, enc, dl, use_mish, masks, D.inv_keep(0.5))
    logits0, grads0 = H.head_grads(w, enc, dl, use_mish)
    assert H.rel_err(logits, logits0) > 1e-2
    # a dropped unit of the last hidden layer has no gradient into the final kernel's row:
    # dW_final[u] = sum_rows a[row][u] g[row], a = 0 where the mask is 0
    assert H.rel_err(grads["dense_1/kernel"], grads0["dense_1/kernel"]) > 1e-2


@CASES
def test_sites_are_consecutive_and_distinct(case):
    kw = R.load_case(*case)[0]
    _, _, _, _, q, L, _, units = R.shape_of(kw)
    s = R.sites(kw)
    assert s == list(range(L * (1 + q) + len(units)))
    assert R.head_site_base(kw) == L * (1 + q)
    # the masks of two sites differ, and so do those of two steps
    a = D.mask_rows(34, 8, 0.5, R.SEED, 0, s[-1])
    assert not np.array_equal(a, D.mask_rows(34, 8, 0.5, R.SEED, 0, s[-2]))
    assert not np.array_equal(a, D.mask_rows(34, 8, 0.5, R.SEED, 1, s[-1]))


@CASES
def test_head_masks_are_mask_rows_over_the_unpadded_plane(case):
    name, b = case
    kw = R.load_case(name, b)[0]
    units, base = R.shape_of(kw)[7], R.head_site_base(kw)
    masks = R.head_masks(kw, b, 0.1, R.SEED, 2)
    assert len(masks) == len(units)
    for j, (m, u) in enumerate(zip(masks, units)):
        assert m.shape == (b, 17, u)
        assert np.array_equal(m.reshape(b * 17, u), D.mask_rows(b * 17, u, 0.1, R.SEED, 2, base + j))
    # image 0 of the batch has the bits of image 0 alone
    alone = R.head_masks(kw, 1, 0.1, R.SEED, 2)
    assert all(np.array_equal(m[:1], a) for m, a in zip(masks, alone))


def test_the_issues_own_mask_figure():
    assert abs(D.mask_rows(51, 6, 0.5, 1234, 0, 8).mean() - 0.474) < 5e-4


@pytest.mark.parametrize("seed", [R.SEED, R.OTHER_SEED])
@CASES
def test_head_masks_at_rate_half_keep_between_03_and_07(case, seed):
    """A condition the GPU tests rely on, not a measurement: at the seeds and steps they use no
    head mask of any case is degenerate."""
    name, b = case
    kw = R.load_case(name, b)[0]
    for step in R.STEPS:
        for j, m in enumerate(R.head_masks(kw, b, 0.5, seed, step)):
            assert 0.3 <= m.mean() <= 0.7, (name, seed, step, j, m.mean())


# ------------------------------------------------------------------ the C entry's checks
@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def _config(L, kw, batch, dtype):
    k = dict(mlp_head_dense_mish_block_repeats=1, use_mish=True)
    k.update(kw)
    h, w, c = k["input_shape"]
    return L.VtdConfig(batch=batch, image_h=h, image_w=w, channels=c, patch_size=k["patch_size"],
                       embedding_dim=k["embedding_dim"], num_heads=k["encoder_num_heads"],
                       key_dim=k["encoder_key_dim"], mlp_quantities=k["encoder_mlp_quantities"],
                       repeat_times=k["encoder_repeat_times"],
                       head_last_units=k["mlp_head_last_units"],
                       head_layers=k["mlp_head_dense_layers_quantity"],
                       head_repeats=k["mlp_head_dense_mish_block_repeats"],
                       use_mish=1 if k["use_mish"] else 0, dtype=dtype)


def test_head_entry_is_bound_and_checks_its_dropout_before_any_device_call(L):
    assert hasattr(L.lib, "vtd_head_backward_dropout")
    kw = R.load_case("ragged_head", 3)[0]
    cfg = _config(L, kw, 3, L.BF16X3)
    params, grads = L.VtdHeadParams(), L.VtdHeadGrads()

    def call(drop, c=cfg):
        return L.lib.vtd_head_backward_dropout(ctypes.byref(c), ctypes.byref(params), 4096, 4096,
                                               4096, ctypes.byref(grads), 4096, 1 << 30, None, drop)
    assert call(None) == -1 and b"null dropout" in L.lib.vtd_last_error()
    for rate in (-0.5, 1.0, 1.5, float("nan"), float("inf")):
        d = L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=rate)
        assert call(ctypes.byref(d)) == -1 and b"rate" in L.lib.vtd_last_error(), rate
    # 3 head layers: site_base + 3 must stay within 32 bits
    d = L.VtdBlockDropout(seed=1, step=0, site_base=0xFFFFFFFE, rate=0.5)
    assert call(ctypes.byref(d)) == -1 and b"site_base" in L.lib.vtd_last_error()
    # a valid dropout, the largest site_base: vtd_head_backward's own checks (null weights here)
    for rate in (0.5, 0.0):
        d = L.VtdBlockDropout(seed=1, step=0, site_base=0xFFFFFFFC, rate=rate)
        assert call(ctypes.byref(d)) == -1 and b"null weight" in L.lib.vtd_last_error()
    # the mode check is vtd_head_backward's
    d = L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=0.5)
    assert call(ctypes.byref(d), _config(L, kw, 3, L.F32)) == -2
