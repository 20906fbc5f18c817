"""encoder_block(dropout=...) / vtd_encoder_block_backward_dropout on the GPU against the masked
float64 block of tests/dropout_oracle.py: the reference's block with `dropout` -- on the
attention probabilities (site_base) and after every MLP activation (site_base + 1 + j).

Cases, measure and bars are those of tests/test_gpu_encoder_block.py (per tensor
max |g - g64| / max |g64|, the key bias against max sum_rows |dK64|; 2e-4 bf16x3, 5e-2 bfloat16;
y within that file's forward tolerance): the masks rescale the device's and the oracle's terms
alike.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import block_grad_oracle as K
from tests import dropout_oracle as D
from tests.test_gpu_encoder_block import same_bits
from tests.test_gpu_head_backward import TOL, within

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]
CASES = K.CASES[:4]
RATES = (0.5, 0.1)
SEED, STEP, BASE = 0xFEEDFACE12345678, 7, 4


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def oracle():
    """One masked float64 run per (case, rate), shared by both modes."""
    cache = {}

    def get(case, rate):
        if (case, rate) not in cache:
            w = K.seeded_weights(case)
            x, dy = K.seeded_inputs(case)
            masks = D.block_masks(case, rate, SEED, STEP, BASE)
            y64, g64, dx64, den = D.chain_grads([w], x, dy, case[6], [masks], D.inv_keep(rate))
            cache[(case, rate)] = dict(w=w, x=x, dy=dy, y64=y64, g64=g64[0], dx64=dx64, den=den[0])
        return cache[(case, rate)]
    return get


def block(vtd, cuda, case, mode, o, **kw):
    """(y, dx, grads) of one encoder_block forward + backward on the oracle's inputs."""
    B, N, d, heads, dk, q, use_mish = case
    x = torch.from_numpy(o["x"]).to(cuda).requires_grad_(True)
    w = [torch.from_numpy(t).to(cuda).requires_grad_(True) for t in o["w"]]
    y = vtd.encoder_block(x, w, num_heads=heads, key_dim=dk, use_mish=use_mish, dtype=mode, **kw)
    y.backward(torch.from_numpy(o["dy"]).to(cuda))
    return y.detach(), x.grad, [t.grad for t in w]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_block_against_masked_float64(vtd, cuda, oracle, case, mode, rate):
    o = oracle(case, rate)
    kw = dict(dropout=rate, seed=SEED, step=STEP, site_base=BASE)
    y, dx, grads = block(vtd, cuda, case, mode, o, **kw)
    errs = K.rel_errors([g.cpu().numpy() for g in grads], dx.cpu().numpy(), o["g64"], o["dx64"],
                        o["den"], case[5])
    top = max(errs, key=errs.get)
    yn = y.cpu().numpy()
    print(f"{K.case_id(case)} {mode} rate {rate}: worst {errs[top]:.3g} ({top}); y "
          f"{np.abs(yn - o['y64']).max() / np.abs(o['y64']).max():.3g}; "
          + ", ".join(f"{n} {v:.2g}" for n, v in errs.items()))
    assert within(yn, o["y64"], TOL[mode])
    for n, v in errs.items():
        assert v <= K.BARS[mode], f"{n}: {v:.3g} > {K.BARS[mode]}"
    # the same call again: the same bits; another step: another y
    y2, dx2, grads2 = block(vtd, cuda, case, mode, o, **kw)
    assert same_bits(y2, y) and same_bits(dx2, dx)
    assert all(same_bits(a, b) for a, b in zip(grads2, grads))
    y3, _, _ = block(vtd, cuda, case, mode, o, **dict(kw, step=STEP + 1))
    assert not same_bits(y3, y)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_no_dropout_is_todays_block_bit_for_bit(vtd, cuda, oracle, case, mode):
    o = oracle(case, 0.5)
    y0, dx0, g0 = block(vtd, cuda, case, mode, o)
    for kw in (dict(dropout=None), dict(dropout=0.0), dict(dropout=0.0, seed=3, step=9)):
        y, dx, g = block(vtd, cuda, case, mode, o, **kw)
        assert same_bits(y, y0) and same_bits(dx, dx0)
        assert all(same_bits(a, b) for a, b in zip(g, g0))


@pytest.mark.parametrize("mode", MODES)
def test_c_entry_workspace_guards_and_rate_zero(vtd, cuda, oracle, mode):
    """The C entry with exactly vtd_encoder_block_backward_workspace_bytes inside 0xA5 guard
    bands gives the autograd op's bits; one byte less is VTD_ERR_WORKSPACE; rate 0 through the
    dropout entry is vtd_encoder_block_backward."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import encoder as enc
    case = K.TINY_MISH
    B, N, d, heads, dk, q, use_mish = case
    o = oracle(case, 0.5)
    y, dx, grads = block(vtd, cuda, case, mode, o, dropout=0.5, seed=SEED, step=STEP, site_base=BASE)
    dims = enc.block_dims(B, N, d, heads, dk, q, use_mish, mode)
    need = enc.workspace_bytes(dims)
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
    x = torch.from_numpy(o["x"]).to(cuda)
    w = [torch.from_numpy(t).to(cuda) for t in o["w"]]
    dy = torch.from_numpy(o["dy"]).to(cuda)
    for rate, want in ((0.5, (y, dx, grads)), (0.0, block(vtd, cuda, case, mode, o))):
        drop = L.VtdBlockDropout(seed=SEED, step=STEP, site_base=BASE, rate=rate)
        got = enc.run(x, w, dims, dy=dy, ws=buf[256:256 + need], drop=drop)
        torch.cuda.synchronize()
        assert same_bits(got[0], want[0]) and same_bits(got[2], want[1])
        assert all(same_bits(a, b) for a, b in zip(got[1], want[2]))
        assert bool((buf[:256] == 0xA5).all() and (buf[-256:] == 0xA5).all())
    with pytest.raises(L.VtdError, match="WORKSPACE"):
        enc.run(x, w, dims, dy=dy, ws=buf[256:256 + need - 1],
                drop=L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=0.5))
    for bad in (L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=1.0),
                L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=float("nan")),
                L.VtdBlockDropout(seed=1, step=0, site_base=0xFFFFFFFF, rate=0.5)):
        with pytest.raises(ValueError):
            enc.run(x, w, dims, dy=dy, ws=buf[256:256 + need], drop=bad)
    params = enc._fill(L.VtdBlockParams(), w, q)
    assert L.lib.vtd_encoder_block_backward_dropout(
        ctypes.byref(dims), ctypes.byref(params), x.data_ptr(), None, y.data_ptr(), None,
        buf.data_ptr() + 256, need, L.stream_ptr(), None) == -1


@pytest.mark.parametrize("mode", MODES)
def test_two_block_chain_with_distinct_sites(vtd, cuda, mode):
    """block(block(x)) through autograd, block i at site_base i (1 + q), against the float64 chain
    with the two blocks' masks."""
    case = K.TINY_MISH
    B, N, d, heads, dk, q, use_mish = case
    rate = 0.5
    blocks = [K.seeded_weights(case, seed=s) for s in (1, 2)]
    x, dy = K.seeded_inputs(case, seed=1)
    bases = [i * (1 + q) for i in range(2)]
    masks = [D.block_masks(case, rate, SEED, STEP, b) for b in bases]
    y64, g64, dx64, den = D.chain_grads(blocks, x, dy, use_mish, masks, D.inv_keep(rate))
    xt = torch.from_numpy(x).to(cuda).requires_grad_(True)
    ws = [[torch.from_numpy(t).to(cuda).requires_grad_(True) for t in w] for w in blocks]
    y = xt
    for w, base in zip(ws, bases):
        y = vtd.encoder_block(y, w, num_heads=heads, key_dim=dk, use_mish=use_mish, dtype=mode,
                              dropout=rate, seed=SEED, step=STEP, site_base=base)
    (y * torch.from_numpy(dy).to(cuda)).sum().backward()
    assert within(y.detach().cpu().numpy(), y64, TOL[mode])
    for b, w in enumerate(ws):
        errs = K.rel_errors([t.grad.cpu().numpy() for t in w], xt.grad.cpu().numpy(), g64[b], dx64,
                            den[b], q)
        top = max(errs, key=errs.get)
        print(f"two-block chain {mode} rate {rate}, block {b}: worst {errs[top]:.3g} ({top})")
        for n, v in errs.items():
            assert v <= K.BARS[mode], f"block {b} {n}: {v:.3g} > {K.BARS[mode]}"


def test_validation(vtd, cuda):
    case = K.TINY_MISH
    B, N, d, heads, dk, q, use_mish = case
    x = torch.from_numpy(K.seeded_inputs(case)[0]).to(cuda)
    w = [torch.from_numpy(t).to(cuda) for t in K.seeded_weights(case)]
    kw = dict(num_heads=heads, key_dim=dk, use_mish=use_mish)
    with pytest.raises(ValueError, match="seed"):
        vtd.encoder_block(x, w, dropout=0.5, seed=None, **kw)
    with pytest.raises(ValueError, match="rate"):
        vtd.encoder_block(x, w, dropout=1.0, seed=1, **kw)
    with pytest.raises(ValueError, match="site_base"):
        vtd.encoder_block(x, w, dropout=0.5, seed=1, site_base=(1 << 32) - 2, **kw)
