"""vtd_encoder_block_backward, encoder_block and Model.encoder_block_weights on the GPU against
the float64 block of tests/block_grad_oracle.py.

Cases (B, N, d, heads, key_dim, q, act), the smallest shapes at which each branch of the chain can
still go wrong:
  (1, 3, 8, 1, 4, 1, mish)        fewest rows; one MLP layer: the MLP step runs once, with g = dy
  (3, 25, 24, 3, 10, 3, mish)     the tiny_mish block: key_dim 10 -> dkp 32, d 24 -> d_p 64, every
                                  pad path of the gather / un-gather kernels
  (2, 40, 20, 2, 12, 2, gelu)     the tiny_gelu block
  (2, 400, 32, 3, 16, 2, mish)    N > 256: multi-workgroup attention passes
  (16, 256, 64, 2, 32, 2, mish)   4096 rows: several GEMM row tiles, msplit > 1, many LayerNorm
                                  ranges, key_dim == dkp
  (2, 77, 768, 12, 64, 3, gelu)   the real widths (LayerNorm NV = 3, dkp 64, MLP 3072 / 1536 / 768)

Measure per tensor: max |g - g64| / max |g64| against the oracle fed the same float32 x, dy and
weights; bars head_grad_oracle.BARS, 2e-4 in bf16x3 and 5e-2 in bfloat16, for every tensor: the
CPU emulation (tests/test_block_grad_kat.py) stays under half of them at every case (worst 5.0e-5
and 1.6e-2), so no tensor needed a bar of its own.  One tensor has no max |g64|: the key bias,
whose gradient is zero for every input (softmax ignores a shift common to all keys); its error is
taken against max sum_rows |dK64|, the magnitude of the terms that cancel
(block_grad_oracle._denominators), as the attention test does for its single-key case.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import block_grad_oracle as K
from tests.test_gpu_head_backward import TOL, within

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["bf16x3", "bfloat16"]
GUARD = 256            # bytes of 0xA5 on either side of every output


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def enc(vtd):
    from vision_transformer_detector_amd import encoder
    return encoder


@pytest.fixture(scope="module")
def oracle():
    """One float64 run per case, shared by both modes and every test."""
    cache = {}

    def get(case):
        if case not in cache:
            w = K.seeded_weights(case)
            x, dy = K.seeded_inputs(case)
            y64, g64, dx64, den = K.block_grads(w, x, dy, case[6])
            cache[case] = dict(w=w, x=x, dy=dy, y64=y64, g64=g64, dx64=dx64, den=den)
        return cache[case]
    return get


def guarded(shape, device):
    """(tensor, buffer): a float32 tensor inside a byte buffer filled with 0xA5, GUARD bytes of
    it on either side."""
    n = 4 * int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
    return buf[GUARD:GUARD + n].view(torch.float32).reshape(shape), buf


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


@pytest.fixture(scope="module")
def runs(cuda, enc, oracle):
    """The device calls of one (case, mode), shared by the tests below."""
    cache = {}

    def get(case, mode):
        key = (case, mode)
        if key in cache:
            return cache[key]
        B, N, d, heads, dk, q, use_mish = case
        o = oracle(case)
        w = [torch.from_numpy(t).to(cuda) for t in o["w"]]
        x, dy = torch.from_numpy(o["x"]).to(cuda), torch.from_numpy(o["dy"]).to(cuda)
        dims = enc.block_dims(B, N, d, heads, dk, q, use_mish, mode)
        need = enc.workspace_bytes(dims)
        # run A: every output inside guard bands, the workspace poisoned with NaN bytes
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        outs = [guarded(x.shape, cuda)] + [guarded(t.shape, cuda) for t in w] \
            + [guarded(x.shape, cuda)]
        y, grads, dx = enc.run(x, w, dims, dy=dy, ws=ws,
                               out=(outs[0][0], [t for t, _ in outs[1:-1]], outs[-1][0]))
        # run B: the same call again on the workspace as run A left it; run Z on zeros
        again = enc.run(x, w, dims, dy=dy, ws=ws)
        zeroed = enc.run(x, w, dims, dy=dy, ws=torch.zeros_like(ws))
        fwd_only = enc.run(x, w, dims, ws=torch.full_like(ws, 0xFF))[0]
        no_dx = enc.run(x, w, dims, dy=dy, want_dx=False, ws=ws)
        torch.cuda.synchronize()
        cache[key] = dict(o=o, w=w, x=x, dy=dy, dims=dims, y=y, grads=grads, dx=dx,
                          buffers=[b for _, b in outs], again=again, zeroed=zeroed,
                          fwd_only=fwd_only, no_dx=no_dx)
        return cache[key]
    return get


params = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", K.CASES, ids=K.case_id)


@params
@cases
def test_gradients_against_float64(runs, case, mode):
    r = runs(case, mode)
    o = r["o"]
    for g, g64 in zip(r["grads"], o["g64"]):
        assert tuple(g.shape) == g64.shape and g.dtype == torch.float32
    errs = K.rel_errors([g.cpu().numpy() for g in r["grads"]], r["dx"].cpu().numpy(), o["g64"],
                        o["dx64"], o["den"], case[5])
    top = max(errs, key=errs.get)
    print(f"{K.case_id(case)} {mode}: worst {errs[top]:.3g} ({top}); "
          + ", ".join(f"{n} {v:.2g}" for n, v in errs.items()))
    for n, v in errs.items():
        assert v <= K.BARS[mode], f"{n}: {v:.3g} > {K.BARS[mode]}"


@params
@cases
def test_forward_value(runs, case, mode):
    """y of the forward-only call has the bits of the full call's y, and is within the mode's
    forward tolerance of the float64 block."""
    r = runs(case, mode)
    assert same_bits(r["fwd_only"], r["y"])
    y, y64 = r["y"].cpu().numpy(), r["o"]["y64"]
    print(f"{K.case_id(case)} {mode}: forward max |y - y64| / max |y64| "
          f"{np.abs(y - y64).max() / np.abs(y64).max():.3g}")
    assert within(y, y64, TOL[mode])


@params
@cases
def test_runs_are_bit_identical_and_read_nothing_unwritten(runs, case, mode):
    """The run on a NaN-poisoned workspace, a second run on the workspace it left and a run on a
    zeroed workspace give the same bits in every output: nothing is read before it is written,
    pad columns included, and no sum depends on timing."""
    r = runs(case, mode)
    for name in ("again", "zeroed"):
        y, grads, dx = r[name]
        assert same_bits(y, r["y"]) and same_bits(dx, r["dx"]), name
        for i, (a, b) in enumerate(zip(grads, r["grads"])):
            assert same_bits(a, b), (name, K.names(case[5])[i])
    for t in [r["y"], r["dx"]] + list(r["grads"]):
        assert bool(torch.isfinite(t).all())


@params
@cases
def test_guard_bands_intact(runs, case, mode):
    r = runs(case, mode)
    labels = ["y"] + K.names(case[5]) + ["dx"]
    for label, buf in zip(labels, r["buffers"]):
        assert guards_intact(buf), label


@params
@cases
def test_without_dx_the_weight_gradients_keep_their_bits(runs, case, mode):
    r = runs(case, mode)
    _, grads, dx = r["no_dx"]
    assert dx is None
    for i, (a, b) in enumerate(zip(grads, r["grads"])):
        assert same_bits(a, b), K.names(case[5])[i]


@params
@cases
def test_autograd_op_equals_the_c_call(vtd, runs, case, mode):
    r = runs(case, mode)
    B, N, d, heads, dk, q, use_mish = case
    x = r["x"].clone().requires_grad_(True)
    w = [t.clone().requires_grad_(True) for t in r["w"]]
    y = vtd.encoder_block(x, w, num_heads=heads, key_dim=dk, use_mish=use_mish, dtype=mode)
    assert same_bits(y.detach(), r["y"])
    y.backward(r["dy"])
    assert same_bits(x.grad, r["dx"])
    for i, (t, g) in enumerate(zip(w, r["grads"])):
        assert same_bits(t.grad, g), K.names(q)[i]
    # inputs that do not require grad get None: x and every other weight frozen
    x2 = r["x"].clone()
    w2 = [t.clone().requires_grad_(i % 2 == 0) for i, t in enumerate(r["w"])]
    y2 = vtd.encoder_block(x2, w2, num_heads=heads, key_dim=dk, use_mish=use_mish, dtype=mode)
    y2.backward(r["dy"])
    assert x2.grad is None
    for i, (t, g) in enumerate(zip(w2, r["grads"])):
        if i % 2 == 0:
            assert same_bits(t.grad, g), K.names(q)[i]
        else:
            assert t.grad is None, K.names(q)[i]


@params
def test_two_block_chain(vtd, cuda, mode):
    """y2 = block(block(x, w_a), w_b) through torch autograd at the tiny_mish shape against the
    float64 two-block chain, same measure and bars."""
    case = K.TINY_MISH
    B, N, d, heads, dk, q, use_mish = case
    blocks = [K.seeded_weights(case, seed=s) for s in (1, 2)]
    x, dy = K.seeded_inputs(case, seed=1)
    y64, g64, dx64, den = K.chain_grads(blocks, x, dy, use_mish)
    xt = torch.from_numpy(x).to(cuda).requires_grad_(True)
    ws = [[torch.from_numpy(t).to(cuda).requires_grad_(True) for t in w] for w in blocks]
    y = xt
    for w in ws:
        y = vtd.encoder_block(y, w, num_heads=heads, key_dim=dk, use_mish=use_mish, dtype=mode)
    (y * torch.from_numpy(dy).to(cuda)).sum().backward()
    assert within(y.detach().cpu().numpy(), y64, TOL[mode])
    for b, w in enumerate(ws):
        errs = K.rel_errors([t.grad.cpu().numpy() for t in w], xt.grad.cpu().numpy(), g64[b], dx64,
                            den[b], q)
        top = max(errs, key=errs.get)
        print(f"two-block chain {mode}, block {b}: worst {errs[top]:.3g} ({top})")
        for n, v in errs.items():
            assert v <= K.BARS[mode], f"block {b} {n}: {v:.3g} > {K.BARS[mode]}"


@params
def test_model_encoder_block_weights(vtd, cuda, mode):
    z = np.load(os.path.join(GOLD, "tiny_gelu.npz"))
    kw = json.loads(str(z["kwargs"]))
    kw["input_shape"] = tuple(kw["input_shape"])
    w = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    model.set_weights(w)
    q, reps = kw["encoder_mlp_quantities"], kw["encoder_repeat_times"]
    per = 12 + 2 * q
    all_names = list(vtd.keras_weight_names(kw, model.dims).items())
    for i in range(reps):
        bw = model.encoder_block_weights(i)
        want = all_names[3 + i * per: 3 + (i + 1) * per]
        assert list(bw) == [n for n, _ in want]
        for (n, shape), t in zip(want, bw.values()):
            assert tuple(t.shape) == tuple(shape) and t.dtype == torch.float32 and t.is_cuda
            assert not t.requires_grad
            assert np.array_equal(t.cpu().numpy(), np.asarray(w[n], np.float32)), n
    assert "attention_output/kernel" in list(model.encoder_block_weights(0))[8]
    for bad in (-1, reps, 0.0):
        with pytest.raises(ValueError, match="block index"):
            model.encoder_block_weights(bad)
    # the block applied to these weights reproduces the float64 block on them
    d, heads, dk = kw["embedding_dim"], kw["encoder_num_heads"], kw["encoder_key_dim"]
    use_mish = kw.get("use_mish", True)
    x = np.random.default_rng(5).standard_normal((2, model.dims.tokens, d)).astype(np.float32)
    bw = model.encoder_block_weights(reps - 1)
    y = vtd.encoder_block(torch.from_numpy(x).to(cuda), bw, num_heads=heads, key_dim=dk,
                          use_mish=use_mish, dtype=mode)
    w64 = [torch.tensor(t.cpu().numpy(), dtype=torch.float64) for t in bw.values()]
    y64 = K.block_forward(w64, torch.tensor(x, dtype=torch.float64), use_mish).numpy()
    assert within(y.cpu().numpy(), y64, TOL[mode])
    # fresh copies: writing into one leaves the model's weights alone
    first = next(iter(bw.values()))
    first.add_(1.0)
    assert not torch.equal(first, next(iter(model.encoder_block_weights(reps - 1).values())))


def test_encoder_block_validation(vtd, cuda):
    case = K.CASES[0]
    B, N, d, heads, dk, q, use_mish = case
    w = [torch.from_numpy(t).to(cuda) for t in K.seeded_weights(case)]
    x = torch.from_numpy(K.seeded_inputs(case)[0]).to(cuda)
    kw = dict(num_heads=heads, key_dim=dk)
    with pytest.raises(ValueError, match="x must be a device tensor"):
        vtd.encoder_block(x.cpu(), w, **kw)
    with pytest.raises(ValueError, match="x must be float32"):
        vtd.encoder_block(x.double(), w, **kw)
    with pytest.raises(ValueError, match=r"\(B, N, d\)"):
        vtd.encoder_block(x[0], w, **kw)
    with pytest.raises(ValueError, match=r"12 \+ 2 q"):
        vtd.encoder_block(x, w[:-1], **kw)
    with pytest.raises(ValueError, match=r"weights\[2\] \(query kernel\) has shape"):
        vtd.encoder_block(x, w[:2] + [w[2][..., :2]] + w[3:], **kw)
    with pytest.raises(ValueError, match=r"weights\[9\] \(attention_output bias\) must be float32"):
        vtd.encoder_block(x, w[:9] + [w[9].double()] + w[10:], **kw)
    with pytest.raises(ValueError, match=r"weights\[12\] \(MLP 1 kernel\) must be a device tensor"):
        vtd.encoder_block(x, w[:12] + [w[12].cpu()] + w[13:], **kw)
    with pytest.raises(ValueError, match="dtype"):
        vtd.encoder_block(x, w, dtype="float32", **kw)
