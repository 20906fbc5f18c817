"""Model.gradients on the GPU: every weight's gradient against the float64 whole model of
tests/model_grad_oracle.py, at the cases of tests/test_gpu_head_backward.py in both modes.

Two comparisons.  Stage-wise: each stage (stem, every block, head) against its float64 stage
fed the device's own stage input and upstream gradient, at the project's bars
(head_grad_oracle.BARS).  End to end: every gradient against the float64 whole model fed the
same float32 images and the device's d loss / d logits (the loss is not smooth, so the oracle
starts from the device's dlogits, as the head test does), at the bars the CPU emulation fixed
(model_grad_oracle.bar: the project's, or the tensor's own from OWN_BARS).  Measure per tensor:
max |g - g64| / max |g64|; the key biases, whose true gradient is zero, against
max sum_rows |dK64| as tests/test_gpu_encoder_block.py does.
"""
import pytest
import torch

from tests import block_grad_oracle as K
from tests import head_grad_oracle as H
from tests import model_grad_oracle as M
from tests.test_gpu_encoder_block import same_bits
from tests.test_gpu_head_backward import CASES, TOL, build, load_case, train_logits, within

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def runs(vtd, cuda):
    """One device run per (case, mode) -- Model.gradients twice, and the same chain stage by
    stage through the stage entries -- shared by the tests below."""
    from vision_transformer_detector_amd import encoder as enc
    from vision_transformer_detector_amd import loss as vloss
    from vision_transformer_detector_amd import stem
    cache = {}

    def get(name, batch, mode):
        key = (name, mode)
        if key in cache:
            return cache[key]
        kw, w, x, y = load_case(name, batch)
        k = dict(use_mish=True)
        k.update(kw)
        model = build(vtd, kw, w, mode)
        xd = torch.from_numpy(x).to(cuda)
        out5, grads = model.gradients(xd, y)
        out5_b, grads_b = model.gradients(xd, y)
        # the stages one by one
        p, d = k["patch_size"], k["embedding_dim"]
        heads, dk, q = k["encoder_num_heads"], k["encoder_key_dim"], k["encoder_mlp_quantities"]
        reps = k["encoder_repeat_times"]
        sw = list(model.stem_weights().values())
        bw = [list(model.encoder_block_weights(i).values()) for i in range(reps)]
        xs = [vtd.patch_embedding(xd, sw, patch_size=p, dtype=mode)]
        bdims = enc.block_dims(batch, model.dims.tokens, d, heads, dk, q, k["use_mish"], mode)
        for i in range(reps):
            xs.append(enc.run(xs[i], bw[i], bdims)[0])
        out5_h, hg = model.head_gradients(None, y, encoded=xs[reps])
        dys = [None] * (reps + 1)
        dys[reps] = hg["encoded_images"]
        bg = [None] * reps
        for i in range(reps - 1, -1, -1):
            _, bg[i], dys[i] = enc.run(xs[i], bw[i], bdims, dy=dys[i + 1], want_y=False)
        sdims = stem.stem_dims(batch, *k["input_shape"], p, d, mode)
        _, sg = stem.run(xd, sw, sdims, dx0=dys[0], want_x0=False)
        logits = train_logits(model, xs[reps])
        _, dlogits = vloss.loss_and_grad(y, logits, params=vloss.fused_loss_params(model.loss))
        inference = model(xd, training=False)
        torch.cuda.synchronize()
        cache[key] = dict(kw=kw, k=k, w=w, x=x, xd=xd, y=y, model=model, out5=out5, grads=grads,
                          out5_b=out5_b, grads_b=grads_b, sw=sw, bw=bw, xs=xs, dys=dys, hg=hg,
                          out5_h=out5_h, bg=bg, sg=sg, logits=logits, dlogits=dlogits,
                          inference=inference)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def oracle(runs):
    """The float64 whole model per (case, mode), fed the device's d loss / d logits."""
    cache = {}

    def get(name, batch, mode):
        key = (name, mode)
        if key not in cache:
            r = runs(name, batch, mode)
            cache[key] = M.model_grads(r["kw"], r["w"], r["x"], r["dlogits"].cpu().numpy())
        return cache[key]
    return get


params = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])


@params
@cases
def test_keys_shapes_and_repeat_calls(runs, case, mode):
    r = runs(*case, mode)
    model = r["model"]
    assert list(r["grads"]) == model.weight_names()
    for n, g in r["grads"].items():
        assert tuple(g.shape) == tuple(model.weight_shapes[n]), n
        assert g.dtype == torch.float32 and g.is_cuda and bool(torch.isfinite(g).all()), n
    assert tuple(r["grads"][M.POS].shape) == (model.dims.tokens, 1)
    assert r["out5"].shape == r["out5_h"].shape and same_bits(r["out5"], r["out5_b"])
    for n, g in r["grads"].items():
        assert same_bits(g, r["grads_b"][n]), n


@params
@cases
def test_gradients_equal_the_stage_calls_bit_for_bit(runs, case, mode):
    """Model.gradients against patch_embedding, encoder.run per block, head_gradients on the
    last block's output, and the stage backward calls in reverse: the same bits everywhere, the
    head entries those of head_gradients(images, y, encoded=x_L)."""
    r = runs(*case, mode)
    model = r["model"]
    assert same_bits(r["out5"], r["out5_h"])
    stage = list(r["sg"]) + [g for blk in r["bg"] for g in blk]
    stage += [r["hg"][n] for n in model.head_weight_names()]
    assert len(stage) == len(r["grads"])
    for (n, g), s in zip(r["grads"].items(), stage):
        assert same_bits(g, s), n
    assert list(r["hg"]) == model.head_weight_names() + ["encoded_images"]


@params
@cases
def test_stages_against_float64(runs, case, mode):
    """Each stage against its float64 stage fed the device's own input and upstream gradient,
    at the project's bars."""
    r = runs(*case, mode)
    k, bars = r["k"], H.BARS[mode]
    stem_names, block_names, _ = M.split_names(r["kw"])
    worst = {}
    _, g64 = H.head_grads(r["w"], r["xs"][-1].cpu().numpy(), r["dlogits"].cpu().numpy(),
                          k["use_mish"])
    for n, g in r["hg"].items():
        worst[n] = H.rel_err(g.cpu().numpy(), g64[n])
    for i, names in enumerate(block_names):
        bw = [t.cpu().numpy() for t in r["bw"][i]]
        _, b64, dx64, den = K.block_grads(bw, r["xs"][i].cpu().numpy(),
                                          r["dys"][i + 1].cpu().numpy(), k["use_mish"])
        errs = K.rel_errors([g.cpu().numpy() for g in r["bg"][i]], r["dys"][i].cpu().numpy(), b64,
                            dx64, den, k["encoder_mlp_quantities"])
        worst.update({names[j]: v for j, v in enumerate(list(errs.values())[:-1])})
        worst[f"x_{i}"] = errs["x"]
    _, s64 = M.stem_grads([t.cpu().numpy() for t in r["sw"]], r["x"], k["patch_size"],
                          r["dys"][0].cpu().numpy())
    for n, g, ref in zip(stem_names, r["sg"], s64):
        worst[n] = H.rel_err(g.cpu().numpy(), ref)
    top = max(worst, key=worst.get)
    print(f"{case[0]} B={case[1]} {mode}: stage-wise worst {worst[top]:.3g} ({top})")
    for n, v in worst.items():
        assert v <= bars, f"{n}: {v:.3g} > {bars}"


@params
@cases
def test_end_to_end_against_float64(runs, oracle, case, mode):
    r = runs(*case, mode)
    _, g64, _, den = oracle(*case, mode)
    assert list(g64) == list(r["grads"])
    errs = M.rel_errors({n: g.cpu().numpy() for n, g in r["grads"].items()}, g64, den)
    top = max(errs, key=lambda n: errs[n] / M.bar(mode, n))
    print(f"{case[0]} B={case[1]} {mode}: end-to-end worst {errs[top]:.3g} ({top}, bar "
          f"{M.bar(mode, top)}); " + ", ".join(f"{n} {v:.2g}" for n, v in errs.items()))
    for n, v in errs.items():
        assert v <= M.bar(mode, n), f"{n}: {v:.3g} > {M.bar(mode, n)}"


@params
@cases
def test_training_chain_logits(runs, oracle, case, mode):
    """The training chain's logits: within the mode's forward tolerance of model(images) and of
    the float64 whole model."""
    r = runs(*case, mode)
    logits64 = oracle(*case, mode)[0]
    logits = r["logits"].cpu().numpy()
    assert within(logits, r["inference"].cpu().numpy(), TOL[mode])
    assert within(logits, logits64, TOL[mode])


@params
def test_autograd_chain_reproduces_the_encoder_entries(vtd, runs, mode):
    """patch_embedding -> encoder_block x L through torch autograd, from the head's
    d loss / d encoded_images: the bits of Model.gradients' stem and encoder entries."""
    r = runs("tiny_mish", 3, mode)
    k = r["k"]
    sw = [t.clone().requires_grad_(True) for t in r["sw"]]
    bw = [[t.clone().requires_grad_(True) for t in blk] for blk in r["bw"]]
    y = vtd.patch_embedding(r["xd"], sw, patch_size=k["patch_size"], dtype=mode)
    for blk in bw:
        y = vtd.encoder_block(y, blk, num_heads=k["encoder_num_heads"],
                              key_dim=k["encoder_key_dim"], use_mish=k["use_mish"], dtype=mode)
    assert same_bits(y.detach(), r["xs"][-1])
    y.backward(r["hg"]["encoded_images"])
    leaves = sw + [t for blk in bw for t in blk]
    for (n, g), t in zip(r["grads"].items(), leaves):
        assert same_bits(t.grad, g), n


def test_float32_mode_raises(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = build(vtd, kw, w, "float32")
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.gradients(torch.from_numpy(x).to(cuda), y)


def test_needs_a_compiled_loss(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = vtd.create_vision_transformer_detector(**kw, dtype="bf16x3")
    with pytest.raises(ValueError, match="compile"):
        model.gradients(torch.from_numpy(x).to(cuda), y)
