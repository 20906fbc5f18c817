"""Model.gradients / head_gradients with a compiled dropout seed on the GPU: the whole training
graph with the reference's dropout -- block i at site_base i (1 + q), the head at L (1 + q).

As tests/test_gpu_model_gradients.py: Model.gradients equals the stage calls bit for bit, and
each stage is held against its masked float64 stage (tests/dropout_oracle.py's block,
tests/model_dropout_oracle.py's head, the undropped stem) fed the device's own stage input and
upstream gradient, at the project's bars (head_grad_oracle.BARS).  There is no end-to-end bar of
its own: the stage bars and the bit identity cover the chain.
"""
import functools

import pytest
import torch

from tests import block_grad_oracle as K
from tests import dropout_oracle as D
from tests import head_grad_oracle as H
from tests import model_dropout_oracle as R
from tests import model_grad_oracle as M
from tests.test_gpu_encoder_block import same_bits

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]
STEP = 1

modes = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
rates = pytest.mark.parametrize("rate", R.RATES)


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


def build(vtd, kw, w, mode, **compile_kw):
    model = vtd.create_vision_transformer_detector(**kw, dtype=mode)
    model.set_weights(w)
    model.compile(loss=functools.partial(vtd.my_custom_loss), **compile_kw)
    return model


@pytest.fixture(scope="module")
def runs(vtd, cuda):
    """One device run per (case, mode, rate): Model.gradients twice on a seeded dropout model,
    and the same chain stage by stage through the stage entries."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import encoder as enc
    from vision_transformer_detector_amd import loss as vloss
    from vision_transformer_detector_amd import stem
    cache = {}

    def get(name, batch, mode, rate):
        key = (name, mode, rate)
        if key in cache:
            return cache[key]
        kw, w, x, y = R.load_case(name, batch)
        k = dict(use_mish=True)
        k.update(kw)
        model = build(vtd, dict(kw, dropout=rate), w, mode, dropout_seed=R.SEED)
        assert model.dropout_seed == R.SEED
        xd = torch.from_numpy(x).to(cuda)
        out5, grads = model.gradients(xd, y, step=STEP)
        out5_b, grads_b = model.gradients(xd, y, step=STEP)
        p, d = k["patch_size"], k["embedding_dim"]
        heads, dk, q = k["encoder_num_heads"], k["encoder_key_dim"], k["encoder_mlp_quantities"]
        reps = k["encoder_repeat_times"]
        sw = list(model.stem_weights().values())
        bw = [list(model.encoder_block_weights(i).values()) for i in range(reps)]
        xs = [vtd.patch_embedding(xd, sw, patch_size=p, dtype=mode)]
        bdims = enc.block_dims(batch, model.dims.tokens, d, heads, dk, q, k["use_mish"], mode)
        drops = [L.VtdBlockDropout(seed=R.SEED, step=STEP, site_base=i * (1 + q), rate=rate)
                 for i in range(reps)]
        for i in range(reps):
            xs.append(enc.run(xs[i], bw[i], bdims, drop=drops[i])[0])
        # the head: the autograd op on the last block's output, then the loss gradient
        x_last = xs[reps].clone().requires_grad_(True)
        hw = model.head_weights()
        for t in hw.values():
            t.requires_grad_(True)
        logits = model.detection_head(x_last, hw, seed=R.SEED, step=STEP)
        out5_s, dlogits = vloss.loss_and_grad(y, logits.detach(),
                                              params=vloss.fused_loss_params(model.loss))
        logits.backward(dlogits)
        hg = {n: t.grad for n, t in hw.items()}
        dys = [None] * (reps + 1)
        dys[reps] = x_last.grad
        bg = [None] * reps
        for i in range(reps - 1, -1, -1):
            _, bg[i], dys[i] = enc.run(xs[i], bw[i], bdims, dy=dys[i + 1], want_y=False,
                                       drop=drops[i])
        sdims = stem.stem_dims(batch, *k["input_shape"], p, d, mode)
        _, sg = stem.run(xd, sw, sdims, dx0=dys[0], want_x0=False)
        out5_h, hgrads = model.head_gradients(None, y, encoded=xs[reps], step=STEP)
        torch.cuda.synchronize()
        cache[key] = dict(kw=kw, k=k, w=w, x=x, xd=xd, y=y, model=model, out5=out5, grads=grads,
                          out5_b=out5_b, grads_b=grads_b, sw=sw, bw=bw, xs=xs, dys=dys, hg=hg,
                          bg=bg, sg=sg, logits=logits.detach(), dlogits=dlogits, out5_s=out5_s,
                          out5_h=out5_h, hgrads=hgrads)
        return cache[key]
    return get


@rates
@modes
@cases
def test_gradients_equal_the_stage_calls_bit_for_bit(runs, case, mode, rate):
    """Model.gradients(step=t) against patch_embedding, encoder.run per block with the block's
    VtdBlockDropout, detection_head on the last block's output, the loss gradient, and the stage
    backward calls in reverse: the same bits everywhere, twice."""
    r = runs(*case, mode, rate)
    model = r["model"]
    assert list(r["grads"]) == model.weight_names()
    assert same_bits(r["out5"], r["out5_s"]) and same_bits(r["out5"], r["out5_b"])
    stage = list(r["sg"]) + [g for blk in r["bg"] for g in blk]
    stage += [r["hg"][n] for n in model.head_weight_names()]
    assert len(stage) == len(r["grads"])
    for (n, g), s in zip(r["grads"].items(), stage):
        assert bool(torch.isfinite(g).all()), n
        assert same_bits(g, s), n
        assert same_bits(g, r["grads_b"][n]), n


@rates
@modes
@cases
def test_head_gradients_equal_detection_head_and_the_loss(runs, case, mode, rate):
    r = runs(*case, mode, rate)
    model = r["model"]
    assert list(r["hgrads"]) == model.head_weight_names() + ["encoded_images"]
    assert same_bits(r["out5_h"], r["out5_s"])
    for n in model.head_weight_names():
        assert same_bits(r["hgrads"][n], r["hg"][n]), n
    assert same_bits(r["hgrads"]["encoded_images"], r["dys"][-1])
    # another step: other masks
    out5, _ = model.head_gradients(None, r["y"], encoded=r["xs"][-1], step=STEP + 1)
    assert not same_bits(out5, r["out5_h"])


@rates
@modes
@cases
def test_stages_against_masked_float64(runs, case, mode, rate):
    """Each stage against its masked float64 stage fed the device's own input and upstream
    gradient, at the project's bars."""
    r = runs(*case, mode, rate)
    k, bars, b = r["k"], H.BARS[mode], case[1]
    c = D.inv_keep(rate)
    stem_names, block_names, _ = M.split_names(r["kw"])
    bmasks, hmasks = R.model_masks(r["kw"], b, rate, R.SEED, STEP)
    worst = {}
    _, g64 = R.head_grads(r["w"], r["xs"][-1].cpu().numpy(), r["dlogits"].cpu().numpy(),
                          k["use_mish"], hmasks, c)
    for n, g in r["hg"].items():
        worst[n] = H.rel_err(g.cpu().numpy(), g64[n])
    worst["encoded_images"] = H.rel_err(r["dys"][-1].cpu().numpy(), g64["encoded_images"])
    for i, names in enumerate(block_names):
        bw = [t.cpu().numpy() for t in r["bw"][i]]
        _, b64, dx64, den = D.chain_grads([bw], r["xs"][i].cpu().numpy(),
                                          r["dys"][i + 1].cpu().numpy(), k["use_mish"],
                                          [bmasks[i]], c)
        errs = K.rel_errors([g.cpu().numpy() for g in r["bg"][i]], r["dys"][i].cpu().numpy(),
                            b64[0], dx64, den[0], k["encoder_mlp_quantities"])
        worst.update({names[j]: v for j, v in enumerate(list(errs.values())[:-1])})
        worst[f"x_{i}"] = errs["x"]
    _, s64 = M.stem_grads([t.cpu().numpy() for t in r["sw"]], r["x"], k["patch_size"],
                          r["dys"][0].cpu().numpy())
    for n, g, ref in zip(stem_names, r["sg"], s64):
        worst[n] = H.rel_err(g.cpu().numpy(), ref)
    top = max(worst, key=worst.get)
    print(f"{case[0]} B={b} {mode} rate {rate}: stage-wise worst {worst[top]:.3g} ({top})")
    for n, v in worst.items():
        assert v <= bars, f"{n}: {v:.3g} > {bars}"


@modes
@cases
def test_without_a_seed_gradients_are_the_dropout_none_models(vtd, cuda, runs, case, mode):
    """A dropout model with no compiled seed runs today's graph: the bits of a dropout=None model
    with the same weights, whatever `step` says; and they are not the seeded model's."""
    r = runs(*case, mode, 0.5)
    plain = build(vtd, r["kw"], r["w"], mode)
    want5, want = plain.gradients(r["xd"], r["y"])
    for model, step in ((build(vtd, dict(r["kw"], dropout=0.5), r["w"], mode), 3),
                        (build(vtd, dict(r["kw"], dropout=0.0), r["w"], mode, dropout_seed=R.SEED), 3),
                        (build(vtd, r["kw"], r["w"], mode, dropout_seed=R.SEED), 0)):
        out5, grads = model.gradients(r["xd"], r["y"], step=step)
        assert same_bits(out5, want5)
        for n, g in want.items():
            assert same_bits(grads[n], g), n
        h5, hg = model.head_gradients(r["xd"], r["y"], step=step)
        p5, pg = plain.head_gradients(r["xd"], r["y"])
        assert same_bits(h5, p5) and all(same_bits(hg[n], pg[n]) for n in pg)
    assert not same_bits(r["out5"], want5)


def test_compile_keeps_and_clears_the_seed(vtd, cuda):
    kw, w, x, y = R.load_case("tiny_mish", 2)
    model = build(vtd, dict(kw, dropout=0.1), w, "bf16x3", dropout_seed=7)
    assert model.dropout_seed == 7
    xd = torch.from_numpy(x).to(cuda)
    a5, _ = model.gradients(xd, y, step=4)
    b5, _ = model.gradients(xd, y, step=5)
    assert not same_bits(a5, b5)
    model.compile(loss=model.loss)                        # a later compile without it clears it
    assert model.dropout_seed is None
    c5, _ = model.gradients(xd, y, step=4)
    assert same_bits(c5, build(vtd, kw, w, "bf16x3").gradients(xd, y)[0])
    for bad in (-1, 1 << 64, 1.5, "3", True):
        with pytest.raises(ValueError, match="dropout_seed"):
            model.compile(loss=model.loss, dropout_seed=bad)
    # inference is untouched by the seed
    seeded = build(vtd, dict(kw, dropout=0.1), w, "bf16x3", dropout_seed=7)
    assert same_bits(seeded(xd), build(vtd, kw, w, "bf16x3")(xd))
