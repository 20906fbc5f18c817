"""Model.gradients(image_gradient=True) and Model.image_gradient on the GPU, in both modes, over
model_grad_oracle.CASES: d loss / d images against the float64 whole model of
tests/image_grad_oracle.py fed the same float32 images and the device's own d loss / d logits
(the loss is not smooth, so the oracle starts there, as tests/test_gpu_model_gradients.py does),
at image_grad_oracle.bar -- the project's bars, which the CPU emulation of the whole chain stays
under half of (tests/test_image_grad_kat.py).  Every other output keeps its bits."""
import pytest
import torch

from tests import image_grad_oracle as G
from tests import model_grad_oracle as M
from tests.test_gpu_encoder_block import same_bits
from tests.test_gpu_head_backward import CASES, build, load_case, train_logits

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]

params = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def runs(vtd, cuda):
    """One device run per (case, mode), shared by the tests below."""
    from vision_transformer_detector_amd import loss as vloss
    cache = {}

    def get(name, batch, mode):
        key = (name, mode)
        if key in cache:
            return cache[key]
        kw, w, x, y = load_case(name, batch)
        model = build(vtd, kw, w, mode)
        xd = torch.from_numpy(x).to(cuda)
        out5_plain, plain = model.gradients(xd, y)
        out5, grads = model.gradients(xd, y, image_gradient=True)
        out5_b, grads_b = model.gradients(xd, y, image_gradient=True)
        out5_i, dimages = model.image_gradient(xd, y)
        cache[key] = dict(kw=kw, w=w, x=x, xd=xd, y=y, model=model, out5_plain=out5_plain,
                          plain=plain, out5=out5, grads=grads, out5_b=out5_b, grads_b=grads_b,
                          out5_i=out5_i, dimages=dimages, vloss=vloss)
        return cache[key]
    return get


def device_dlogits(vtd, r, mode):
    """d loss / d logits as Model.gradients forms it: the stage entries forward, then
    vtd_loss_grad at the training chain's logits."""
    from vision_transformer_detector_amd import encoder as enc
    k = dict(use_mish=True)
    k.update(r["kw"])
    model, vloss = r["model"], r["vloss"]
    x = vtd.patch_embedding(r["xd"], list(model.stem_weights().values()),
                            patch_size=k["patch_size"], dtype=mode)
    bdims = enc.block_dims(r["xd"].shape[0], model.dims.tokens, k["embedding_dim"],
                           k["encoder_num_heads"], k["encoder_key_dim"],
                           k["encoder_mlp_quantities"], k["use_mish"], mode)
    for i in range(k["encoder_repeat_times"]):
        x = enc.run(x, list(model.encoder_block_weights(i).values()), bdims)[0]
    logits = train_logits(model, x)
    return vloss.loss_and_grad(r["y"], logits, params=vloss.fused_loss_params(model.loss))[1]


@params
@cases
def test_images_entry_against_float64(vtd, runs, case, mode):
    r = runs(*case, mode)
    dlogits = device_dlogits(vtd, r, mode).cpu().numpy()
    _, g64, _ = G.model_image_grad64(r["kw"], r["w"], r["x"], dlogits)
    g = r["grads"]["images"]
    assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == r["x"].shape
    assert bool(torch.isfinite(g).all())
    err = G.rel_err(g.cpu().numpy(), g64)
    bar = G.bar(mode, case[0])
    print(f"{case[0]} B={case[1]} {mode}: images max |g - g64| / max |g64| {err:.3g} (bar {bar})")
    assert err <= bar


@params
@cases
def test_every_other_output_keeps_its_bits(runs, case, mode):
    """ "images" is the one last key; out5 and the weight entries equal those of the call
    without the flag, and a second call's, bit for bit; image_gradient() returns that entry."""
    r = runs(*case, mode)
    model = r["model"]
    assert list(r["plain"]) == model.weight_names()
    assert list(r["grads"]) == model.weight_names() + ["images"]
    assert same_bits(r["out5"], r["out5_plain"]) and same_bits(r["out5"], r["out5_b"])
    for n, g in r["plain"].items():
        assert same_bits(r["grads"][n], g), n
    for n, g in r["grads"].items():
        assert same_bits(r["grads_b"][n], g), n
    assert same_bits(r["out5_i"], r["out5"])
    assert same_bits(r["dimages"], r["grads"]["images"])


@params
def test_autograd_chain_reproduces_the_image_gradient(vtd, runs, mode):
    """patch_embedding(image_gradient=True) -> encoder_block x L -> model.detection_head ->
    my_custom_loss through torch autograd: images.grad has the bits of grads["images"]."""
    r = runs("tiny_mish", 3, mode)
    k = dict(use_mish=True)
    k.update(r["kw"])
    model = r["model"]
    images = r["xd"].clone().requires_grad_(True)
    y = vtd.patch_embedding(images, list(model.stem_weights().values()),
                            patch_size=k["patch_size"], dtype=mode, image_gradient=True)
    for i in range(k["encoder_repeat_times"]):
        y = vtd.encoder_block(y, list(model.encoder_block_weights(i).values()),
                              num_heads=k["encoder_num_heads"], key_dim=k["encoder_key_dim"],
                              use_mish=k["use_mish"], dtype=mode)
    logits = model.detection_head(y)
    loss = vtd.my_custom_loss(torch.from_numpy(r["y"]).to(images.device), logits)
    loss.backward()
    assert same_bits(loss.detach().reshape(1), r["out5"][:1])
    assert same_bits(images.grad, r["grads"]["images"])
    # the default leaves images.grad None through the same chain
    images2 = r["xd"].clone().requires_grad_(True)
    y = vtd.patch_embedding(images2, list(model.stem_weights().values()),
                            patch_size=k["patch_size"], dtype=mode)
    y.backward(torch.ones_like(y))
    assert images2.grad is None


@params
def test_dropout_model_same_step_same_bits(vtd, cuda, mode):
    """A model built with dropout and compiled with a seed: the same step gives the same bits,
    another step other ones, and the weight entries are those of the call without the flag."""
    import functools
    kw, w, x, y = load_case("tiny_mish", 3)
    model = vtd.create_vision_transformer_detector(**dict(kw, dropout=0.1), dtype=mode)
    model.set_weights(w)
    model.compile(loss=functools.partial(vtd.my_custom_loss), dropout_seed=7)
    xd = torch.from_numpy(x).to(cuda)
    out5, grads = model.gradients(xd, y, step=2, image_gradient=True)
    out5_b, dimages = model.image_gradient(xd, y, step=2)
    out5_p, plain = model.gradients(xd, y, step=2)
    _, other = model.image_gradient(xd, y, step=3)
    assert same_bits(out5, out5_b) and same_bits(out5, out5_p)
    assert same_bits(grads["images"], dimages)
    assert bool(torch.isfinite(dimages).all())
    for n, g in plain.items():
        assert same_bits(grads[n], g), n
    assert not same_bits(other, dimages)


def test_float32_mode_raises(vtd, cuda):
    kw, w, x, y = load_case("tiny_mish", 2)
    model = build(vtd, kw, w, "float32")
    xd = torch.from_numpy(x).to(cuda)
    with pytest.raises(ValueError, match="bf16x3.*bfloat16"):
        model.gradients(xd, y, image_gradient=True)
    with pytest.raises(ValueError, match="image_gradient.*bf16x3.*bfloat16"):
        model.image_gradient(xd, y)
