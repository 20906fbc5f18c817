"""The yardstick of vtd_stem_image_grad and Model.gradients(image_gradient=True): d loss / d
images in float64, and the CPU emulation of the device's chain of roundings.

The stem is linear in the images: x0 = extract(images) W + b + pos, so
    d loss / d images = unpatch(dx0 W^T),
`unpatch` the adjoint of tf.image.extract_patches(SAME).  The adjoint is built from the numpy
oracle's own forward, not from an index formula: the forward applied to an image that holds
1 .. H W C says which image element every patch column copied (0: a pad), and the adjoint puts
each patch column's gradient back there.  Every image element is copied exactly once, so nothing
is added up; the gradient that falls on a pad is dropped.

Measure and bars (the rule of tests/model_grad_oracle.py): max |g - g64| / max |g64| of the
tensor, against head_grad_oracle.BARS (2e-4 bf16x3, 5e-2 bfloat16) provided the CPU emulation
stays at or under half of that in every case; where it does not, the tensor at that case gets a
bar of its own in OWN_BARS, twice the emulation's worst rounded up to two digits.
tests/test_image_grad_kat.py measures the emulation at every case and holds the table to it; no
bar comes from a device's output.
"""
import numpy as np
import torch

from oracle import vtd_numpy as V
from tests import block_grad_oracle as K
from tests import head_grad_oracle as H
from tests import model_grad_oracle as M

BARS = H.BARS

# (B, H, W, p, d[, C]) of tests/test_gpu_stem_image_grad.py; C = 3 where it is left out
STEM_CASES = list(M.STEM_CASES) + [
    (1, 5, 7, 2, 8),              # odd sizes
    (1, 3, 5, 8, 8),              # one token, a patch larger than the image
    (2, 34, 34, 17, 28),          # patch_dim 867: the reference's own patch and width
    (2, 9, 9, 3, 16, 1),          # C = 1
    (1, 8, 8, 4, 8, 4),           # C = 4
]
MODEL_CASES = M.CASES

# mode -> case id -> bar of "images": the cases whose emulated error passes half the project's
# bar; the value is twice the emulation's worst, rounded up to two digits.  None in either mode:
# the emulation's worst is, for the stem alone, 8.7e-6 bf16x3 (B3_20x12_p4_d6) and 4.8e-3
# bfloat16 (B1_3x5_p8_d8); for the whole model, 1.7e-5 bf16x3 and 8.4e-3 bfloat16 (both at
# tiny_gelu) -- the roundings of the head and of every block reach the first block's input
# gradient, which the stem only multiplies by W^T, and stay well under half of 5e-2.
OWN_BARS = {
    "bf16x3": {},
    "bfloat16": {},
}


def parse(case):
    """(B, H, W, p, d, C) of a case tuple."""
    return tuple(case[:5]) + ((case[5] if len(case) > 5 else 3),)


def stem_case_id(case):
    B, Hh, Ww, p, d, C = parse(case)
    return f"B{B}_{Hh}x{Ww}_p{p}_d{d}" + ("" if C == 3 else f"_C{C}")


def bar(mode, case_id):
    return OWN_BARS[mode].get(case_id, BARS[mode])


# ------------------------------------------------------------------ the adjoint
def source_index(shape, p):
    """(N, P) int64: the 1-based flat index into one (H, W, C) image of the element every patch
    column holds, 0 for a pad -- the numpy oracle's forward applied to 1 .. H W C."""
    Hh, Ww, C = shape
    marks = np.arange(1, Hh * Ww * C + 1, dtype=np.float64).reshape(1, Hh, Ww, C)
    return V.extract_patches_same(marks, p)[0].astype(np.int64)


def unpatch(dP, shape, p):
    """The adjoint of extract_patches_same: dP (B, N, P) -> (B, H, W, C), same dtype."""
    dP = np.asarray(dP)
    idx = source_index(shape, p)
    assert dP.shape[1:] == idx.shape
    keep = idx > 0
    # every image element exactly once: the assignment below adds nothing up
    assert np.array_equal(np.sort(idx[keep]), np.arange(1, int(np.prod(shape)) + 1))
    out = np.zeros((dP.shape[0], int(np.prod(shape))), dP.dtype)
    out[:, idx[keep] - 1] = dP[:, keep]
    return out.reshape((dP.shape[0],) + tuple(shape))


# ------------------------------------------------------------------ the stem alone
def seeded(case, seed=0):
    """(W (P, d), dx0 (B, N, d)) float32: the Keras initialiser's scale, dx0 ~ N(0, 1)."""
    B, Hh, Ww, p, d, C = parse(case)
    rng = np.random.default_rng([B, Hh, Ww, p, d, C, seed, 1])
    gh, gw = V.token_grid(Hh, Ww, p)
    P = p * p * C
    lim = np.sqrt(6.0 / (P + d))
    w = rng.uniform(-lim, lim, (P, d)).astype(np.float32)
    dx0 = rng.standard_normal((B, gh * gw, d)).astype(np.float32)
    return w, dx0


def stem_image_grad64(w, dx0, shape, p):
    """d loss / d images (B, H, W, C) float64 from W (P, d) and dx0 (B, N, d); shape = (H, W, C)."""
    dP = np.asarray(dx0, np.float64) @ np.asarray(w, np.float64).T
    return unpatch(dP, shape, p)


def emulated_stem_image_grad(w, dx0, shape, p, mode):
    """float32, as the device forms it: dP = dx0 W^T on the mode's operands with float32 sums
    (head_grad_oracle.mm), then the copy."""
    g = torch.tensor(np.asarray(dx0, np.float32))
    B, N, d = g.shape
    dP = H.mm(g.reshape(B * N, d), torch.tensor(np.asarray(w, np.float32)).T, mode)
    return unpatch(dP.numpy().reshape(B, N, -1), shape, p)


def rel_err(got, ref):
    return H.rel_err(got, ref)


# ------------------------------------------------------------------ the whole model
def model_image_grad64(kw, weights, images, dlogits):
    """(logits, dimages, dx0) in float64 from d loss / d logits: model_grad_oracle's autograd to
    the first block's input, then the stem's adjoint."""
    k = V.resolve_kwargs(**kw)
    logits, _, dxs, _ = M.model_grads(kw, weights, images, dlogits)
    dimg = stem_image_grad64(weights[M.WP], dxs[0], tuple(np.asarray(images).shape[1:]),
                             k["patch_size"])
    return logits, dimg, dxs[0]


def model_forward64(kw, weights, images):
    """logits float64 of float64 images (the central differences' forward)."""
    k = V.resolve_kwargs(**kw)
    wt = {n: torch.tensor(np.asarray(v), dtype=torch.float64) for n, v in weights.items()}
    pt = torch.tensor(V.extract_patches_same(np.asarray(images, np.float64), k["patch_size"]))
    return M.model_forward(kw, wt, pt).numpy()


def emulated_model_image_grad(kw, weights, images, dlogits, mode):
    """float32: the device's chain on the CPU as model_grad_oracle.emulated_model_backward runs
    it (which does not return the first block's input gradient, so its few lines are restated),
    then the emulated stem image gradient."""
    k = V.resolve_kwargs(**kw)
    stem, blocks, _ = M.split_names(kw)
    heads, dk, use_mish = k["encoder_num_heads"], k["encoder_key_dim"], k["use_mish"]
    xs = [M.emulated_stem_forward([weights[n] for n in stem], images, k["patch_size"], mode)]
    for names in blocks:
        y, _, _ = K.emulated_block_backward([weights[n] for n in names], xs[-1],
                                            np.zeros_like(xs[-1]), heads, dk, use_mish, mode)
        xs.append(y)
    _, hg = H.emulated_head_backward(weights, xs[-1], dlogits, use_mish, mode)
    dy = hg["encoded_images"]
    for i in range(len(blocks) - 1, -1, -1):
        _, _, dy = K.emulated_block_backward([weights[n] for n in blocks[i]], xs[i], dy, heads,
                                             dk, use_mish, mode)
    return emulated_stem_image_grad(weights[M.WP], dy, tuple(np.asarray(images).shape[1:]),
                                    k["patch_size"], mode)
