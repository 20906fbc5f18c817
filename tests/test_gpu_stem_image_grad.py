"""vtd_stem_image_grad and patch_embedding(image_gradient=True) on the GPU, in both modes, at
the cases (B, H, W, p, d[, C]) of tests/image_grad_oracle.py:

  model_grad_oracle.STEM_CASES   pad on one axis and on both; patch_dim 147, not a multiple of
                                 8; d % 4 != 0; 4096 rows; patch_dim and d of 768
  (1, 5, 7, 2, 8)                odd sizes
  (1, 3, 5, 8, 8)                one token, a patch larger than the image
  (2, 34, 34, 17, 28)            patch_dim 867, runs of 51 floats: the reference's patch and width
  (2, 9, 9, 3, 16, C=1), (1, 8, 8, 4, 8, C=4)

Designed operands (exact): integers that bf16 holds exactly, so the split mode's lo pieces are
zero, with every partial sum below 2^24, so fp32 is exact in any summation order and the result
must equal the int64 product bit for bit.  "residues": W[k][j] = (7k + 3j) % 13 - 6, dx0[m][j] =
(5m + j) % 9 - 4, |sum| <= 24 d <= 18,432.  "address": dx0[m] = (1, m % 97, 0, ...), W[k] =
(k % 101, 128, 0, ...), so dP[m][k] = k % 101 + 128 (m % 97) < 2^14 decodes to (row, patch
column): a misplaced pixel shows as its coordinates.
Seeded operands: against float64 at image_grad_oracle.bar (the project's bars; the CPU
emulation stays under half of them at every case, tests/test_image_grad_kat.py).
"""
import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import image_grad_oracle as G
from tests import model_grad_oracle as M
from tests.test_gpu_encoder_block import GUARD, same_bits

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]

params = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", G.STEM_CASES, ids=G.stem_case_id)


@pytest.fixture(scope="module")
def stem(cuda):
    from vision_transformer_detector_amd import stem
    return stem


def shape_of(case):
    B, Hh, Ww, p, d, C = G.parse(case)
    gh, gw = V.token_grid(Hh, Ww, p)
    return B, Hh, Ww, p, d, C, gh * gw, p * p * C


def designed(case, design):
    """(W (P, d), dx0 (B, N, d)) int64."""
    B, Hh, Ww, p, d, C, N, P = shape_of(case)
    k, m, j = np.arange(P)[:, None], np.arange(B * N)[:, None], np.arange(d)[None, :]
    if design == "residues":
        w, dx0 = (7 * k + 3 * j) % 13 - 6, (5 * m + j) % 9 - 4
    else:
        w, dx0 = np.zeros((P, d), np.int64), np.zeros((B * N, d), np.int64)
        w[:, 0], w[:, 1] = k[:, 0] % 101, 128
        dx0[:, 0], dx0[:, 1] = 1, m[:, 0] % 97
    return w.astype(np.int64), dx0.reshape(B, N, d).astype(np.int64)


def nan_guarded(shape, device):
    """(tensor, buffer): a float32 tensor inside a NaN-filled float32 buffer, GUARD bytes of it
    on either side."""
    n, g = int(np.prod(shape)), GUARD // 4
    buf = torch.full((n + 2 * g,), float("nan"), dtype=torch.float32, device=device)
    return buf[g:g + n].view(shape), buf


def run(stem, cuda, case, mode, w, dx0, out=None, poison=0xFF):
    B, Hh, Ww, p, d, C, N, P = shape_of(case)
    dims = stem.stem_dims(B, Hh, Ww, C, p, d, mode)
    ws = torch.full((stem.image_grad_workspace_bytes(dims),), poison, dtype=torch.uint8,
                    device=cuda)
    wd = torch.from_numpy(np.asarray(w, np.float32)).to(cuda)
    gd = torch.from_numpy(np.asarray(dx0, np.float32)).to(cuda)
    return stem.image_grad(gd, wd, dims, ws=ws, out=out), dims, wd, gd


@params
@cases
@pytest.mark.parametrize("design", ["residues", "address"])
def test_designed_operands_are_exact(stem, cuda, case, mode, design):
    B, Hh, Ww, p, d, C, N, P = shape_of(case)
    w, dx0 = designed(case, design)
    dP = dx0 @ w.T                                                        # int64, exact
    # integers up to 256 are bf16 values; the sum of the products' magnitudes bounds every
    # partial sum in any order
    assert int(np.abs(w).max()) <= 256 and int(np.abs(dx0).max()) <= 256
    assert int((np.abs(dx0).reshape(-1, d) @ np.abs(w).T).max()) < 1 << 24
    want = G.unpatch(dP, (Hh, Ww, C), p)
    got, *_ = run(stem, cuda, case, mode, w, dx0)
    got = got.cpu()
    ok = torch.equal(got, torch.from_numpy(want.astype(np.float32)))
    if not ok and design == "address":
        bad = np.argwhere(got.numpy() != want)[0]
        v, e = int(got.numpy()[tuple(bad)]), int(want[tuple(bad)])
        print(f"image element {tuple(bad)}: holds (row % 97, column % 101) = ({v // 128}, "
              f"{v % 128}), expected ({e // 128}, {e % 128})")
    assert ok


@params
@cases
def test_every_element_written_and_nothing_else(stem, cuda, case, mode):
    """dimages inside a NaN-filled buffer with guards on both sides, over a NaN-poisoned
    workspace: no NaN is left inside -- every element was written, from written sources --, the
    guards keep their bits, and the values are those of a plain call."""
    B, Hh, Ww, p, d, C, N, P = shape_of(case)
    w, dx0 = G.seeded(case)
    out, buf = nan_guarded((B, Hh, Ww, C), cuda)
    before = buf.clone()
    got, *_ = run(stem, cuda, case, mode, w, dx0, out=out)
    plain, *_ = run(stem, cuda, case, mode, w, dx0, poison=0)
    torch.cuda.synchronize()
    g = GUARD // 4
    assert got.data_ptr() == out.data_ptr()
    assert not bool(torch.isnan(buf[g:-g]).any())
    assert same_bits(buf[:g], before[:g]) and same_bits(buf[-g:], before[-g:])
    assert same_bits(got, plain)


@pytest.fixture(scope="module")
def seeded_runs(stem, cuda):
    """One float64 oracle per case; per (case, mode): the entry twice, with a vtd_stem_backward
    call before and after."""
    cache, oracle = {}, {}

    def get(case, mode):
        key = (case, mode)
        if key in cache:
            return cache[key]
        B, Hh, Ww, p, d, C, N, P = shape_of(case)
        if case not in oracle:
            w, dx0 = G.seeded(case)
            oracle[case] = (w, dx0, G.stem_image_grad64(w, dx0, (Hh, Ww, C), p))
        w, dx0, g64 = oracle[case]
        rng = np.random.default_rng(3)
        images = torch.from_numpy(rng.uniform(0, 1, (B, Hh, Ww, C)).astype(np.float32)).to(cuda)
        sw = [torch.from_numpy(rng.uniform(-.05, .05, (N, 1)).astype(np.float32)).to(cuda), None,
              torch.from_numpy(rng.uniform(-.05, .05, (d,)).astype(np.float32)).to(cuda)]
        first, dims, wd, gd = run(stem, cuda, case, mode, w, dx0)
        sw[1] = wd
        before = stem.run(images, sw, dims, dx0=gd)
        second = stem.image_grad(gd, wd, dims)
        after = stem.run(images, sw, dims, dx0=gd)
        torch.cuda.synchronize()
        cache[key] = dict(g64=g64, first=first, second=second, before=before, after=after,
                          images=images, sw=sw, dx0=gd, dims=dims)
        return cache[key]
    return get


@params
@cases
def test_seeded_against_float64(seeded_runs, case, mode):
    r = seeded_runs(case, mode)
    got = r["first"]
    assert got.dtype == torch.float32 and tuple(got.shape) == r["g64"].shape
    err = G.rel_err(got.cpu().numpy(), r["g64"])
    bar = G.bar(mode, G.stem_case_id(case))
    print(f"{G.stem_case_id(case)} {mode}: max |g - g64| / max |g64| {err:.3g} (bar {bar})")
    assert err <= bar


@params
@cases
def test_repeat_calls_and_stem_backward_undisturbed(seeded_runs, case, mode):
    r = seeded_runs(case, mode)
    assert same_bits(r["first"], r["second"])
    (x0a, ga), (x0b, gb) = r["before"], r["after"]
    assert same_bits(x0a, x0b)
    for a, b in zip(ga, gb):
        assert same_bits(a, b)


@params
def test_dimages_off_a_16_byte_boundary_takes_the_generic_path(stem, seeded_runs, cuda, mode):
    """A case whose sizes allow the vector path, written at a base 4 bytes past a 16-B
    boundary: the bits of the aligned call."""
    case = M.STEM_CASES[2]                                   # 80 x 80, p 4: W C, p C % 4 == 0
    r = seeded_runs(case, mode)
    flat = torch.empty(r["first"].numel() + 1, dtype=torch.float32, device=cuda)
    shifted = flat[1:].view(r["first"].shape)
    assert shifted.data_ptr() % 16 == 4
    stem.image_grad(r["dx0"], r["sw"][1], r["dims"], out=shifted)
    assert same_bits(shifted, r["first"])


@params
@cases
def test_patch_embedding_fills_images_grad(seeded_runs, case, mode):
    """image_gradient=True: images.grad has the entry's bits and the weight gradients those of
    the default call; the default leaves images.grad None."""
    import vision_transformer_detector_amd as vtd
    r = seeded_runs(case, mode)
    p = G.parse(case)[3]
    grads = {}
    for flag in (True, False):
        w = [t.clone().requires_grad_(True) for t in r["sw"]]
        images = r["images"].clone().requires_grad_(True)
        kw = dict(image_gradient=True) if flag else {}
        x0 = vtd.patch_embedding(images, w, patch_size=p, dtype=mode, **kw)
        assert same_bits(x0.detach(), r["before"][0])
        x0.backward(r["dx0"])
        grads[flag] = (images.grad, [t.grad for t in w])
    assert grads[False][0] is None
    assert same_bits(grads[True][0], r["first"])
    for a, b, c in zip(grads[True][1], grads[False][1], r["before"][1]):
        assert same_bits(a, b) and same_bits(a, c)
    # images that do not require grad: nothing to fill, nothing raised
    w = [t.clone().requires_grad_(True) for t in r["sw"]]
    vtd.patch_embedding(r["images"], w, patch_size=p, dtype=mode,
                        image_gradient=True).backward(r["dx0"])
    assert r["images"].grad is None and same_bits(w[1].grad, r["before"][1][1])
