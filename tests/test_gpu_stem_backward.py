"""vtd_stem_backward and patch_embedding on the GPU against the float64 stem of
tests/model_grad_oracle.py, in both modes.

Cases (B, H, W, p, d), C = 3:
  (3, 40, 36, 8, 24)     the tiny_mish stem: SAME pad on one axis, N = 25
  (2, 33, 50, 7, 20)     the tiny_gelu stem: patch_dim 147, not a multiple of 8; pad on both axes
  (2, 80, 80, 4, 32)     N = 400
  (16, 64, 64, 4, 64)    4096 rows: several msplit ranges of the weight gradient, many waves
  (2, 48, 32, 16, 768)   several 16-B loads per lane (d_p / 8 = 96 chunks), patch_dim 768
  (3, 20, 12, 4, 6)      d % 4 != 0: the generic path of stem_grad_rows_kernel

With seeded dx0 ~ N(0, 1): x0 within the modes' forward tolerances; dW and db within the project's
bars (head_grad_oracle.BARS; the CPU emulation stays under half, tests/test_model_grad_kat.py);
dpos within c 2^-24 sum_b sum_j |dx0| per token, c = model_grad_oracle.dpos_roundings, the adds
of the kernels as written (DESIGN.md "Whole-model gradients").
"""
import numpy as np
import pytest
import torch

from tests import model_grad_oracle as M
from tests.test_gpu_encoder_block import guarded, guards_intact, same_bits
from tests.test_gpu_head_backward import TOL, within

pytestmark = pytest.mark.gpu
MODES = ["bf16x3", "bfloat16"]


@pytest.fixture(scope="module")
def vtd(cuda):
    import vision_transformer_detector_amd as m
    return m


@pytest.fixture(scope="module")
def stem(vtd):
    from vision_transformer_detector_amd import stem
    return stem


@pytest.fixture(scope="module")
def oracle():
    """One float64 run per case, shared by both modes and every test."""
    cache = {}

    def get(case):
        if case not in cache:
            images, sw, dx0 = M.seeded_stem(case)
            x64, g64 = M.stem_grads(sw, images, case[3], dx0)
            cache[case] = dict(images=images, sw=sw, dx0=dx0, x64=x64, g64=g64)
        return cache[case]
    return get


def up(n, m):
    return -(-n // m) * m


def layout(case, mode):
    """Byte offsets of the G operand and the row sums in the workspace (vtd_stem_bwd.hip,
    StemPlan: patches, W^T, G, row sums, each rounded up to 256 bytes) and G's row width."""
    B, Hh, Ww, p, d = case
    N = (-(-Hh // p)) * (-(-Ww // p))
    R, Pp, Dp = B * N, up(p * p * 3, 64), up(d, 64)
    eop, kk = (4, 3) if mode == "bf16x3" else (2, 1)
    gop = up(R * Pp * eop, 256) + up(Dp * kk * Pp * 2, 256)
    return gop, gop + up(R * Dp * eop, 256), Dp * eop // 2, R, Dp


@pytest.fixture(scope="module")
def runs(cuda, stem, oracle):
    """The device calls of one (case, mode), shared by the tests below."""
    cache = {}

    def get(case, mode):
        key = (case, mode)
        if key in cache:
            return cache[key]
        B, Hh, Ww, p, d = case
        o = oracle(case)
        images = torch.from_numpy(o["images"]).to(cuda)
        w = [torch.from_numpy(t).to(cuda) for t in o["sw"]]
        dx0 = torch.from_numpy(o["dx0"]).to(cuda)
        dims = stem.stem_dims(B, Hh, Ww, 3, p, d, mode)
        need = stem.workspace_bytes(dims)
        # run A: every output inside guard bands, the workspace poisoned with NaN bytes
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        outs = [guarded(dx0.shape, cuda)] + [guarded(t.shape, cuda) for t in w]
        x0, grads = stem.run(images, w, dims, dx0=dx0, ws=ws,
                             out=(outs[0][0], [t for t, _ in outs[1:]]))
        left = ws.clone()
        # run B: the same call again on the workspace as run A left it; run Z on zeros
        again = stem.run(images, w, dims, dx0=dx0, ws=ws)
        zeroed = stem.run(images, w, dims, dx0=dx0, ws=torch.zeros_like(ws))
        fwd_only = stem.run(images, w, dims, ws=torch.full_like(ws, 0xFF))[0]
        no_x0 = stem.run(images, w, dims, dx0=dx0, want_x0=False, ws=torch.full_like(ws, 0xFF))
        torch.cuda.synchronize()
        cache[key] = dict(o=o, images=images, w=w, dx0=dx0, dims=dims, x0=x0, grads=grads,
                          buffers=[b for _, b in outs], again=again, zeroed=zeroed,
                          fwd_only=fwd_only, no_x0=no_x0, left=left)
        return cache[key]
    return get


params = pytest.mark.parametrize("mode", MODES)
cases = pytest.mark.parametrize("case", M.STEM_CASES, ids=M.stem_case_id)


@params
@cases
def test_forward_value(runs, case, mode):
    """x0 of the forward-only call has the bits of the full call's, and is within the mode's
    forward tolerance of the float64 stem."""
    r = runs(case, mode)
    assert same_bits(r["fwd_only"], r["x0"])
    x0, x64 = r["x0"].cpu().numpy(), r["o"]["x64"]
    assert x0.shape == x64.shape
    print(f"{M.stem_case_id(case)} {mode}: forward max |x0 - x64| / max |x64| "
          f"{np.abs(x0 - x64).max() / np.abs(x64).max():.3g}")
    assert within(x0, x64, TOL[mode])


@params
@cases
def test_gradients_against_float64(runs, case, mode):
    r = runs(case, mode)
    o = r["o"]
    got = [g.cpu().numpy().astype(np.float64) for g in r["grads"]]
    for g, g64 in zip(got, o["g64"]):
        assert g.shape == g64.shape
    assert all(g.dtype == torch.float32 for g in r["grads"])
    errs = [float(np.abs(g - g64).max() / np.abs(g64).max()) for g, g64 in zip(got, o["g64"])]
    c = M.dpos_roundings(case[0], case[4])
    bound = c * 2.0 ** -24 * np.abs(o["dx0"].astype(np.float64)).sum(axis=(0, 2))
    dpos_err = np.abs(got[0] - o["g64"][0])[:, 0]
    print(f"{M.stem_case_id(case)} {mode}: dW {errs[1]:.3g}, db {errs[2]:.3g}, dpos {errs[0]:.3g} "
          f"(worst error / bound {(dpos_err / bound).max():.3g}, c = {c})")
    assert errs[1] <= M.BARS[mode], f"dW: {errs[1]:.3g} > {M.BARS[mode]}"
    assert errs[2] <= M.BARS[mode], f"db: {errs[2]:.3g} > {M.BARS[mode]}"
    assert np.all(dpos_err <= bound)


@params
@cases
def test_operand_rows_equal_act_forward(cuda, runs, case, mode):
    """The G operand stem_grad_rows_kernel left in the workspace has the bits
    vtd_act_forward(VTD_ACT_NONE) writes for the same dx0, pad columns included, and the row
    sums beside it are within their bound of the float64 sums."""
    from vision_transformer_detector_amd import _lib as L
    r = runs(case, mode)
    gop, rowsum, ld, R, Dp = layout(case, mode)
    d = case[4]
    want = torch.full((R * ld * 2,), 0xFF, dtype=torch.uint8, device=cuda)
    L.check(L.lib.vtd_act_forward(r["dx0"].data_ptr(), R, d, d, L.ACT_NONE, want.data_ptr(), ld,
                                  L.BF16X3 if mode == "bf16x3" else L.BF16, L.stream_ptr()),
            "vtd_act_forward")
    torch.cuda.synchronize()
    assert torch.equal(r["left"][gop:gop + R * ld * 2], want)
    sums = r["left"][rowsum:rowsum + 4 * R].view(torch.float32).cpu().numpy().astype(np.float64)
    dx = r["o"]["dx0"].astype(np.float64).reshape(R, d)
    c = M.dpos_roundings(0, d)
    assert np.all(np.abs(sums - dx.sum(1)) <= c * 2.0 ** -24 * np.abs(dx).sum(1))


@params
@cases
def test_runs_are_bit_identical_and_read_nothing_unwritten(runs, case, mode):
    """The run on a NaN-poisoned workspace, a second run on the workspace it left and a run on a
    zeroed workspace give the same bits in every output, and so does the call without x0."""
    r = runs(case, mode)
    for name in ("again", "zeroed", "no_x0"):
        x0, grads = r[name]
        assert (x0 is None) if name == "no_x0" else same_bits(x0, r["x0"]), name
        for i, (a, b) in enumerate(zip(grads, r["grads"])):
            assert same_bits(a, b), (name, i)
    for t in [r["x0"]] + list(r["grads"]):
        assert bool(torch.isfinite(t).all())


@params
@cases
def test_guard_bands_intact(runs, case, mode):
    r = runs(case, mode)
    for label, buf in zip(("x0", "dpos", "dW", "db"), r["buffers"]):
        assert guards_intact(buf), label


@params
def test_dx0_off_a_16_byte_boundary_takes_the_generic_path(stem, runs, mode):
    """d % 4 == 0 but a base 4 bytes past a 16-B boundary: the same bits as the aligned call."""
    case = M.STEM_CASES[0]
    r = runs(case, mode)
    flat = torch.empty(r["dx0"].numel() + 1, dtype=torch.float32, device=r["dx0"].device)
    shifted = flat[1:].view(r["dx0"].shape)
    shifted.copy_(r["dx0"])
    assert shifted.data_ptr() % 16 == 4
    _, grads = stem.run(r["images"], r["w"], r["dims"], dx0=shifted, want_x0=False)
    for a, b in zip(grads, r["grads"]):
        assert same_bits(a, b)


@params
@cases
def test_autograd_op_equals_the_c_call(vtd, runs, case, mode):
    r = runs(case, mode)
    w = [t.clone().requires_grad_(True) for t in r["w"]]
    images = r["images"].clone().requires_grad_(True)
    x0 = vtd.patch_embedding(images, w, patch_size=case[3], dtype=mode)
    assert same_bits(x0.detach(), r["x0"])
    x0.backward(r["dx0"])
    assert images.grad is None
    for t, g in zip(w, r["grads"]):
        assert same_bits(t.grad, g)
    # weights that do not require grad get None
    w2 = [t.clone().requires_grad_(i != 1) for i, t in enumerate(r["w"])]
    vtd.patch_embedding(r["images"], w2, patch_size=case[3], dtype=mode).backward(r["dx0"])
    assert w2[1].grad is None and same_bits(w2[0].grad, r["grads"][0])
    assert same_bits(w2[2].grad, r["grads"][2])


def test_patch_embedding_validation(vtd, cuda):
    case = M.STEM_CASES[0]
    images, sw, _ = M.seeded_stem(case)
    x = torch.from_numpy(images).to(cuda)
    w = [torch.from_numpy(t).to(cuda) for t in sw]
    with pytest.raises(ValueError, match="images must be float32"):
        vtd.patch_embedding(x.double(), w, patch_size=8)
    with pytest.raises(ValueError, match=r"\(B, H, W, C\)"):
        vtd.patch_embedding(x[0], w, patch_size=8)
    with pytest.raises(ValueError, match=r"weights\[0\] \(position embedding\) has shape"):
        vtd.patch_embedding(x, [w[0][:, 0]] + w[1:], patch_size=8)
    with pytest.raises(ValueError, match=r"weights\[1\] \(linear_projection kernel\) has shape"):
        vtd.patch_embedding(x, [w[0], w[1][:-1], w[2]], patch_size=8)
    with pytest.raises(ValueError, match=r"weights\[2\] \(linear_projection bias\) must be float32"):
        vtd.patch_embedding(x, w[:2] + [w[2].double()], patch_size=8)
    with pytest.raises(ValueError, match=r"weights\[0\] \(position embedding\) must be a device"):
        vtd.patch_embedding(x, [w[0].cpu()] + w[1:], patch_size=8)
    with pytest.raises(ValueError, match="linear_projection kernel.*must be a"):
        vtd.patch_embedding(x, [w[0], w[2], w[2]], patch_size=8)
