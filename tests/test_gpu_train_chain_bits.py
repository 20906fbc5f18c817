"""The training chains give recorded bits: sha256 digests over the raw bytes of every output of
encoder.run (vtd_encoder_block_backward), head.run (vtd_head_backward) and stem.run
(vtd_stem_backward) against tests/golden/train_chain_digests.json.

Each chain runs forward-only and forward + backward from the oracles' seeded inputs, in both
modes, without dropout and with rate 0.25, seed 7, step 3 (the stem has no dropout).  The head's
`encoded` is a seeded N(0, 1) tensor, so the file does not depend on the inference forward.
Every launch of a chain is deterministic (no atomics, fixed summation orders), so a changed
digest means a launch was added, dropped, reordered or given other arguments.

The digests were recorded on an MI355X from a build of the commit BEFORE the training chains
moved into csrc/vtd_train_runtime.hip, never from the code under test:
    tools/build_prev.sh <that commit>
    VTD_LIB_PATH=vision_transformer_detector_amd/libvtd_prev.so python -c "import json; \
        from tests import test_gpu_train_chain_bits as t; \
        json.dump(t.all_digests(), open(t.GOLDEN, 'w'), indent=0, sort_keys=True)"
with none of the VTD_* environment switches set.  A later change that alters these bits on
purpose (a kernel's summation order, a split choice) re-records the file from its own build
and says so.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import vtd_numpy as V
from tests import block_grad_oracle as K
from tests import head_grad_oracle as H
from tests import model_grad_oracle as M
from tests.test_host_cpu import _cfg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "train_chain_digests.json")
MODES = ["bf16x3", "bfloat16"]
RATE, SEED, STEP = 0.25, 7, 3
BLOCK_SITE_BASE, HEAD_SITE_BASE = 0, 6

# None of model_grad_oracle.CASES splits K in the head, so one more: its first head GEMM is
# (M 51, N 576, K 1024), split 2 ways in bfloat16 and 6 ways in bf16x3 (SPLITK_HEAD)
SPLITK_KW = dict(input_shape=(128, 128, 3), patch_size=4, embedding_dim=16,
                 mlp_head_last_units=136, mlp_head_dense_layers_quantity=3,
                 mlp_head_dense_mish_block_repeats=1)
SPLITK_HEAD = {"bfloat16": 2, "bf16x3": 6}
HEAD_CASES = M.CASES + [("splitk", 3)]
STEM_CASES = [(16, 64, 64, 4, 64), (2, 33, 50, 7, 20)]
assert all(c in M.STEM_CASES for c in STEM_CASES)


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrays]


def block_digests(case, mode):
    """{"<pass>/<drop>/<output>": sha256}: pass fwd (y) or bwd (y, dx, the weight gradients)."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import encoder as enc
    B, N, d, heads, dk, q, use_mish = case
    dims = enc.block_dims(B, N, d, heads, dk, q, use_mish, mode)
    w = _dev(K.seeded_weights(case))
    x, dy = _dev(K.seeded_inputs(case))
    out = {}
    for dname, drop in (("nodrop", None),
                        ("drop", L.VtdBlockDropout(seed=SEED, step=STEP,
                                                   site_base=BLOCK_SITE_BASE, rate=RATE))):
        y, _, _ = enc.run(x, w, dims, drop=drop)
        out[f"fwd/{dname}/y"] = digest(y)
        y, grads, dx = enc.run(x, w, dims, dy=dy, drop=drop)
        out[f"bwd/{dname}/y"] = digest(y)
        out[f"bwd/{dname}/dx"] = digest(dx)
        for n, g in zip(K.names(q), grads):
            out[f"bwd/{dname}/{n}"] = digest(g)
    return out


def head_inputs(name, batch):
    """(kwargs, the head's weights by Keras name, encoded (B, N, d), dlogits (B, 17, 6))."""
    if name == "splitk":
        kw = dict(SPLITK_KW)
        w = V.init_weights(seed=11, **kw)
        rng = np.random.default_rng(batch)
        dlogits = (rng.normal(0.0, 1.0, (batch, 17, 6)) / (batch * 17)).astype(np.float32)
    else:
        kw, w, _, dlogits = M.load_case(name, batch)
    k = V.resolve_kwargs(**kw)
    gh, gw = V.token_grid(k["input_shape"][0], k["input_shape"][1], k["patch_size"])
    rng = np.random.default_rng([gh * gw, k["embedding_dim"], batch])
    encoded = rng.standard_normal((batch, gh * gw, k["embedding_dim"])).astype(np.float32)
    return kw, H.head_weights(w, dtype=torch.float32), encoded, dlogits


def head_digests(case, mode):
    """{"<pass>/<drop>/<output>": sha256}: pass fwd (logits) or bwd (the weight gradients,
    d_encoded)."""
    from vision_transformer_detector_amd import _lib as L
    from vision_transformer_detector_amd import head
    from vision_transformer_detector_amd.detector import _resolve_dtype
    name, b = case
    kw, hw, encoded, dlogits = head_inputs(name, b)
    cfg = _cfg(L, kw, batch=b, dtype=_resolve_dtype(mode))
    w = [t.cuda() for t in hw.values()]
    enc, dl = _dev([encoded, dlogits])
    out = {}
    for dname, drop in (("nodrop", None),
                        ("drop", L.VtdBlockDropout(seed=SEED, step=STEP,
                                                   site_base=HEAD_SITE_BASE, rate=RATE))):
        logits = torch.empty((b, 17, 6), dtype=torch.float32, device=enc.device)
        head.run(cfg, enc, w, logits=logits, drop=drop)
        out[f"fwd/{dname}/logits"] = digest(logits)
        grads = [torch.empty_like(t) for t in w]
        dx = torch.empty_like(enc)
        head.run(cfg, enc, w, dlogits=dl, grads=grads, d_encoded=dx, drop=drop)
        for n, g in zip(hw, grads):
            out[f"bwd/{dname}/{n}"] = digest(g)
        out[f"bwd/{dname}/d_encoded"] = digest(dx)
    return out


def stem_digests(case, mode):
    """{"<pass>/<output>": sha256}: pass fwd (x0) or bwd (x0, dpos, dW, db)."""
    from vision_transformer_detector_amd import stem
    B, Hh, Ww, p, d = case
    images, sw, dx0 = M.seeded_stem(case)
    dims = stem.stem_dims(B, Hh, Ww, 3, p, d, mode)
    (img, dx), w = _dev([images, dx0]), _dev(sw)
    x0, _ = stem.run(img, w, dims)
    out = {"fwd/x0": digest(x0)}
    x0, grads = stem.run(img, w, dims, dx0=dx)
    out["bwd/x0"] = digest(x0)
    for n, g in zip(("pos", "w", "b"), grads):
        out[f"bwd/{n}"] = digest(g)
    return out


RUNS = ([("block", c, K.case_id(c), block_digests) for c in K.CASES] +
        [("head", c, c[0], head_digests) for c in HEAD_CASES] +
        [("stem", c, M.stem_case_id(c), stem_digests) for c in STEM_CASES])


def all_digests():
    """{"<chain>/<case>/<mode>": {output: sha256}} of the loaded library (the recording)."""
    return {f"{chain}/{cid}/{mode}": fn(case, mode)
            for chain, case, cid, fn in RUNS for mode in MODES}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_golden_holds_every_run(golden):
    assert sorted(golden) == sorted(f"{r[0]}/{r[2]}/{m}" for r in RUNS for m in MODES)


@pytest.mark.parametrize("mode", MODES)
def test_splitk_case_splits_its_first_head_gemm(cuda, mode):
    """The case cannot silently stop covering the head's split-K branch."""
    from vision_transformer_detector_amd import _lib as L
    x3 = mode == "bf16x3"
    assert L.lib.vtd_gemm_splitk_choice(51, 576, 3 * 1024 if x3 else 1024,
                                        L.BF16X3 if x3 else L.BF16) == SPLITK_HEAD[mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("run", RUNS, ids=lambda r: f"{r[0]}-{r[2]}")
def test_outputs_have_the_recorded_bits(cuda, golden, run, mode):
    chain, case, cid, fn = run
    want = golden[f"{chain}/{cid}/{mode}"]
    got = fn(case, mode)
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong
    if chain != "stem":          # the masks act: dropout changes the forward's bits
        fwd = [k for k in want if k.startswith("fwd/nodrop/")]
        assert all(want[k] != want[k.replace("nodrop", "drop")] for k in fwd)
