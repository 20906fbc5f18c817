"""The workspace plans of the training chains are pinned on the CPU: the three
*_backward_workspace_bytes queries against tests/golden/train_workspace_bytes.json.  The plans
hold the split-K / msplit choices next to the offsets, so a changed choice, buffer or padding
rule shows as a changed byte count.  No GPU: without a device the CU count falls back to 256.
"""
import ctypes
import json
import os

import pytest

from tests import block_grad_oracle as K
from tests import model_grad_oracle as M
from tests.test_host_cpu import CONFIGS, _cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_workspace_bytes.json")
# (B, N, d, heads, key_dim, q): the block oracle's cases and C2's block at batch 64 and 1
BLOCK_CASES = [c[:6] for c in K.CASES] + [(64, 196, 768, 12, 64, 2), (1, 196, 768, 12, 64, 2)]


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def train_workspace_table(L):
    """{"head/C<n>/<dtype>/<batch>" | "block/<B>x<N>x<d>_h<heads>x<dk>_q<q>/<dtype>" |
    "stem/<B>_<H>x<W>_p<p>_d<d>/<dtype>": bytes, or {"error": code} where the library rejects
    the configuration} of the loaded library."""
    table = {}

    def ask(key, fn, dims):
        n = ctypes.c_size_t()
        rc = fn(ctypes.byref(dims), ctypes.byref(n))
        table[key] = n.value if rc == 0 else {"error": rc}

    for ci, kw in enumerate(CONFIGS):
        for dname in ("BF16", "BF16X3", "F32"):
            for b in (1, 8, 64):
                ask(f"head/C{ci + 1}/{dname}/{b}", L.lib.vtd_head_backward_workspace_bytes,
                    _cfg(L, kw, batch=b, dtype=getattr(L, dname)))
    for B, N, d, heads, dk, q in BLOCK_CASES:
        for dname in ("BF16", "BF16X3"):
            ask(f"block/{B}x{N}x{d}_h{heads}x{dk}_q{q}/{dname}",
                L.lib.vtd_encoder_block_backward_workspace_bytes,
                L.VtdBlockDims(batch=B, tokens=N, d=d, num_heads=heads, key_dim=dk,
                               mlp_quantities=q, use_mish=1, dtype=getattr(L, dname)))
    for B, H, W, p, d in M.STEM_CASES:
        for dname in ("BF16", "BF16X3"):
            ask(f"stem/{B}_{H}x{W}_p{p}_d{d}/{dname}", L.lib.vtd_stem_backward_workspace_bytes,
                L.VtdStemDims(batch=B, H=H, W=W, C=3, patch=p, d=d, dtype=getattr(L, dname)))
    return table


def test_train_workspace_bytes_match_recorded_table(L):
    """vtd_head_backward_workspace_bytes for the four CONFIGS x {BF16, BF16X3, F32} x batch
    {1, 8, 64} (F32 has no backward: its error code is what is recorded),
    vtd_encoder_block_backward_workspace_bytes for BLOCK_CASES x {BF16, BF16X3} and
    vtd_stem_backward_workspace_bytes for model_grad_oracle.STEM_CASES x {BF16, BF16X3} equal
    the recorded table entry by entry.

    The table was recorded from a build of the commit BEFORE the training chains moved into
    csrc/vtd_train_runtime.hip (so it checks that restructuring, and every later change,
    against the earlier plans, never against the code under test):
        tools/build_prev.sh <that commit>
        VTD_LIB_PATH=vision_transformer_detector_amd/libvtd_prev.so python -c "import json; \
            from tests import test_train_plan_host as t; \
            from vision_transformer_detector_amd import _lib; \
            json.dump(t.train_workspace_table(_lib), open(t.GOLDEN, 'w'), indent=0)"
    with none of the VTD_* environment switches set.  A change that alters a training
    workspace on purpose re-records the table from its own build and says so."""
    want = json.load(open(GOLDEN))
    got = train_workspace_table(L)
    n_stem = len(M.STEM_CASES)
    assert sorted(got) == sorted(want)
    assert len(want) == 4 * 3 * 3 + len(BLOCK_CASES) * 2 + n_stem * 2
    for k, v in want.items():        # a byte count everywhere but F32
        assert isinstance(v, dict) == ("/F32/" in k), k
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
