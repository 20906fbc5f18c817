"""The designed-operand generator of tests/gemm_designs.py, checked without a GPU: the pieces
split as designed, the 2^24 rule holds, an fp32 GEMM emulation reproduces the expected output
bit for bit in every accumulation order, and each seeded kernel fault breaks that equality --
while the single dropped lo element passes the random-operand tolerance of
test_gpu_bf16x3.test_split_gemm_vs_fp64 (the gap the designed tests close)."""
import math

import numpy as np
import pytest
import torch

from tests import gemm_designs as G

MODES = ("bf16", "f32", "bf16x3")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K", [(9, 7, 64), (5, 17, 192), (3, 4, 1280)])
def test_design_invariants(mode, M, N, K):
    d = G.make_design(mode, M, N, K)
    assert d.check_rule() < 2 ** 24
    # row / column exponents reach both ends and are not monotone (M >= 4)
    assert d.c.max() == 12 and d.c.min() == -12 and (np.diff(d.c) > 0).any() and (np.diff(d.c) < 0).any()
    assert (np.diff(d.t) != 0).all()
    exp = d.expected()
    f32 = G.cast_f32(exp)                                     # representable (asserts inside)
    assert np.isfinite(f32).all() and (np.abs(f32[f32 != 0]) > 1e-30).all()
    hi, lo = G.cast_split(exp)
    assert np.array_equal(hi, G.cast_bf16(exp))
    assert (np.abs(G.bf16_value(hi).astype(np.float64) + G.bf16_value(lo) - exp)
            <= 2.0 ** -16 * np.abs(exp)).all()
    if mode == "bf16x3":
        P = K
        assert d.a_op.shape == (M, 2 * P) and d.b_op.shape == (N, 3 * P) and d.Kcall == 3 * P
        assert np.array_equal(d.b_op[:, :P], d.b_op[:, P:2 * P])        # both hi copies equal
        # the expectation is the three products only: it differs from the f32 product by lo.lo
        full = (d.ha + d.la / 256) @ (d.hb + d.lb / 256).T
        lolo = (d.la / 256) @ (d.lb / 256).T
        assert np.array_equal(exp / (d.unit * 256), full - lolo)
        if K <= 192:
            assert (lolo != 0).any()
        # no h is a power of two
        assert not np.isin(np.abs(d.ha), (1, 2, 4, 8)).any()


@pytest.mark.parametrize("mode", MODES)
def test_emulation_is_exact_in_every_order(mode):
    d = G.make_design(mode, 9, 7, 192)
    want = G.cast_f32(d.expected())
    for order in G.ORDERS:
        assert np.array_equal(G.emulate(d.a_read, d.b_read, order), want), order


def test_long_k_ranges_and_refusal():
    assert G.base_range("bf16x3", 1280) == ((5, 6, 7), 3)
    assert G.base_range("bf16x3", 1344) == ((3,), 1)
    assert G.base_range("bf16x3", 3072) == ((3,), 1)
    with pytest.raises(ValueError):
        G.make_design("bf16x3", 2, 2, 3136)
    d = G.make_design("bf16x3", 2, 3, 3072)
    assert np.array_equal(G.emulate(d.a_read, d.b_read, "reverse"), G.cast_f32(d.expected()))


@pytest.mark.parametrize("epi", [("bias",), ("bias", "rowadd"), ("bias", "resid"),
                                 ("bias", "lnfold"), ("bias", "rowadd", "resid", "lnfold")])
@pytest.mark.parametrize("mode", MODES)
def test_epilogue_data_keeps_the_rule(mode, epi):
    d = G.make_design(mode, 11, 9, 128, epi=epi)
    assert d.check_rule() < 2 ** 24
    G.cast_f32(d.expected())
    # the same epilogue in fp32, in the kernels' order of operations
    v = G.emulate(d.a_read, d.b_read, "four_lanes")
    e = d.epi
    if "lnfold" in e:
        st = d.lnstat()
        v = (v - st[:, :1] * e["colsum"].astype(np.float32)[None, :]) * st[:, 1:]
    for a in d.addends():
        v = v + a.astype(np.float32)
    assert v.dtype == np.float32 and np.array_equal(v, G.cast_f32(d.expected()))
    if "rowadd" in e:
        assert e["rowadd_ncols"] < d.N
    assert np.array_equal(G.bf16_value(G.bf16_bits(e["resid"].astype(np.float32))), e["resid"]) \
        if "resid" in e else True


def test_scatter_expected_is_the_keras_reshape():
    T, B = 5, 2
    v = np.arange(B * T * 17, dtype=np.float64).reshape(B * T, 17)
    s = G.scatter_expected(v, T)
    for m in range(B * T):
        for n in range(17):
            b, t = divmod(m, T)
            f = t * 17 + n
            assert s[b * 17 + f // T, f % T] == v[m, n]


@pytest.mark.parametrize("fault", G.FAULTS, ids=lambda f: f.__name__)
def test_seeded_fault_breaks_the_exact_comparison(fault):
    d = G.make_design("bf16x3", 16, 16, 192)
    want = G.cast_f32(d.expected())
    assert np.array_equal(G.emulate(d.a_read, d.b_read), want)
    got = fault(d)
    assert not np.array_equal(got, want), fault.__name__


def test_dropped_lo_element_passes_the_random_operand_tolerance():
    """The operands of test_gpu_bf16x3.test_split_gemm_vs_fp64 at 200 x 300 x 1024 (N(0, 1)
    and N(0, 1 / K), the check err <= 2e-5 max |ref|): the three products with one lo element of
    A dropped still pass it.  The exact comparison above does not let the same fault through."""
    M, N, K = 200, 300, 1024
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).numpy()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).numpy()
    ref64 = A.astype(np.float64) @ W.astype(np.float64).T
    ahi, alo = (G.bf16_value(p).astype(np.float64) for p in G.split_bits(A))
    bhi, blo = (G.bf16_value(p).astype(np.float64) for p in G.split_bits(W))
    # a typical element: the one with the median |lo| (the very largest lo, under the largest
    # weight, would move an output by 1e-3 and be caught)
    flat = np.argsort(np.abs(alo), axis=None)[alo.size // 2]
    m, k = np.unravel_index(flat, alo.shape)
    alo[m, k] = 0.0
    got = ahi @ bhi.T + alo @ bhi.T + ahi @ blo.T
    err = np.abs(got - ref64).max()
    assert err <= 2e-5 * np.abs(ref64).max()
    # ... and it is a real fault: that row moved by more than the fp32 sum's own rounding
    clean = got[m] + (G.bf16_value(G.split_bits(A)[1])[m, k].astype(np.float64)) * bhi[:, k]
    assert np.abs(clean - got[m]).max() > 2.0 ** -24 * np.abs(ref64[m]).max()


def test_branch_table_names_every_kernel_and_knob_value():
    from tests.test_gpu_gemm_designed import BRANCHES
    kernels = {b["kernel"] for b in BRANCHES}
    assert kernels == {"skinny", "tn128", "pp2", "pp2-epilogues", "tile-order", "splitk",
                       "f32-pp2", "wgrad", "w4", "mx8", "mx8-x4"}
    by = {b["kernel"]: b for b in BRANCHES}
    assert set(by["pp2"]["knobs"]["GEMM_TR"]) == {0, 1}
    assert set(by["pp2"]["knobs"]["SKINNY"]) == {-1, 0}
    assert set(by["tile-order"]["knobs"]["GEMM_NGW"]) == {-1, 0, 1, 2, 3}
    assert set(by["f32-pp2"]["knobs"]["F32_PP2"]) == {0, 1}
    assert set(by["tn128"]["knobs"]["SKINNY"]) == {-1, 0}
    assert set(by["mx8"]["knobs"]["GEMM_TR"]) == {0, 1}
    assert set(by["w4"]["knobs"]["GEMM_TPW"]) >= {2}
    assert {b["dtype"] for b in BRANCHES if b["kernel"] in ("skinny", "tn128", "pp2", "splitk")} \
        >= {("bf16", "bf16x3")}
    for b in BRANCHES:
        assert b["shapes"] and b["reached"], b["kernel"]
