"""The LayerNorm-backward yardstick (tests/ln_grad_oracle.py) checked on the CPU: the float64
formulas against float64 torch.autograd, known answers on the designed rows, the fp32
restatement of the kernels under HALF of every derived bar on every case the device runs
(tests/test_gpu_layernorm_backward.py holds the device to the whole bar), a seeded defect that
the measure must catch, the restated launch geometry against the library's own workspace size,
and every argument error of vtd_layernorm_backward, which must answer before any device call
(the pointers here are never dereferenced).  The counts k_dx and k_param behind the bars are
derived in the oracle's docstring."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ln_grad_oracle as O

CASES = O.shape_cases() + O.design_cases() + O.reduce_cases()


def test_float64_formulas_match_torch_autograd():
    c = O.Case(252, 13)
    x = torch.tensor(c.x, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(c.gamma, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(c.beta, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (c.D,), g, b, eps=O.EPS)
    np.testing.assert_allclose(y.detach().numpy(), O.forward64(c.x, c.gamma, c.beta), rtol=1e-12,
                               atol=1e-12)
    y.backward(torch.tensor(c.dy, dtype=torch.float64))
    x64 = c.x.astype(np.float64)
    mean = x64.mean(axis=1)
    rstd = 1.0 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(axis=1) + O.EPS)
    ref = O.backward64(c.x, np.stack([mean, rstd], axis=1), c.gamma, c.dy)
    scale = np.abs(ref["dx"]).max()
    np.testing.assert_allclose(x.grad.numpy(), ref["dx"], rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(g.grad.numpy(), ref["dgamma"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(b.grad.numpy(), ref["dbeta"], rtol=1e-12, atol=1e-12)
    # add is the residual path's gradient: it adds to dx and to its measure alone
    with_add = O.backward64(c.x, np.stack([mean, rstd], axis=1), c.gamma, c.dy, c.add)
    np.testing.assert_array_equal(with_add["dx"], ref["dx"] + c.add)
    np.testing.assert_array_equal(with_add["den_x"], ref["den_x"] + np.abs(c.add))
    np.testing.assert_array_equal(with_add["dgamma"], ref["dgamma"])


def test_known_answers_on_designed_rows():
    c = O.Case(64, 5, "const", seed=1)
    stat = O.stats32(c.x)
    ref = O.backward64(c.x, stat, c.gamma, c.dy)
    # the constant row: mean exact, xhat = 0, rstd = 1 / sqrt(eps); dx = rstd (gy - mean(gy))
    assert stat[0, 0] == np.float32(2.5) and abs(stat[0, 1] - 1 / np.sqrt(O.EPS)) < 1e-5
    gy = c.dy[0].astype(np.float64) * 1.5
    np.testing.assert_allclose(ref["dx"][0], float(stat[0, 1]) * (gy - gy.mean()), rtol=1e-12)
    # constant dy and constant gamma: gy - mean(gy) = 0 and sum(xhat) ~ 0, dx cancels
    assert np.abs(ref["dx"][2]).max() < 1e-3 * ref["den_x"][2].min()
    # dy in one column j: dx_j = rstd gy_j (1 - 1 / D - xhat_j^2 / D)
    j = int(np.flatnonzero(c.dy[3])[0])
    xh = (c.x[3].astype(np.float64) - float(stat[3, 0])) * float(stat[3, 1])
    want = float(stat[3, 1]) * (-1.25 * 1.5) * (1 - 1 / 64 - xh[j] ** 2 / 64)
    np.testing.assert_allclose(ref["dx"][3, j], want, rtol=1e-12)
    np.testing.assert_array_equal(ref["dbeta"], c.dy.astype(np.float64).sum(axis=0))
    # gamma = 0: dx is add alone, and without add it is exactly zero in the emulation too
    z = O.Case(64, 5, "zero", seed=1)
    zs = O.stats32(z.x)
    assert not O.backward64(z.x, zs, z.gamma, z.dy)["dx"].any()
    assert not O.emulate(z.x, zs, z.gamma, z.dy)[0].any()
    np.testing.assert_array_equal(O.emulate(z.x, zs, z.gamma, z.dy, z.add)[0], z.add)


def test_geometry():
    assert O.row_counts()[2] == O.multi_range_rows() == 9
    for rows in (1, 7, 8, 9, 4096, 8192, 8193, 50176, 51200, 10 ** 7):
        rpr, R = O.range_rows(rows), O.ranges(rows)
        assert rpr % 4 == 0 and rpr >= 8 and 1 <= R <= O.MAX_RANGES
        assert (R - 1) * rpr < rows <= R * rpr
    assert O.k_dx(768, "vec") == 28 and O.k_dx(4096, "vec") == 80 and O.k_dx(7, "generic") == 17
    assert O.k_dx(4100, "generic") == 65 + 16
    assert O.k_param(5) == 2 + 1 + 19 and O.k_param(50176) == 13 + 61 + 19
    assert (O.ranges(323), O.range_rows(8200), O.ranges(8200)) == (41, 12, 684)
    assert O.route(768, (768, 772)) == "vec" and O.route(768, (770,)) == "generic"
    assert O.route(768, (768,), misaligned=True) == "generic"
    assert O.route(4100) == "generic" and O.route(7) == "generic"


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_emulation_stays_under_half_of_every_bar(c):
    stat = O.stats32(c.x)
    worst = 0.0
    natural = O.route(c.D)
    for path in {natural, "generic"}:                      # "generic" again: a misaligned base
        for add in (None, c.add):
            ref = O.backward64(c.x, stat, c.gamma, c.dy, add)
            got = O.emulate(c.x, stat, c.gamma, c.dy, add, path)
            r = O.ratios(got, ref, c.D, c.rows, path)
            worst = max(worst, *r)
            assert max(r) <= 0.5, (path, add is not None, r)
    print(f"{c!r}: worst fraction of a bar {worst:.3f}")


@pytest.mark.parametrize("shape", O.OP_SHAPES)
def test_op_level_emulation_with_fp32_statistics(shape):
    """What tests/test_gpu_layernorm_backward.py::test_op asks of the device: fp32 statistics in,
    float64 with float64 statistics as the reference, the same bars."""
    c = O.op_case(shape)
    ref = O.backward64(c.x, O.stats64(c.x), c.gamma, c.dy)
    got = O.emulate(c.x, O.stats_fp32(c.x), c.gamma, c.dy)
    r = O.ratios(got, ref, c.D, c.rows, "vec")
    print(f"{shape}: fractions of the bars {r}")
    assert max(r) <= 0.5


def test_vector_and_generic_paths_sum_the_parameters_in_one_order():
    c = O.Case(252, 9)
    stat = O.stats32(c.x)
    a = O.emulate(c.x, stat, c.gamma, c.dy, None, "vec")
    b = O.emulate(c.x, stat, c.gamma, c.dy, None, "generic")
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


def test_the_measure_catches_seeded_defects():
    c = O.Case(768, 9)
    stat = O.stats32(c.x)
    ref = O.backward64(c.x, stat, c.gamma, c.dy, c.add)
    dx, dg, db = O.emulate(c.x, stat, c.gamma, c.dy, c.add)
    assert max(O.ratios((dx, dg, db), ref, c.D, c.rows, "vec")) <= 0.5
    # the xhat term dropped; mean over D - 1; add forgotten; one row left out of dbeta / dgamma
    xh = (c.x - stat[:, :1]) * stat[:, 1:]
    gy = c.dy * c.gamma
    no_xhat = stat[:, 1:] * (gy - gy.mean(axis=1, keepdims=True)) + c.add
    assert O.ratio(no_xhat, ref["dx"], ref["den_x"], O.k_dx(c.D, "vec") * O.U) > 1
    biased = ref["dx"] + stat[:, 1:] * gy.mean(axis=1, keepdims=True) / c.D
    assert O.ratio(biased, ref["dx"], ref["den_x"], O.k_dx(c.D, "vec") * O.U) > 1
    assert O.ratio(dx - c.add, ref["dx"], ref["den_x"], O.k_dx(c.D, "vec") * O.U) > 1
    cg = O.k_param(c.rows) * O.U
    assert O.ratio(db - c.dy[8], ref["dbeta"], ref["den_b"], cg) > 1
    assert O.ratio(dg - c.dy[8] * xh[8], ref["dgamma"], ref["den_g"], cg) > 1


# ------------------------------------------------------------------ the library's host side
@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def test_abi_is_declared_and_the_version_stays(L):
    for name in ("vtd_layernorm_backward_workspace_bytes", "vtd_layernorm_backward"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert L.lib.vtd_abi_version() == 17
    import vision_transformer_detector_amd as vtd
    assert "layer_norm" in vtd.__all__ and callable(vtd.layer_norm)


def test_workspace_follows_the_restated_geometry(L):
    n = ctypes.c_size_t()
    for rows in (1, 5, 8, 9, 17, 4096, 8192, 8193, 50176, 51200, 2 ** 33):
        for D in (4, 7, 768, 4100):
            assert L.lib.vtd_layernorm_backward_workspace_bytes(rows, D, ctypes.byref(n)) == 0
            assert n.value == O.ranges(rows) * 2 * D * 4, (rows, D)
    for args in ((0, 4, ctypes.byref(n)), (4, 0, ctypes.byref(n)), (-1, 4, ctypes.byref(n)),
                 (4, 4, None)):
        assert L.lib.vtd_layernorm_backward_workspace_bytes(*args) == -1


def test_argument_errors_need_no_device(L):
    n = ctypes.c_size_t()
    L.lib.vtd_layernorm_backward_workspace_bytes(9, 64, ctypes.byref(n))
    ok = dict(x=1024, ldx=64, stat=2048, gamma=4096, dy=8192, lddy=64, add=None, ldadd=0, rows=9,
              D=64, dx=16384, lddx=64, dgamma=32768, dbeta=65536, ws=131072, ws_bytes=n.value)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.vtd_layernorm_backward(a["x"], a["ldx"], a["stat"], a["gamma"], a["dy"],
                                            a["lddy"], a["add"], a["ldadd"], a["rows"], a["D"],
                                            a["dx"], a["lddx"], a["dgamma"], a["dbeta"], a["ws"],
                                            a["ws_bytes"], None)

    bad = [("null x", dict(x=None), -1, b"null"), ("null stat", dict(stat=None), -1, b"null"),
           ("null gamma", dict(gamma=None), -1, b"null"), ("null dy", dict(dy=None), -1, b"null"),
           ("null dx", dict(dx=None), -1, b"null"), ("rows = 0", dict(rows=0), -1, b"size"),
           ("rows < 0", dict(rows=-3), -1, b"size"), ("D = 0", dict(D=0), -1, b"size"),
           ("ldx < D", dict(ldx=63), -1, b"leading"), ("lddy < D", dict(lddy=60), -1, b"leading"),
           ("lddx < D", dict(lddx=0), -1, b"leading"),
           ("ldadd < D", dict(add=512, ldadd=32), -1, b"leading"),
           ("dgamma alone", dict(dbeta=None), -1, b"together"),
           ("dbeta alone", dict(dgamma=None), -1, b"together"),
           ("stat alignment", dict(stat=2052), -1, b"8-byte"),
           ("x alignment", dict(x=1026), -1, b"4-byte"),
           ("null workspace", dict(ws=None), -1, b"workspace"),
           ("workspace alignment", dict(ws=131080), -1, b"16-byte"),
           ("small workspace", dict(ws_bytes=n.value - 1), -4, b"workspace smaller")]
    for what, kw, code, word in bad:
        assert call(**kw) == code, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
    with pytest.raises(ValueError):
        L.check(call(rows=0), "vtd_layernorm_backward")
    with pytest.raises(L.VtdError):
        L.check(call(ws_bytes=0), "vtd_layernorm_backward")


def test_layer_norm_argument_checks():
    import vision_transformer_detector_amd as vtd
    x, g = torch.zeros(2, 3, 8), torch.ones(8)
    with pytest.raises(ValueError, match="device tensor"):
        vtd.layer_norm(x, g, g)
    with pytest.raises(ValueError, match="device tensor"):
        vtd.layer_norm(np.zeros((2, 8), np.float32), g, g)
