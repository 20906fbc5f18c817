"""vtd_layernorm_backward and the layer_norm op on the device against float64, held to the bars
derived in tests/ln_grad_oracle.py (c = k_dx 2^-24 componentwise on dx, c_g = k_param 2^-24 on
dgamma / dbeta; tests/test_ln_grad_kat.py keeps the fp32 restatement of the kernels under half of
each on the same cases).

Every case runs with add null, separate and aliased to dx, with ldx, lddy, lddx, ldadd above D
(multiples of 4 on the vector path), every input's pad columns and guards NaN, every output
0xA5 outside the rows x D (resp. D) elements the contract writes -- those bytes must come back
-- and twice: the runs must be bit-identical.  The row statistics come from vtd_layernorm_stats,
as in the op.  Row counts 1, 5 and the smallest count with two ranges and a ragged last one, read
from vtd_layernorm_backward_workspace_bytes; widths 4 .. 4096 on the vector kernels, 7 and 4100
on the generic path, which a misaligned x must take as well.

Measured on an MI355X, as fractions of the bars (the tests print them): dx at most 0.199 (D 64,
8200 rows), dgamma 0.119, dbeta 0.090, each within a few per cent of the CPU restatement's figure
for the same case; the misaligned case 0.076 / 0.099 / 0.066; the op against float64 autograd 0.109
/ 0.066 / 0.037 at (1, 77, 768).  The module runs in about 5 s, the longest case in 0.3 s."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ln_grad_oracle as O
from tests.test_gpu_gemm_designed import Buf, in_buf, out_buf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def ws_bytes(L, rows, D):
    n = ctypes.c_size_t()
    L.check(L.lib.vtd_layernorm_backward_workspace_bytes(rows, D, ctypes.byref(n)), "workspace")
    return n.value


def lib_ranges(L, rows, D=4):
    return ws_bytes(L, rows, D) // (8 * D)


def device_stats(L, xptr, rows, D, ldx, dev):
    st = torch.empty((rows, 2), device=dev, dtype=torch.float32)
    L.check(L.lib.vtd_layernorm_stats(xptr, L.F32, rows, D, ldx, O.EPS, st.data_ptr(),
                                      L.stream_ptr()), "vtd_layernorm_stats")
    return st


def leading(D, path):
    """ldx, lddy, lddx, ldadd, all above D."""
    return (D + 4, D + 8, D + 12, D + 16) if path == "vec" else (D + 1, D + 2, D + 3, D + 5)


def unchanged_outside(buf, got):
    m = buf.mask
    assert np.array_equal(got.view(np.uint32)[~m], buf.initial().view(np.uint32)[~m]), \
        "bytes outside the written elements changed"


def run(L, dev, c, add_mode, params=True, x_shift=0, lds=None, stat=None):
    """One call inside guards.  add_mode None / "separate" / "alias"; x_shift: x starts that
    many floats past a 256-byte boundary; stat: host statistics to use instead of the device's.
    Returns (dx, dgamma, dbeta, stat), numpy."""
    D, rows = c.D, c.rows
    path = O.route(D, misaligned=x_shift % 4 != 0)
    ldx, lddy, lddx, ldadd = lds or leading(D, path)
    if x_shift:
        body = np.full(rows * ldx + x_shift, np.nan, np.float32)
        v = body[x_shift:].reshape(rows, ldx)
        v[:, :D] = c.x
        xb = Buf(dev, body.reshape(1, -1), "in")
    else:
        xb = in_buf(dev, c.x, ldx)
    xptr = xb.ptr + 4 * x_shift
    dyb, gb = in_buf(dev, c.dy, lddy), in_buf(dev, c.gamma, D)
    stat = device_stats(L, xptr, rows, D, ldx, dev) if stat is None else \
        torch.tensor(stat, device=dev)
    mask = np.zeros((rows, lddx), bool)
    mask[:, :D] = True
    addptr = None
    if add_mode == "alias":
        init = np.zeros((rows, lddx), np.float32)
        init[:, :D] = c.add
        dxb = out_buf(dev, rows, lddx, np.float32, mask, init)
        addptr, ldadd = dxb.ptr, lddx
    else:
        dxb = out_buf(dev, rows, lddx, np.float32, mask)
        if add_mode == "separate":
            ab = in_buf(dev, c.add, ldadd)
            addptr = ab.ptr
    dgb = dbb = ws = None
    n = 0
    if params:
        dgb = out_buf(dev, 1, D, np.float32, np.ones((1, D), bool))
        dbb = out_buf(dev, 1, D, np.float32, np.ones((1, D), bool))
        n = ws_bytes(L, rows, D)
        ws = torch.full((n,), 0xA5, device=dev, dtype=torch.uint8)
    L.check(L.lib.vtd_layernorm_backward(
        xptr, ldx, stat.data_ptr(), gb.ptr, dyb.ptr, lddy, addptr, ldadd, rows, D, dxb.ptr, lddx,
        dgb.ptr if params else None, dbb.ptr if params else None, L.ptr(ws), n, L.stream_ptr()),
        "vtd_layernorm_backward")
    torch.cuda.synchronize()
    dx = dxb.read()
    unchanged_outside(dxb, dx)
    for b in (xb, dyb, gb):
        b.read()                                           # input guards intact
    dg = dgb.read()[0] if params else None
    db = dbb.read()[0] if params else None
    return dx[:, :D].copy(), dg, db, stat.cpu().numpy()


def check_case(L, dev, c, x_shift=0):
    path = O.route(c.D, misaligned=x_shift % 4 != 0)
    worst = [0.0, 0.0, 0.0]
    results = {}
    for add_mode in (None, "separate", "alias"):
        got = run(L, dev, c, add_mode, x_shift=x_shift)
        again = run(L, dev, c, add_mode, x_shift=x_shift)
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two runs differ"
        ref = O.backward64(c.x, got[3], c.gamma, c.dy, c.add if add_mode else None)
        r = O.ratios(got[:3], ref, c.D, c.rows, path)
        worst = [max(a, b) for a, b in zip(worst, r)]
        results[add_mode] = got
    # add does not reach the parameter gradients; separate and aliased add give the same bits
    for k in (1, 2):
        assert np.array_equal(results[None][k], results["separate"][k])
    assert np.array_equal(results["separate"][0], results["alias"][0])
    print(f"{c!r} {path}: fractions of the bars dx {worst[0]:.3f} dgamma {worst[1]:.3f} "
          f"dbeta {worst[2]:.3f} (k_dx {O.k_dx(c.D, path)}, k_param {O.k_param(c.rows)})")
    assert max(worst) <= 1.0, worst
    return results


def test_restated_geometry_is_the_library_s(L):
    # the smallest count with two ranges, from the workspace function: the first range then
    # holds rows - 1 rows and the last one a single row, ragged
    rows = 1
    while lib_ranges(L, rows) < 2:
        rows += 1
    assert lib_ranges(L, rows) == 2 and rows - 1 > 1
    assert rows == O.row_counts()[2]
    for c in O.shape_cases() + O.reduce_cases():
        assert lib_ranges(L, c.rows, c.D) == O.ranges(c.rows)


@pytest.mark.parametrize("c", O.shape_cases(), ids=repr)
def test_shapes(L, cuda, c):
    check_case(L, cuda, c)


@pytest.mark.parametrize("c", O.design_cases(), ids=repr)
def test_designed_rows(L, cuda, c):
    res = check_case(L, cuda, c)
    if c.gamma_mode == "zero":
        assert not res[None][0].any()
        assert np.array_equal(res["separate"][0], c.add)


@pytest.mark.parametrize("c", O.reduce_cases(), ids=repr)
def test_many_ranges(L, cuda, c):
    check_case(L, cuda, c)


def test_misaligned_base_takes_the_generic_path(L, cuda):
    c = O.Case(768, 9)
    lds = (772, 776, 780, 784)
    aligned = run(L, cuda, c, "separate", lds=lds)
    shifted = run(L, cuda, c, "separate", x_shift=1, lds=lds, stat=aligned[3])
    ref = O.backward64(c.x, shifted[3], c.gamma, c.dy, c.add)
    r = O.ratios(shifted[:3], ref, c.D, c.rows, "generic")
    print(f"misaligned x, generic path: fractions of the bars {r}")
    assert max(r) <= 1.0
    # the two paths agree within the bar on dx and sum dgamma / dbeta in one order
    assert (np.abs(aligned[0].astype(np.float64) - shifted[0])
            <= O.k_dx(c.D, "generic") * O.U * ref["den_x"]).all()
    assert np.array_equal(aligned[1], shifted[1]) and np.array_equal(aligned[2], shifted[2])
    # a leading dimension that is no multiple of 4 does the same
    odd = run(L, cuda, c, "separate", lds=(769, 770, 771, 773), stat=aligned[3])
    assert max(O.ratios(odd[:3], ref, c.D, c.rows, "generic")) <= 1.0
    assert np.array_equal(odd[0], shifted[0])


def test_without_parameter_gradients(L, cuda):
    for c in (O.Case(768, 9), O.Case(7, 5)):
        full = run(L, cuda, c, "separate")
        only = run(L, cuda, c, "separate", params=False)
        assert only[1] is None and np.array_equal(full[0], only[0])


@pytest.mark.parametrize("shape", O.OP_SHAPES)
def test_op(L, cuda, shape):
    import vision_transformer_detector_amd as vtd
    from vision_transformer_detector_amd import layernorm as LN
    D, rows = shape[-1], shape[0] * shape[1]
    c = O.op_case(shape)
    x = torch.tensor(c.x.reshape(shape), device=cuda, requires_grad=True)
    g = torch.tensor(c.gamma, device=cuda, requires_grad=True)
    b = torch.tensor(c.beta, device=cuda, requires_grad=True)
    dy = torch.tensor(c.dy.reshape(shape), device=cuda)
    y = vtd.layer_norm(x, g, b)
    y.backward(dy)
    np.testing.assert_allclose(y.detach().cpu().numpy().reshape(rows, D),
                               O.forward64(c.x, c.gamma, c.beta), rtol=1e-5, atol=1e-5)
    # bit for bit the C call on the same statistics
    x2d = x.detach().reshape(rows, D)
    stat = device_stats(L, x2d.data_ptr(), rows, D, D, cuda)
    dx, dg, db = LN.backward(x2d, stat, g.detach(), dy.reshape(rows, D))
    assert torch.equal(x.grad.reshape(rows, D), dx) and torch.equal(g.grad, dg)
    assert torch.equal(b.grad, db)
    # float64 torch autograd, its own statistics
    x64 = torch.tensor(c.x, dtype=torch.float64, requires_grad=True)
    g64 = torch.tensor(c.gamma, dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor(c.beta, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(x64, (D,), g64, b64, eps=O.EPS).backward(
        torch.tensor(c.dy, dtype=torch.float64))
    den = O.backward64(c.x, O.stats64(c.x), c.gamma, c.dy)
    r = [O.ratio(x.grad.cpu().numpy().reshape(rows, D), x64.grad.numpy(), den["den_x"],
                 O.k_dx(D, "vec") * O.U),
         O.ratio(g.grad.cpu().numpy(), g64.grad.numpy(), den["den_g"], O.k_param(rows) * O.U),
         O.ratio(b.grad.cpu().numpy(), b64.grad.numpy(), den["den_b"], O.k_param(rows) * O.U)]
    print(f"layer_norm {shape} against float64 autograd: fractions of the bars {r}")
    assert max(r) <= 1.0
    # a tensor that needs no gradient gets none; x alone still works
    x.grad = None
    vtd.layer_norm(x, g.detach(), b.detach()).backward(dy)
    assert torch.equal(x.grad.reshape(rows, D), dx)
    for bad in (dict(gamma=g[:-1]), dict(x=x.double()), dict(beta=b.cpu()), dict(eps=0.0)):
        kw = dict(x=x, gamma=g, beta=b, eps=1e-3)
        kw.update(bad)
        with pytest.raises(ValueError):
            vtd.layer_norm(kw["x"], kw["gamma"], kw["beta"], kw["eps"])


def test_argument_errors_touch_no_output(L, cuda):
    c = O.Case(64, 9)
    D, rows = c.D, c.rows
    xb, dyb, gb = in_buf(cuda, c.x, D), in_buf(cuda, c.dy, D), in_buf(cuda, c.gamma, D)
    stat = device_stats(L, xb.ptr, rows, D, D, cuda)
    dxb = out_buf(cuda, rows, D, np.float32, np.ones((rows, D), bool))
    dgb = out_buf(cuda, 1, D, np.float32, np.ones((1, D), bool))
    dbb = out_buf(cuda, 1, D, np.float32, np.ones((1, D), bool))
    n = ws_bytes(L, rows, D)
    ws = torch.full((n,), 0xA5, device=cuda, dtype=torch.uint8)
    ok = dict(x=xb.ptr, ldx=D, stat=stat.data_ptr(), gamma=gb.ptr, dy=dyb.ptr, lddy=D, add=None,
              ldadd=0, rows=rows, D=D, dx=dxb.ptr, lddx=D, dgamma=dgb.ptr, dbeta=dbb.ptr,
              ws=ws.data_ptr(), ws_bytes=n)
    bad = [(dict(x=None), -1), (dict(stat=None), -1), (dict(gamma=None), -1), (dict(dy=None), -1),
           (dict(rows=0), -1), (dict(D=-1), -1), (dict(ldx=D - 1), -1), (dict(lddy=D - 1), -1),
           (dict(lddx=D - 1), -1), (dict(add=dyb.ptr, ldadd=D - 1), -1), (dict(dgamma=None), -1),
           (dict(dbeta=None), -1), (dict(ws=None), -1), (dict(ws_bytes=n - 1), -4),
           (dict(ws_bytes=0), -4)]
    for kw, code in bad:
        a = dict(ok, **kw)
        rc = L.lib.vtd_layernorm_backward(a["x"], a["ldx"], a["stat"], a["gamma"], a["dy"],
                                          a["lddy"], a["add"], a["ldadd"], a["rows"], a["D"],
                                          a["dx"], a["lddx"], a["dgamma"], a["dbeta"], a["ws"],
                                          a["ws_bytes"], L.stream_ptr())
        assert rc == code, (kw, rc, L.lib.vtd_last_error())
    torch.cuda.synchronize()
    for b in (dxb, dgb, dbb):
        assert np.array_equal(b.read().view(np.uint32), b.initial().view(np.uint32))
    assert bool((ws == 0xA5).all())
