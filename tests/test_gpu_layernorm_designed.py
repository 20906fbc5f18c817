"""The LayerNorm family (csrc/vtd_elementwise.hip) on designed rows against float64, every
dispatch branch, every device buffer inside guard bands, through the C-ABI.

Rows, references, bounds, the restated dispatch (`route`) and the tables of cases come from
tests/ln_designs.py (see its docstring); tests/test_ln_designs_host.py shows on the CPU that
the same checks pass a faithful fp32 emulation of the kernels and fail nine seeded defects.
In short: order-free rows x = m + h k (sum(k) == 0) make the mean, every deviation and the sum
of squares exact in fp32 in any summation order, so `mean` must be bit-exact, rstd within 2^-22
and f32 y within 4 x 2^-23 (|p| + |beta|) of float64 in every lane layout; constant rows give
y == beta byte for byte (and, with a designed beta, an independent byte-exact reference for the
fused MX-fp8 quantizer from oracle/mx8.py); general N(1, 3) rows and one high-offset row per case
are held to 8 x the error of fp32 numpy evaluations of the same formula + 4 ulp.  Every case
asserts its route; the route table covers every instantiation of the family.

Buffers follow tests/test_gpu_gemm_designed.py: x pad columns [D, ldx), the lead-in of a
misaligned x / gamma / beta and all input guards are NaN; gamma and beta hold exactly D elements;
outputs are 0xA5 outside what the contract writes (before the buffer, rows past `rows`, MX
columns [Kq, ldq), scale rows past `rows`) and must come back bit for bit; output columns
[D, ldy) must be zero; ldx != ldy, ldy - D in {0, 4, 100}.

Measured on an MI355X, worst over all cases (the tests print these figures):
  vtd_layernorm                 designed rows, error / bound 0.387; general rows, device error /
                                fp32-numpy error 1.89 (10.2 against numpy's pairwise evaluation
                                alone: D = 63, offset 1e3, see ln_designs on the yardstick)
  vtd_layernorm_stats           designed 0.452 of 2^-22, every mean bit-exact; general 2.36 (5.10
                                pairwise alone); rstd bit-equal to the numpy fp32 value in 660 of
                                696 rows
  vtd_layernorm_stats_finalize  designed 0.469 of 2^-22, every mean bit-exact, knob launches
                                bit-equal to the default; general 2.41; rstd bit-equal to the
                                numpy fp32 merge in 18619 of 18653 rows
  vtd_layernorm_mx8             byte equality with oracle/mx8.py (constant rows) and with
                                vtd_layernorm (bf16) + vtd_quantize_mx8, f32 input included: the
                                16- and the 4-column kernel agree on order-free rows, no FMA
                                contraction difference shows
  vtd_fold_layernorm            equality
No case is skipped and no kernel bug was found; the comment on ln16_ok was corrected.  The module
runs in 3.2 s, the longest test in 0.5 s.
"""
import time

import numpy as np
import pytest
import torch

from tests import ln_designs as LD
from tests.test_gpu_bf16x3 import split_np
from tests.test_gpu_gemm_designed import Buf, check_out, col_mask, collect, in_buf, out_buf

pytestmark = pytest.mark.gpu

REPORTS = {}


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def report(entry):
    return REPORTS.setdefault(entry, LD.Report())


def show(*entries):
    for e in entries:
        print(f"{e}: {report(e)}")


class Operands:
    """x, gamma, beta of one case on the device, inside NaN guards, at their offsets."""

    def __init__(self, L, dev, c, beta=None):
        self.c, self.dev = c, dev
        self.xb = Buf(dev, c.x_body(), "in")
        self.gb = in_buf(dev, c.vec_body(c.gamma), c.g_off + c.D)
        self.bb = in_buf(dev, c.vec_body(c.beta if beta is None else beta), c.g_off + c.D)
        self.x = self.xb.ptr + c.x_off * c.isz
        self.g, self.b = self.gb.ptr + 4 * c.g_off, self.bb.ptr + 4 * c.g_off
        self.xcode = L.BF16 if c.xdt == "bf16" else L.F32
        m = c.mis()
        assert (self.x % 16, self.g % 16, self.b % 16) == (m["x_mis"], m["g_mis"], m["b_mis"])


def all_true(rows, ld):
    return np.ones((rows, ld), bool)


def run_layernorm(L, ops, out, P, route):
    """vtd_layernorm into a guarded buffer; returns the [rows][D] result (f32 values or bf16
    bits; for a split output the whole [rows][2 P] body)."""
    c = ops.c
    ldy = 2 * P if out == "split" else P
    o = out_buf(ops.dev, c.rows, ldy, np.float32 if out == "f32" else np.uint16,
                all_true(c.rows, ldy))
    assert o.ptr % 16 == 0 and c.route("layernorm", P=P, out=out) == route
    code = {"f32": L.F32, "bf16": L.BF16, "split": L.BF16X3}[out]
    L.check(L.lib.vtd_layernorm(ops.x, ops.xcode, c.rows, c.D, c.ldx, ops.g, ops.b, 1e-3, o.ptr,
                                ldy, code, L.stream_ptr()), "layernorm")
    torch.cuda.synchronize()
    got = o.read()                                        # both guards intact
    if out == "split":
        return got
    bits = got.view(np.uint32 if out == "f32" else np.uint16)
    assert (bits[:, c.D:] == 0).all(), "output columns [D, ldy) must be zero"
    return got[:, :c.D]


def run_stats(L, ops, route):
    c = ops.c
    st = out_buf(ops.dev, c.rows, 2, np.float32, all_true(c.rows, 2))
    assert c.route("layernorm_stats") == route
    L.check(L.lib.vtd_layernorm_stats(ops.x, ops.xcode, c.rows, c.D, c.ldx, 1e-3, st.ptr,
                                      L.stream_ptr()), "layernorm_stats")
    torch.cuda.synchronize()
    return st.read()


def run_mx8(L, ops, Kq, route):
    """vtd_layernorm_mx8 into guarded buffers: (bytes [rows][Kq], scales [rows][Kq / 32], the
    buffers).  ldq = Kq + 16 and s_rows = rows + 3: what lies past Kq / rows must stay 0xA5."""
    c = ops.c
    ldq, s_rows = Kq + 16, c.rows + 3
    q = out_buf(ops.dev, c.rows, ldq, np.uint8, col_mask(c.rows, ldq, (0, Kq)))
    _, smask = LD.scale_body(np.zeros((c.rows, Kq // 32), np.uint8), s_rows, 0)
    s = out_buf(ops.dev, Kq // 128, 4 * s_rows, np.uint8, smask)
    assert c.route("layernorm_mx8", Kq=Kq) == route
    L.check(L.lib.vtd_layernorm_mx8(ops.x, ops.xcode, c.rows, c.D, c.ldx, ops.g, ops.b, 1e-3,
                                    q.ptr, ldq, Kq, s.ptr, s_rows, L.stream_ptr()),
            "layernorm_mx8")
    torch.cuda.synchronize()
    return q, s, s_rows


def unfused_mx8(L, dev, ybits, Kq):
    """vtd_quantize_mx8 of the bf16 LayerNorm output (the [rows][D] bits the bf16 case returned)."""
    rows, D = ybits.shape
    ld = -(-D // 8) * 8
    h = np.zeros((rows, ld), np.uint16)
    h[:, :D] = ybits
    ht = torch.from_numpy(h.view(np.int16)).to(dev)
    q = torch.full((rows, Kq), 0x7F, dtype=torch.uint8, device=dev)
    s = torch.full((Kq // 128, rows, 4), 0xFF, dtype=torch.uint8, device=dev)
    L.check(L.lib.vtd_quantize_mx8(ht.data_ptr(), L.BF16, rows, D, ld, Kq, q.data_ptr(), Kq,
                                   s.data_ptr(), rows, L.stream_ptr()), "quantize_mx8")
    torch.cuda.synchronize()
    return q.cpu().numpy(), s.cpu().numpy().transpose(1, 0, 2).reshape(rows, Kq // 32)


def scales_of(sbuf, rows, s_rows):
    """The device scale layout [Kq / 128][s_rows][4] -> [rows][Kq / 32]; the rest untouched."""
    got = sbuf.read()
    bits = got.reshape(got.shape[0], s_rows, 4)
    assert (bits[:, rows:] == 0xA5).all(), "scale rows past `rows` were written"
    return bits[:, :rows].transpose(1, 0, 2).reshape(rows, -1)


LANE_COLUMNS = {"layernorm_kernel": 4, "layernorm_mx8_kernel": 4, "layernorm16_kernel": 16,
                "layernorm16_mx8_kernel": 16, "layernorm_generic_kernel": 1}


def one_case(L, dev, c):
    """Every call of ln_designs.calls(c): the three output forms, the statistics, and the fused
    MX-fp8 output against the unfused pair."""
    ops = Operands(L, dev, c)
    y32 = ybits = plain = None
    rep_y, rep_s = LD.Report(), LD.Report()
    for call in LD.calls(c):
        route, entry = call["route"], call["entry"]
        what = f"{c} {entry} {call.get('out', '')} {route}"
        if entry == "layernorm":
            got = run_layernorm(L, ops, call["out"], call["P"], route)
            if call["out"] == "f32":
                y32 = got
                LD.check_y(c, "f32", got, rep_y, what, route)
            elif call["out"] == "bf16":
                ybits, plain = got, route
                LD.check_y(c, "bf16", got, None, what, route)
            else:
                # the f32 output of this same case is what met float64
                assert np.array_equal(got, split_np(y32, call["P"], 0)), \
                    f"{what}: split output != split_np(f32 output)"
        elif entry == "layernorm_stats":
            LD.check_stats(c, run_stats(L, ops, route), rep_s, what, route)
        else:
            Kq = call["Kq"]
            q, s, s_rows = run_mx8(L, ops, Kq, route)
            qf = q.read()
            assert (qf[:, Kq:] == 0xA5).all(), f"{what}: columns [Kq, ldq) were written"
            sf = scales_of(s, c.rows, s_rows)
            qu, su = unfused_mx8(L, dev, ybits, Kq)
            # order-free and constant rows: equal by construction in any lane layout; the other
            # rows where both sides sum in the same lane order (the kernels' stated property)
            same = LANE_COLUMNS[route[0]] == LANE_COLUMNS[plain[0]]
            keep = np.ones(c.rows, bool) if same else c.designed
            assert np.array_equal(qf[keep, :Kq], qu[keep]) and np.array_equal(sf[keep], su[keep]), \
                f"{what}: fused != layernorm (bf16) + quantize_mx8 on rows " \
                f"{np.argwhere((qf[:, :Kq] != qu).any(1) | (sf != su).any(1)).ravel().tolist()}"
            assert (qf[:, c.D:Kq] == 0).all() and (sf[:, -(-c.D // 32):] == 1).all()
    ops.xb.read(), ops.gb.read(), ops.bb.read()          # input guards untouched
    print(f"{c}\n  y: {rep_y}\n  stats: {rep_s}")
    report("vtd_layernorm").merge(rep_y)
    report("vtd_layernorm_stats").merge(rep_s)


@pytest.mark.parametrize("xdt,rows", [(t, r) for t in ("f32", "bf16") for r in (1, 11)])
def test_layernorm_family(L, cuda, xdt, rows):
    t0 = time.perf_counter()
    cases = LD.ln_cases(xdt, rows)
    collect(cases, lambda c: one_case(L, cuda, c))
    show("vtd_layernorm", "vtd_layernorm_stats")
    print(f"{len(cases)} cases in {time.perf_counter() - t0:.2f} s")


def test_layernorm_mx8_constant_rows(L, cuda):
    """A constant row's fused output is the MX-fp8 quantization of bf16(beta): bytes and scale
    bytes from oracle/mx8.py, on both fused kernels, every NC / NV, both input dtypes."""
    t0 = time.perf_counter()
    cases = LD.mx_const_cases()

    def one(c):
        ops = Operands(L, cuda, c)
        for wide in (False, True):
            Kq = LD.mx_kq(c, wide)
            if wide and c.D not in LD.MX_WIDE:
                continue
            route = c.route("layernorm_mx8", Kq=Kq)
            assert route[0] in LD.MX_D and (c.x_off or c.D in LD.MX_D[route[0]]), route
            q, s, s_rows = run_mx8(L, ops, Kq, route)
            want_q, want_s = LD.mx_expected(np.broadcast_to(c.beta, (c.rows, c.D)), Kq)
            wq = np.zeros(q.shape, np.uint8)
            wq[:, :Kq] = want_q
            check_out(s, LD.scale_body(want_s, s_rows, 0)[0], f"{c} Kq {Kq} {route} scales")
            check_out(q, wq, f"{c} Kq {Kq} {route} bytes")
    collect(cases, one)
    print(f"{len(cases)} cases in {time.perf_counter() - t0:.2f} s")


def test_harness_notices_one_changed_element(L, cuda):
    """One element of an order-free row changed by one step h in the uploaded x (the expectation
    unchanged): the mean stops being exact."""
    c = LD.Case("f32", 11, 4096)
    one_case(L, cuda, c)
    c.x = c.x.copy()
    c.x[1, 4095] += np.float32(0.125)
    ops = Operands(L, cuda, c)
    c.x[1, 4095] -= np.float32(0.125)
    with pytest.raises(AssertionError, match="must be exact"):
        LD.check_stats(c, run_stats(L, ops, c.route("layernorm_stats")))
    with pytest.raises(AssertionError, match="outside the bound"):
        route = c.route("layernorm", P=4096)
        LD.check_y(c, "f32", run_layernorm(L, ops, "f32", 4096, route), kernel=route)


# ------------------------------------------------------------------ vtd_layernorm_stats_finalize
def run_finalize(L, dev, p, knob=-1):
    part = in_buf(dev, p.part, 2)
    st = out_buf(dev, p.rows, 2, np.float32, all_true(p.rows, 2))
    args = (part.ptr, p.rows, p.slots, p.D, 1e-3, st.ptr, L.stream_ptr())
    if knob > 0:
        with L.knob(L.KNOB_FIN_WGS, knob):
            L.check(L.lib.vtd_layernorm_stats_finalize(*args), "finalize")
    else:
        L.check(L.lib.vtd_layernorm_stats_finalize(*args), "finalize")
    torch.cuda.synchronize()
    part.read()
    return st.read()


def test_stats_finalize_on_hand_made_partials(L, cuda):
    t0 = time.perf_counter()
    rep = report("vtd_layernorm_stats_finalize")
    default = {}

    def unrolled(case):
        s, r, knob = case
        assert LD.route("layernorm_stats_finalize", slots=s) == ("ln_stats_finalize_s_kernel", s)
        p = LD.Partials(r, s)
        got = run_finalize(L, cuda, p, knob)
        p.check(got, rep, f"finalize {case}")
        if knob < 0:
            default[(s, r)] = got
        else:
            assert np.array_equal(got.view(np.uint32), default[(s, r)].view(np.uint32)), \
                "the grid-stride launch and the default launch differ"
    collect(LD.FIN_UNROLLED, unrolled)

    def generic(case):
        s, r = case
        assert LD.route("layernorm_stats_finalize", slots=s) == ("ln_stats_finalize_kernel", 0)
        p = LD.Partials(r, s, seed=1)
        p.check(run_finalize(L, cuda, p), rep, f"finalize {case}")
    collect(LD.FIN_GENERIC, generic)

    for rows, slots in ((300, 12), (257, 13)):              # block means N(200, 2)
        p = LD.Partials(rows, slots, general=True)
        p.check(run_finalize(L, cuda, p), rep, f"finalize general {rows} x {slots}")
    show("vtd_layernorm_stats_finalize")
    print(f"{time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ vtd_fold_layernorm
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fold_layernorm_designed(L, cuda, dtype):
    def one(case):
        (N, K, ldw, ldo), with_bias = case
        f = LD.Fold(N, K, ldw, ldo)
        w = in_buf(cuda, f.w, ldw)
        g, b = in_buf(cuda, f.gamma, K), in_buf(cuda, f.beta, K)
        bi = in_buf(cuda, f.bias_in, N)
        np_dt = np.float32 if dtype == "f32" else np.uint16
        wo = out_buf(cuda, N, ldo, np_dt, all_true(N, ldo))
        bo = out_buf(cuda, 1, N, np.float32, all_true(1, N))
        cs = out_buf(cuda, 1, N, np.float32, all_true(1, N))
        L.check(L.lib.vtd_fold_layernorm(w.ptr, N, K, ldw, g.ptr, b.ptr,
                                         bi.ptr if with_bias else None, wo.ptr, ldo,
                                         L.F32 if dtype == "f32" else L.BF16, bo.ptr, cs.ptr,
                                         L.stream_ptr()), "fold_layernorm")
        torch.cuda.synchronize()
        w_out, bias, colsum = f.expected(with_bias, dtype == "bf16")
        what = f"fold {dtype} {case}"
        check_out(wo, w_out if dtype == "f32" else LD.bf16_bits(w_out), what + " w_out")
        check_out(bo, bias.reshape(1, N), what + " bias_out")
        check_out(cs, colsum.reshape(1, N), what + " colsum")
        for buf in (w, g, b, bi):
            buf.read()
    collect([(s, wb) for s in LD.FOLD_SHAPES for wb in (False, True)], one)
