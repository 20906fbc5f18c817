"""The GEMM family against EXACT expected outputs on designed operands, every dispatch branch,
with every device buffer inside guard bands.

Operands come from tests/gemm_designs.py: small integers (bf16 / f32) or h + l / 256 split
pieces (bf16x3) dressed with exact power-of-two row, column and K-block scales, such that every
partial sum in any order is an fp32 number.  A correct kernel therefore returns the expected
array as numbers -- np.array_equal, no tolerance -- and a dropped, doubled or misplaced
element, row, column, K-block or tile does not.  BRANCHES is the table of what is run and how
each shape reaches its kernel; `route` restates gemm_launch's conditions and every case
asserts its route.

Guard bands: every device operand and output is a view inside one larger allocation with a
leading dimension larger than its width and, on each side, a guard of at least 256 rows of
that leading dimension and 64 KiB.  Input guards and pad columns hold NaN; output guards and
the pads the contract does not write hold the byte 0xA5 and must come back bit for bit; pads
the contract writes must hold that value (dW columns [N, ldw) zero).  Regions a kernel may read
hold finite contract-conforming values: the MX scale rows up to sa_rows / sb_rows, wgrad
operand columns up to the piece width (zero).

MX-fp8 keeps a tolerance (the scaled MFMA's internal reduction is not known to be exact): the
project's own bounds of test_gpu_mx8.py on the problem normalized by its row / column scales.

Activation epilogue (GELU-tanh / Mish forward) against float64 over the value range: bound
5 x the error of the same fp32 formulas in numpy (the margin rule of test_gpu_act_grad.py for
the ~1-ulp v_exp_f32 / v_rcp_f32).  Measured on an MI355X, worst |got - ref64| / max(1, |ref64|):
  Mish  1.89e-7 at z = 9.46 (scalar apply_act, f32 operands), 1.87e-7 at z = 9.1875 (packed
        act_mish2, both accumulator layouts); the numpy fp32 formulas give 1.59e-7 at z = 8.75;
  GELU  1.22e-7 at z = 1.95 (scalar), 1.13e-7 at z = 1.5 (packed); numpy 1.14e-7 at z = 2.52
        (1.18e-7 at z = 1.5703 on the bf16-representable grid).
"""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import mx8 as MX
from tests import gemm_designs as G
from tests.test_gpu_act_grad import grid_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


# ------------------------------------------------------------------ the branch table
SK_M = (1, 15, 16, 17, 63, 64, 65, 130)
SK_N = (1, 6, 17, 31, 32, 33, 320)
SK_K = (64, 512, 576, 1088, 2048)
SK_P = (64, 192, 1024)
TN_M = (1, 127, 128, 129, 257)
TN_N = (1, 17, 64, 127, 129, 200)
TN_K = (64, 128, 192, 320)
PP_M = (1, 255, 256, 257, 513)
PP_N = (328, 513, 520)
PP_N_NOSKINNY = (72, 255, 256, 264)
PP_KSTEPS = (1, 2, 3, 4, 5, 7, 8, 9)
TILE_GRIDS = ((1, 3), (2, 3), (3, 5), (2, 7))
SPLITK_BF16 = ((3, 3), (5, 2), (17, 4))
# bf16x3 (K-steps of the 3 P loop, ksplit): wrap (at 2 P / 64) on the boundary of the last range
# (3, 3: ranges of 1, wrap at 2; 9, 3: ranges of 3, wrap at 6), inside the last range (15, 2:
# ranges of 8 and 7, wrap at 10), inside a middle range (51, 4: ranges of 13, wrap at 34)
SPLITK_X3 = ((3, 3), (9, 3), (15, 2), (51, 4))
WG_M = (1, 31, 32, 33, 95, 300)
WG_KN = (1, 6, 17, 127, 128, 129)
MX_SHAPES = ((37, 29, 128), (257, 264, 256), (300, 200, 384))

BRANCHES = [
    dict(kernel="skinny", dtype=("bf16", "bf16x3"), knobs={},
         reached="bf16 operands, N <= 320 (kSkinnyMaxN) and staged K <= 2048 (bf16x3: 2 P): "
                 "gemm_launch's `skinny`; N <= 64 or few tiles keeps it off pp2",
         shapes=dict(M=SK_M, N=SK_N, K=SK_K, P=SK_P)),
    dict(kernel="tn128", dtype=("bf16", "bf16x3", "f32"), knobs={"SKINNY": (-1, 0)},
         reached="f32 below 64 tiles; bf16 / bf16x3 with N <= 64 and KNOB_SKINNY = 0, or with "
                 "N = 17 and staged K > 2048 (skinny refuses): the last else of gemm_launch",
         shapes=dict(M=TN_M, N=TN_N, K=TN_K)),
    dict(kernel="pp2", dtype=("bf16", "bf16x3"), knobs={"GEMM_TR": (0, 1), "SKINNY": (-1, 0)},
         reached="N > 320, or N > 64 with KNOB_SKINNY = 0: `few`; bf16x3 runs the wrap "
                 "(EpiArgs::aw = 2 P / 64)",
         shapes=dict(M=PP_M, N=PP_N + PP_N_NOSKINNY, ksteps=PP_KSTEPS)),
    dict(kernel="pp2-epilogues", dtype=("bf16", "bf16x3"), knobs={"GEMM_TR": (0, 1)},
         reached="pp2_fast_epilogue (bias set, ldo % 8 == 0, aligned) picks the specialised "
                 "code, full tiles the fast stores; bias NULL / N = 255 the generic epilogue",
         shapes=((256, 512, 128), (257, 328, 64), (130, 255, 64))),
    dict(kernel="tile-order", dtype=("bf16", "bf16x3"), knobs={"GEMM_NGW": (-1, 0, 1, 2, 3)},
         reached="tile_group_width: the knob when >= 0, else 4 at >= 8 n-tiles (N = 2304), 3 "
                 "at 6 (N = 1536); grouped when 0 < ngw < tiles_n, last group narrower",
         shapes=dict(grids=TILE_GRIDS, default=((257, 1536), (257, 2304)))),
    dict(kernel="splitk", dtype=("bf16", "bf16x3"), knobs={},
         reached="vtd_gemm_splitk: EPI_PARTIAL when N % 8 == 0, the generic partial store "
                 "otherwise (N = 260), then gemm_splitk_epilogue_kernel",
         shapes=dict(bf16=SPLITK_BF16, bf16x3=SPLITK_X3, N=(328, 260))),
    dict(kernel="f32-pp2", dtype=("f32",), knobs={"F32_PP2": (0, 1)},
         reached="f32 with >= 64 tiles of 256 x 256 (2049 x 1800: 9 x 8) and KNOB_F32_PP2 != 0; "
                 "0 sends the same problem to the 128 x 128 kernel",
         shapes=((2049, 1800, 64), (2049, 1800, 128), (2049, 1800, 192))),
    dict(kernel="wgrad", dtype=("bf16", "bf16x3"), knobs={},
         reached="vtd_gemm_wgrad; msplit 1 writes dW, msplit > 1 the partial planes + reduce",
         shapes=dict(M=WG_M, KN=WG_KN)),
    dict(kernel="w4", dtype=("bf16",), knobs={"GEMM_TPW": (2, 3)},
         reached="diagnostic library only (vtd_diag_build): VTD_GEMM_VARIANT = 12, and "
                 "KNOB_GEMM_TPW > 1 for the multi-tile pp2 kernel; skipped otherwise",
         shapes=dict(M=PP_M, N=PP_N)),
    dict(kernel="mx8", dtype=("fp8",), knobs={"GEMM_TR": (0, 1)},
         reached="vtd_gemm_mx8: a zero bias the fast codes, NULL the generic; KNOB_GEMM_TR = 1 "
                 "the transposed kernel where there is no residual",
         shapes=MX_SHAPES + ((256, 256, 128),)),
    dict(kernel="mx8-x4", dtype=("fp8",), knobs={},
         reached="diagnostic library only: VTD_MX_VARIANT = 2; skipped otherwise",
         shapes=MX_SHAPES),
]


def route(mode, M, N, Kcall, skinny=-1, f32_pp2=-1):
    """gemm_launch's kernel choice restated (kMinBigTiles 64, SK_KMAX 2048, kSkinnyMaxN 320)."""
    tiles = -(-M // 256) * -(-N // 256)
    big = tiles >= 64 and N > 64
    b16 = mode in ("bf16", "bf16x3")
    staged = 2 * (Kcall // 3) if mode == "bf16x3" else Kcall
    sk = b16 and staged <= 2048 and skinny != 0 and N <= (skinny if skinny >= 64 else 320)
    if b16 and (big or (N > 64 and not sk)):
        return "pp2"
    if mode == "f32" and big and f32_pp2 != 0:
        return "f32-pp2"
    return "skinny" if sk else "tn128"


# ------------------------------------------------------------------ guarded buffers
PATTERN = 0xA5
NAN = {np.dtype(np.uint16): 0x7FC0, np.dtype(np.float32): np.float32("nan"),
       np.dtype(np.uint8): 0x7F}


class Buf:
    """A [rows][ld] device array inside guards.  kind "in": guards NaN; "out": guards 0xA5."""

    def __init__(self, dev, body, kind, nan=None):
        body = np.ascontiguousarray(body)
        isz, ld = body.dtype.itemsize, body.shape[1]
        g = max(256 * ld * isz, 65536)
        g = -(-g // 256) * 256
        if kind == "in":
            guard = np.full(g // isz, NAN[body.dtype] if nan is None else nan,
                            body.dtype).view(np.uint8)
        else:
            guard = np.full(g, PATTERN, np.uint8)
        self.host = np.concatenate([guard, body.view(np.uint8).ravel(), guard])
        self.t = torch.from_numpy(self.host.copy()).to(dev)
        self.g, self.shape, self.dtype = g, body.shape, body.dtype
        self.ptr = self.t.data_ptr() + g
        assert self.ptr % 256 == 0

    def read(self):
        """The body after the call; asserts both guards are untouched."""
        back = self.t.cpu().numpy()
        n = back.size - self.g
        assert np.array_equal(back[:self.g], self.host[:self.g]), "guard before the buffer touched"
        assert np.array_equal(back[n:], self.host[n:]), "guard after the buffer touched"
        return back[self.g:n].view(self.dtype).reshape(self.shape)

    def initial(self):
        n = self.host.size - self.g
        return self.host[self.g:n].view(self.dtype).reshape(self.shape)


def in_buf(dev, data, ld, nan=None):
    """An input: data [rows][w] in a [rows][ld] body, pad columns and guards NaN (or `nan`)."""
    data = np.asarray(data)
    data = data.reshape(1, -1) if data.ndim == 1 else data
    body = np.full((data.shape[0], ld), NAN[data.dtype] if nan is None else nan, data.dtype)
    body[:, :data.shape[1]] = data
    return Buf(dev, body, "in", nan)


def out_buf(dev, rows, ld, dtype, mask, init=None):
    """An output: 0xA5 everywhere, NaN (or `init`) where `mask` says the contract writes."""
    body = np.full(rows * ld * np.dtype(dtype).itemsize, PATTERN, np.uint8).view(dtype) \
        .reshape(rows, ld)
    body[mask] = NAN[np.dtype(dtype)] if init is None else init[mask]
    b = Buf(dev, body, "out")
    b.mask = mask
    return b


def check_out(buf, want, what):
    """The written region equals `want` as numbers, everything else is unchanged."""
    got = buf.read()
    m = buf.mask
    assert m.any()
    if buf.dtype == np.uint16:
        gv, wv = G.bf16_value(got[m]), G.bf16_value(np.asarray(want, np.uint16)[m])
    else:
        gv, wv = got[m], np.asarray(want, buf.dtype)[m]
    assert not np.isnan(gv.astype(np.float64)).any(), f"{what}: NaN in the output"
    if not np.array_equal(gv, wv):
        bad = np.argwhere(m)[gv != wv]
        raise AssertionError(f"{what}: {len(bad)} of {gv.size} outputs differ, first at "
                             f"{bad[:6].tolist()}: got {gv[gv != wv][:6]}, want {wv[gv != wv][:6]}")
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[buf.dtype.itemsize]
    assert np.array_equal(got.view(bits)[~m], buf.initial().view(bits)[~m]), \
        f"{what}: a pad the contract does not write was touched"


def col_mask(rows, ld, *ranges):
    m = np.zeros((rows, ld), bool)
    for c0, c1 in ranges:
        m[:, c0:c1] = True
    return m


# ------------------------------------------------------------------ one designed vtd_gemm call
def run_gemm(L, dev, d, out="f32", fast=False, alias=False, out2=False, scatter=0, ksplit=0,
             what=""):
    """vtd_gemm (or vtd_gemm_splitk) of design d inside guards, checked exactly.
    out "f32" | "bf16" | "split"; fast: ldo % 8 == 0 and a bias (zero when the design has none)."""
    M, N, e = d.M, d.N, d.epi
    dtype = {"bf16": L.BF16, "f32": L.F32, "bf16x3": L.BF16X3}[d.mode]
    A = in_buf(dev, d.a_op, d.a_op.shape[1] + 8)
    Bt = in_buf(dev, d.b_op, d.b_op.shape[1] + 16)
    keep = [A, Bt]
    ep = L.VtdEpilogue()
    bias = e.get("bias", np.zeros(N) if fast else None)
    if bias is not None:
        b = in_buf(dev, bias.astype(np.float32), N + 4)
        keep.append(b)
        ep.bias = b.ptr
    if "rowadd" in e:
        ra = in_buf(dev, e["rowadd"].astype(np.float32), len(e["rowadd"]) + 4)
        keep.append(ra)
        ep.rowadd, ep.rowadd_period, ep.rowadd_ncols = ra.ptr, e["rowadd_period"], e["rowadd_ncols"]
    if "lnfold" in e:
        st = in_buf(dev, d.lnstat().reshape(-1), 2 * M + 4)
        cs = in_buf(dev, e["colsum"].astype(np.float32), N + 4)
        keep += [st, cs]
        ep.lnstat, ep.colsum = st.ptr, cs.ptr
    want64 = d.expected()
    rows, width = M, N
    if scatter:
        want64 = G.scatter_expected(want64, scatter)
        rows, width = want64.shape
    n8 = -(-width // 8) * 8
    # fast epilogues need ldo % 8 == 0; otherwise an odd leading dimension
    piece = n8 + 8 if fast else width + 3
    np_dt = {"f32": np.float32, "bf16": np.uint16, "split": np.uint16}[out]
    if out == "split":
        ldo = 2 * piece
        mask = col_mask(rows, ldo, (0, width), (piece, piece + width))
        hi, lo = G.cast_split(want64)
        want = np.zeros((rows, ldo), np.uint16)
        want[:, :width], want[:, piece:piece + width] = hi, lo
    else:
        ldo = piece
        mask = col_mask(rows, ldo, (0, width))
        want = np.zeros((rows, ldo), np_dt)
        want[:, :width] = G.cast_f32(want64) if out == "f32" else G.cast_bf16(want64)
    init = None
    if "resid" in e:
        r = e["resid"].astype(np.float32)
        r = r if out == "f32" else G.bf16_bits(r)
        if alias:
            init = np.zeros((rows, ldo), np_dt)
            init[:, :N] = r
        else:
            rb = in_buf(dev, r, n8 + 8 if fast else N + 5)
            keep.append(rb)
            ep.resid, ep.ldr = rb.ptr, rb.shape[1]
    o = out_buf(dev, rows, ldo, np_dt, mask, init)
    ep.out, ep.ldo = o.ptr, ldo
    ep.out_dtype = {"f32": L.F32, "bf16": L.BF16, "split": L.BF16X3}[out]
    if alias:
        ep.resid, ep.ldr = o.ptr, ldo
    ep.scatter_tokens = scatter
    o2 = None
    if out2:
        ld2 = n8 + 8 if fast else N + 1
        o2 = out_buf(dev, M, ld2, np.uint16, col_mask(M, ld2, (0, N)))
        ep.out2, ep.ldo2 = o2.ptr, ld2
    lda, ldb = A.shape[1], Bt.shape[1]
    part = None
    if ksplit:
        # [ksplit][M][N] floats, wholly written: guards of 256 rows of N on each side
        part = out_buf(dev, ksplit * M, N, np.float32, np.ones((ksplit * M, N), bool),
                       init=np.full((ksplit * M, N), 7.0, np.float32))
        L.check(L.lib.vtd_gemm_splitk(M, N, d.Kcall, A.ptr, lda, Bt.ptr, ldb, dtype,
                                      ctypes.byref(ep), part.ptr, ksplit * M * N * 4, ksplit,
                                      L.stream_ptr()), what)
    else:
        L.check(L.lib.vtd_gemm(M, N, d.Kcall, A.ptr, lda, Bt.ptr, ldb, dtype, ctypes.byref(ep),
                               L.stream_ptr()), what)
    torch.cuda.synchronize()
    check_out(o, want, what)
    if o2 is not None:
        w2 = np.zeros(o2.shape, np.uint16)
        w2[:, :N] = G.cast_bf16(want64)
        check_out(o2, w2, what + " out2")
    if part is not None:
        part.read()                                 # nothing written past ksplit M N floats
    for b in keep:                                  # inputs and their guards unchanged
        assert np.array_equal(b.read().view(np.uint8), b.initial().view(np.uint8)), what


@contextlib.contextmanager
def knobs(L, **kw):
    with contextlib.ExitStack() as st:
        for name, v in kw.items():
            st.enter_context(L.knob(getattr(L, "KNOB_" + name), v))
        yield


def collect(cases, fn):
    """Run fn(case) for every case; one assertion with every failure."""
    fails = []
    for c in cases:
        try:
            fn(c)
        except AssertionError as ex:
            fails.append(f"{c}: {ex}")
    assert not fails, f"{len(fails)} of {len(cases)} cases failed:\n" + "\n".join(fails[:12])


# ------------------------------------------------------------------ the rows of the table
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_skinny(L, cuda, mode):
    ks = SK_K if mode == "bf16" else SK_P
    cases = [(m, n, k) for m in SK_M for n in SK_N for k in ks]
    cases += [(65, 33, 576 if mode == "bf16" else 192, 13)]       # 13 columns of zero K-pad

    def one(c):
        M, N, K = c[:3]
        d = G.make_design(mode, M, N, K, kreal=K - c[3] if len(c) > 3 else None)
        assert route(mode, M, N, d.Kcall) == "skinny"
        run_gemm(L, cuda, d, what=f"skinny {mode} {c}")
    collect(cases, one)


def test_harness_notices_one_changed_element(L, cuda):
    """The exact comparison on the device notices what the random-operand tolerance lets
    through: one lo element of A zeroed in the uploaded operand (the expectation unchanged)."""
    d = G.make_design("bf16x3", 65, 33, 192)
    run_gemm(L, cuda, d, what="clean")
    m, k = np.argwhere(d.la != 0)[-1]
    d.a_op = d.a_op.copy()
    d.a_op[m, d.K + k] = 0
    with pytest.raises(AssertionError, match="outputs differ"):
        run_gemm(L, cuda, d, what="one lo element dropped")


@pytest.mark.parametrize("out", ["f32", "bf16", "split"])
@pytest.mark.parametrize("skinny", [-1, 0])
def test_small_kernels_epilogue_and_scatter(L, cuda, skinny, out):
    """The scalar epilogue (epi_store) of the skinny and the 128 x 128 kernel: every exact field,
    and the head's Reshape scatter (N = 17)."""
    T, B = 25, 3
    for mode in ("bf16", "bf16x3"):
        with knobs(L, SKINNY=skinny):
            d = G.make_design(mode, B * T, 17, 128, epi=("bias",))
            assert route(mode, d.M, 17, d.Kcall, skinny) == ("skinny" if skinny else "tn128")
            run_gemm(L, cuda, d, out=out, scatter=T, what=f"scatter {mode}")
            if out != "split":
                d = G.make_design(mode, 70, 33, 64, epi=("bias", "rowadd", "resid", "lnfold"))
                run_gemm(L, cuda, d, out=out, out2=True, what=f"all fields {mode}")
                run_gemm(L, cuda, d, out=out, alias=True, what=f"in-place residual {mode}")


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
def test_tn128(L, cuda, mode):
    if mode == "f32":
        cases = [(m, n, k, -1) for m in TN_M for n in TN_N for k in TN_K]
    else:
        cases = [(m, n, k, 0) for m in TN_M for n in (1, 17, 64) for k in TN_K]
        # staged K > 2048: the skinny kernel refuses, N = 17 stays off pp2
        cases += [(m, 17, 2112 if mode == "bf16" else 1088, -1) for m in TN_M]

    def one(c):
        M, N, K, sk = c
        d = G.make_design(mode, M, N, K)
        assert route(mode, M, N, d.Kcall, sk) == "tn128"
        with knobs(L, SKINNY=sk):
            run_gemm(L, cuda, d, what=f"tn128 {mode} {c}")
    collect(cases, one)


@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_pp2_few_tiles(L, cuda, mode, tr):
    ns = [(n, -1) for n in PP_N] + [(n, 0) for n in PP_N_NOSKINNY]
    # every (M, K-steps) pair with N cycling, every (N, K-steps) pair with M cycling
    mk = [(m, k) for m in PP_M for k in PP_KSTEPS]
    nk = [(n, sk, k) for n, sk in ns for k in PP_KSTEPS]
    cases = [(m, ns[i % 7][0], 64 * k, ns[i % 7][1]) for i, (m, k) in enumerate(mk)]
    cases += [(PP_M[i % 5], n, 64 * k, sk) for i, (n, sk, k) in enumerate(nk)]
    cases += [(257, 328, 320, -1, 21)]                             # 21 columns of zero K-pad

    def one(c):
        M, N, K, sk = c[:4]
        d = G.make_design(mode, M, N, K, kreal=K - c[4] if len(c) > 4 else None)
        assert route(mode, M, N, d.Kcall, sk) == "pp2"
        with knobs(L, SKINNY=sk, GEMM_TR=tr):
            run_gemm(L, cuda, d, what=f"pp2 {mode} tr {tr} {c}")
    collect(cases, one)


PP2_EPILOGUES = [
    # (epilogue fields, out, fast, alias, out2)
    (("bias",), "f32", True, False, False),
    (("bias",), "bf16", True, False, False),
    (("bias",), "split", True, False, False),
    (("bias", "resid"), "f32", True, False, False),
    (("bias", "resid"), "bf16", True, True, False),
    (("bias", "resid"), "f32", True, True, True),
    (("bias", "rowadd"), "bf16", True, False, False),
    (("bias", "lnfold"), "bf16", True, False, False),
    (("bias", "lnfold"), "f32", True, False, False),
    (("bias", "rowadd", "resid", "lnfold"), "bf16", True, False, True),
    ((), "f32", False, False, False),
    ((), "split", False, False, False),
    (("rowadd", "resid", "lnfold"), "bf16", False, True, False),
    (("bias", "rowadd", "resid", "lnfold"), "f32", False, False, True),
]


@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_pp2_epilogues(L, cuda, mode, tr):
    shapes = next(b for b in BRANCHES if b["kernel"] == "pp2-epilogues")["shapes"]
    cases = [(s, e) for s in shapes for e in PP2_EPILOGUES]

    def one(c):
        (M, N, K), (fields, out, fast, alias, out2) = c
        d = G.make_design(mode, M, N, K, epi=fields)
        sk = 0 if N <= 320 else -1
        assert route(mode, M, N, d.Kcall, sk) == "pp2"
        with knobs(L, SKINNY=sk, GEMM_TR=tr):
            run_gemm(L, cuda, d, out=out, fast=fast, alias=alias, out2=out2,
                     what=f"pp2 epilogue {mode} tr {tr} {c}")
    collect(cases, one)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_tile_order(L, cuda, mode):
    cases = [(256 * (tm - 1) + 1, 256 * (tn - 1) + 72, ngw)
             for tm, tn in TILE_GRIDS for ngw in (0, 1, 2, 3)]
    cases += [(257, 1536, -1), (257, 2304, -1)]
    cases += [(2049, 2056, -1), (2049, 2056, 2)]                   # 81 tiles: gemm_launch's `big`

    def one(c):
        M, N, ngw = c
        d = G.make_design(mode, M, N, 64)
        assert route(mode, M, N, d.Kcall) == "pp2"
        with knobs(L, GEMM_NGW=ngw):
            run_gemm(L, cuda, d, fast=(ngw == -1), what=f"tile order {mode} {c}")
    collect(cases, one)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_splitk(L, cuda, mode):
    table = SPLITK_BF16 if mode == "bf16" else SPLITK_X3
    cases = [(M, N, nk, ks) for nk, ks in table for M, N in ((257, 328), (100, 260))]

    def one(c):
        M, N, nk, ks = c
        K = 64 * nk if mode == "bf16" else 64 * nk // 3
        d = G.make_design(mode, M, N, K, epi=("bias",))
        assert d.Kcall == 64 * nk
        # the unsplit call and the split one against the same expected array
        run_gemm(L, cuda, d, what=f"unsplit {mode} {c}")
        run_gemm(L, cuda, d, ksplit=ks, what=f"splitk {mode} {c}")
        run_gemm(L, cuda, d, ksplit=ks, out="bf16", fast=True, what=f"splitk bf16 out {mode} {c}")
        # the reduction's epilogue applies the LayerNorm fold, the row add and the residual
        d = G.make_design(mode, M, N, K, epi=("bias", "rowadd", "resid", "lnfold"))
        run_gemm(L, cuda, d, ksplit=ks, alias=True, what=f"splitk all fields {mode} {c}")
    collect(cases, one)


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_f32_pp2(L, cuda, K, knob):
    M, N = 2049, 1800
    d = G.make_design("f32", M, N, K, epi=("bias",) if K == 128 else ())
    assert route("f32", M, N, K, f32_pp2=knob) == ("f32-pp2" if knob else "tn128")
    with knobs(L, F32_PP2=knob):
        run_gemm(L, cuda, d, fast=(K != 192), what=f"f32 pp2 knob {knob} K {K}")


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_wgrad(L, cuda, mode):
    cases = [(m, k, n) for m in WG_M for k in WG_KN for n in WG_KN]
    dtype = L.BF16 if mode == "bf16" else L.BF16X3

    def operand(pieces, w):
        """[hi | lo] (or the bf16 row) with the piece width rounded up to 8 plus 8: the columns
        [w, piece) are zero as every producer writes them, nothing past them exists."""
        pw = -(-w // 8) * 8 + 8
        body = np.zeros((pieces[0].shape[0], pw * len(pieces)), np.uint16)
        for i, p in enumerate(pieces):
            body[:, i * pw:i * pw + w] = p
        return Buf(cuda, body, "in")

    def one(c):
        M, K, N = c
        d = G.make_wgrad_design(mode, M, K, N)
        X, Gr = operand(d.x_op, K), operand(d.g_op, N)
        choice = L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype)
        for msplit in sorted({1, min(2, -(-M // 32)), choice, -(-M // 32)}):
            ldw = N + 3
            dW = out_buf(cuda, K, ldw, np.float32, np.ones((K, ldw), bool))
            db = out_buf(cuda, 1, N + 5, np.float32, col_mask(1, N + 5, (0, N)))
            prow = msplit * (K + 1) if msplit > 1 else 1      # [msplit][K + 1][N] floats
            nfl = prow * N
            part = out_buf(cuda, prow, N, np.float32, np.ones((prow, N), bool),
                           init=np.full((prow, N), 7.0, np.float32))
            L.check(L.lib.vtd_gemm_wgrad(M, K, N, X.ptr, X.shape[1], Gr.ptr, Gr.shape[1], dtype,
                                         dW.ptr, ldw, db.ptr, part.ptr,
                                         nfl * 4 if msplit > 1 else 0, msplit, L.stream_ptr()),
                    "wgrad")
            torch.cuda.synchronize()
            want = np.zeros((K, ldw), np.float32)             # pad columns [N, ldw): zero
            want[:, :N] = G.cast_f32(d.dW)
            check_out(dW, want, f"wgrad {mode} {c} msplit {msplit} dW")
            wdb = np.zeros((1, N + 5), np.float32)
            wdb[0, :N] = G.cast_f32(d.db)
            check_out(db, wdb, f"wgrad {mode} {c} msplit {msplit} db")
            part.read()
    collect(cases, one)


def _need_diag(L):
    if not hasattr(L.lib, "vtd_diag_build"):
        pytest.skip("the w4 / multi-tile / x4 kernels are in the diagnostic build only (make diag)")


@pytest.mark.parametrize("variant", ["w4", "tpw2", "tpw3"])
def test_w4_and_multi_tile_pp2(L, cuda, monkeypatch, variant):
    _need_diag(L)
    if variant == "w4":
        monkeypatch.setenv("VTD_GEMM_VARIANT", "12")
    cases = [(PP_M[i % 5], PP_N[i % 3], 64 * PP_KSTEPS[i % 8]) for i in range(15)]

    def one(c):
        M, N, K = c
        # bias + residual (code 12) and the LayerNorm fold (4 | EPI_LNF) have multi-tile kernels
        for fields, out in (((), "f32"), (("bias",), "bf16"), (("bias", "resid"), "bf16"),
                            (("bias", "lnfold"), "bf16")):
            d = G.make_design("bf16", M, N, K, epi=fields)
            with knobs(L, GEMM_TPW=int(variant[3:]) if variant != "w4" else -1):
                run_gemm(L, cuda, d, out=out, fast=bool(fields), what=f"{variant} {c} {fields}")
    collect(cases, one)


# ------------------------------------------------------------------ MX-fp8
def _mx_operand(L, dev, x, s_rows):
    """vtd_quantize_mx8 of f32 x [rows][K] into guarded buffers: e4m3 [rows][K + 16] with NaN
    pads, scales [K / 128][s_rows][4] whose rows past `rows` (readable by the contract) hold 127
    (2^0)."""
    rows, K = x.shape
    q = torch.full((rows, K), 0x7F, dtype=torch.uint8, device=dev)
    s = torch.full((K // 128 * s_rows * 4,), 127, dtype=torch.uint8, device=dev)
    L.check(L.lib.vtd_quantize_mx8(x.data_ptr(), L.F32, rows, K, K, K, q.data_ptr(), K,
                                   s.data_ptr(), s_rows, L.stream_ptr()), "quantize_mx8")
    torch.cuda.synchronize()
    qn, sn = q.cpu().numpy(), s.cpu().numpy()
    return (in_buf(dev, qn, K + 16), in_buf(dev, sn, sn.size, nan=0xFF),
            MX.dequantize(qn, sn, rows, K))


def _mx_problem(M, N, K, span):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).float().numpy()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).numpy()
    rng = np.random.default_rng([M, N, K])
    r, c = G.exponents(M, span, rng), G.exponents(N, span, rng)
    t = np.repeat(G.kblock_exponents(K // 32), 32)         # per 32-block, balanced A against Bt
    A = A * np.exp2((r[:, None] + t[None, :]).astype(np.float32))
    W = W * np.exp2((c[:, None] - t[None, :]).astype(np.float32))
    return A.astype(np.float32), W.astype(np.float32), r, c


@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("variant", ["1", "2"])
@pytest.mark.parametrize("M,N,K", MX_SHAPES)
def test_mx8_dressed(L, cuda, monkeypatch, M, N, K, variant, tr):
    if variant == "2":
        _need_diag(L)
    monkeypatch.setenv("VTD_MX_VARIANT", variant)
    A, W, r, c = _mx_problem(M, N, K, 40)
    sa_rows, sb_rows = -(-M // 4) * 4 + 4, -(-N // 4) * 4 + 8
    qa, sa, a64 = _mx_operand(L, cuda, torch.from_numpy(A).to(cuda), sa_rows)
    qb, sb, b64 = _mx_operand(L, cuda, torch.from_numpy(W).to(cuda), sb_rows)
    norm = np.exp2(-(r[:, None] + c[None, :]).astype(np.float64))
    rng = np.random.default_rng(K)
    res64 = rng.normal(size=(M, N)) / norm                  # the residual, scaled elementwise
    for bias0, out, resid in ((True, "f32", False), (False, "f32", False), (True, "bf16", False),
                              (True, "f32", True), (False, "bf16", True)):
        ep = L.VtdEpilogue()
        keep = []
        if bias0:
            b = in_buf(cuda, np.zeros(N, np.float32), N + 4)
            keep.append(b)
            ep.bias = b.ptr
        np_dt = np.float32 if out == "f32" else np.uint16
        ldo = -(-N // 8) * 8 + 8 if bias0 else N + 3
        ref = a64 @ b64.T
        if resid:
            r32 = res64.astype(np.float32)
            rv = r32 if out == "f32" else G.bf16_bits(r32)
            rb = in_buf(cuda, rv, ldo)
            keep.append(rb)
            ep.resid, ep.ldr = rb.ptr, ldo
            ref = ref + (r32 if out == "f32" else G.bf16_value(rv)).astype(np.float64)
        o = out_buf(cuda, M, ldo, np_dt, col_mask(M, ldo, (0, N)))
        ep.out, ep.ldo, ep.out_dtype = o.ptr, ldo, L.F32 if out == "f32" else L.BF16
        with knobs(L, GEMM_TR=tr):
            L.check(L.lib.vtd_gemm_mx8(M, N, K, qa.ptr, K + 16, sa.ptr, sa_rows, qb.ptr, K + 16,
                                       sb.ptr, sb_rows, ctypes.byref(ep), L.stream_ptr()), "mx8")
        torch.cuda.synchronize()
        got = o.read()
        assert np.array_equal(got.view(np.uint8).reshape(M, -1)[:, N * got.itemsize:],
                              o.initial().view(np.uint8).reshape(M, -1)[:, N * got.itemsize:])
        gv = (got[:, :N] if out == "f32" else G.bf16_value(got[:, :N])).astype(np.float64)
        assert np.isfinite(gv).all()
        # the normalized problem is the one the project's bounds were measured on
        err = np.abs(gv * norm - ref * norm) / np.maximum(np.abs(ref * norm), 1.0)
        tol = 5e-4 if out == "f32" else 8e-3
        print(f"mx8 {M}x{N}x{K} variant {variant} tr {tr} bias {bias0} {out} resid {resid}: "
              f"worst {err.max():.3g}")
        assert err.max() < tol, (bias0, out, resid, err.max(), np.argwhere(err >= tol)[:5].tolist())
        for b in keep + [qa, sa, qb, sb]:
            b.read()


@pytest.mark.parametrize("tr", [0, 1])
def test_mx8_fp8_output_dressed_rows(L, cuda, tr):
    """(256, 256, 128), rows scaled only: the MX-fp8 output (bytes and scales) equals
    vtd_quantize_mx8 of the bf16 output of the same GEMM."""
    M, N, K = 256, 256, 128
    A, W, r, c = _mx_problem(M, N, K, 40)
    W = W * np.exp2(-c[:, None].astype(np.float32))          # columns not scaled
    qa, sa, _ = _mx_operand(L, cuda, torch.from_numpy(A).to(cuda), M)
    qb, sb, _ = _mx_operand(L, cuda, torch.from_numpy(W.astype(np.float32)).to(cuda), N)
    bias = in_buf(cuda, np.zeros(N, np.float32), N + 4)

    def run(ep):
        with knobs(L, GEMM_TR=tr):
            L.check(L.lib.vtd_gemm_mx8(M, N, K, qa.ptr, K + 16, sa.ptr, M, qb.ptr, K + 16, sb.ptr,
                                       N, ctypes.byref(ep), L.stream_ptr()), "mx8")
        torch.cuda.synchronize()

    o16 = out_buf(cuda, M, N + 8, np.uint16, col_mask(M, N + 8, (0, N)))
    ep = L.VtdEpilogue()
    ep.bias, ep.out, ep.ldo, ep.out_dtype = bias.ptr, o16.ptr, N + 8, L.BF16
    run(ep)
    v16 = o16.read()[:, :N]
    assert not np.isnan(G.bf16_value(v16)).any()
    x = torch.from_numpy(v16.copy().view(np.int16)).view(torch.bfloat16).to(cuda)
    q_ref = torch.full((M, N), 0x7F, dtype=torch.uint8, device=cuda)
    s_ref = torch.full((N // 128 * M * 4,), 0xFF, dtype=torch.uint8, device=cuda)
    L.check(L.lib.vtd_quantize_mx8(x.data_ptr(), L.BF16, M, N, N, N, q_ref.data_ptr(), N,
                                   s_ref.data_ptr(), M, L.stream_ptr()), "quantize")
    o8 = out_buf(cuda, M, N + 16, np.uint8, col_mask(M, N + 16, (0, N)))
    so = out_buf(cuda, 1, N // 128 * M * 4, np.uint8, np.ones((1, N // 128 * M * 4), bool))
    ep2 = L.VtdEpilogue()
    ep2.bias, ep2.out, ep2.ldo, ep2.out_dtype = bias.ptr, o8.ptr, N + 16, L.FP8
    ep2.scale_out, ep2.scale_rows = so.ptr, M
    run(ep2)
    got = o8.read()
    assert np.array_equal(got[:, :N], q_ref.cpu().numpy())
    assert (got[:, N:] == PATTERN).all()
    assert np.array_equal(so.read().ravel(), s_ref.cpu().numpy())


# ------------------------------------------------------------------ activation epilogue
def act_np32(z, mish):
    """The device formulas (vtd_common.h act_mish / act_gelu) restated in numpy fp32."""
    f = np.float32
    z = np.asarray(z, f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if mish:
            e = np.exp2(z * f(1.4426950408889634)).astype(f)
            n = e * (e + f(2))
            y = z * n * (f(1) / (n + f(2)))
            return np.where(z > f(20), z, y).astype(f)
        c0 = f(f(-2) * f(0.7978845608028654) * f(1.4426950408889634))
        c1 = f(c0 * f(0.044715))
        e = np.exp2(z * (c1 * (z * z) + c0)).astype(f)
        return (z * (f(1) / (f(1) + e))).astype(f)


def act_ref64(z, mish):
    z = np.asarray(z, np.float64)
    if mish:
        return z * np.tanh(np.logaddexp(0.0, z))
    return 0.5 * z * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def act_values(bf16):
    v = np.concatenate([grid_values(), np.asarray([200.0, -200.0, 1e19, -1e19], np.float32)])
    if bf16:
        v = G.bf16_value(G.bf16_bits(v))
    # an MFMA accumulator holds neither -0 nor a denormal
    v = np.where(np.abs(v) < 1.2e-38, np.float32(0), v).astype(np.float32)
    side = 128 if bf16 else 64
    pad = (-len(v)) % side
    return np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, side)


def rel_err(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))


ACT_SETUPS = [("f32", -1), ("bf16", 0), ("bf16", 1)]


@pytest.mark.parametrize("setup", ACT_SETUPS, ids=lambda s: f"{s[0]}-tr{s[1]}")
@pytest.mark.parametrize("act_name", ["mish", "gelu"])
def test_activation_epilogue_against_float64(L, cuda, act_name, setup):
    """z through an identity GEMM (the accumulator is z exactly), the activation in the epilogue,
    the output read as f32: the scalar apply_act (f32 operands, 64 x 64 identity, the 128 x 128
    kernel) and the packed act_gelu2 / act_mish2 of the pp2 epilogues (bf16 operands, 128 x 128
    identity, zero bias, KNOB_SKINNY = 0, both KNOB_GEMM_TR values)."""
    mode, tr = setup
    mish = act_name == "mish"
    z = act_values(mode == "bf16")
    M, side = z.shape
    eye = np.eye(side, dtype=np.float32)
    if mode == "bf16":
        A, Bt, dtype = in_buf(cuda, G.bf16_bits(z), side + 8), in_buf(cuda, G.bf16_bits(eye), side + 8), L.BF16
        assert route("bf16", M, side, side, 0) == "pp2"
    else:
        A, Bt, dtype = in_buf(cuda, z, side + 8), in_buf(cuda, eye, side + 8), L.F32
        assert route("f32", M, side, side) == "tn128"
    bias = in_buf(cuda, np.zeros(side, np.float32), side + 4)
    o = out_buf(cuda, M, side + 8, np.float32, col_mask(M, side + 8, (0, side)))
    ep = L.VtdEpilogue()
    ep.act = L.ACT_MISH if mish else L.ACT_GELU_TANH
    ep.out, ep.ldo, ep.out_dtype = o.ptr, side + 8, L.F32
    if mode == "bf16":
        ep.bias = bias.ptr
    with knobs(L, SKINNY=0 if mode == "bf16" else -1, GEMM_TR=tr):
        L.check(L.lib.vtd_gemm(M, side, side, A.ptr, side + 8, Bt.ptr, side + 8, dtype,
                               ctypes.byref(ep), L.stream_ptr()), "vtd_gemm")
    torch.cuda.synchronize()
    got = o.read()[:, :side]
    assert np.array_equal(o.read()[:, side:].view(np.uint32), o.initial()[:, side:].view(np.uint32))
    assert np.isfinite(got).all(), "every output must be finite"
    ref = act_ref64(z, mish)
    cpu = rel_err(act_np32(z, mish), ref)
    err = rel_err(got, ref)
    i, j = np.unravel_index(np.argmax(err), err.shape)
    ic, jc = np.unravel_index(np.argmax(cpu), cpu.shape)
    print(f"{act_name} {mode} tr {tr}: GPU worst {err.max():.3g} at z = {z[i, j]:.6g}; "
          f"CPU fp32 formulas {cpu.max():.3g} at z = {z[ic, jc]:.6g}")
    assert err.max() <= 5 * cpu.max(), (err.max(), float(z[i, j]), cpu.max())
    if mish:
        assert np.array_equal(got[z > 20], z[z > 20])        # returns z exactly
    else:
        assert np.array_equal(got[z >= 30], z[z >= 30])      # large z: z itself
        assert (got[z <= -30] == 0).all()                    # very negative z: +-0
