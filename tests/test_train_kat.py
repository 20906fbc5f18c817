"""Host checks of the whole-model training step, no device: the sparse-order Adam rule of
tests/train_oracle.py in closed form, the grouped pack and the LayerNorm fold restated in numpy
on designed values, the new C-ABI symbols, and every argument check of the new entries."""
import ctypes

import numpy as np
import pytest

from tests import adam_oracle as A
from tests import train_oracle as T

LR = 1e-3
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-7))


# ------------------------------------------------------------------ the sparse-order rule
def test_sparse_first_step_closed_form():
    """From zero moments: m = g (1 - b1), v = g^2 (1 - b2) and, with alpha_1 = lr sqrt(1 - b2) /
    (1 - b1), w moves by lr sign(g) / (1 + eps / (sqrt(1 - b2) |g|))."""
    g = np.array([0.5, -2.0, 1e-3, -7.25, 3.0])
    w0 = np.array([1.0, -1.0, 0.25, 4.0, -3.0])
    z = np.zeros_like(w0)
    w, m, v = T.sparse64(w0, z, z, g, 1, LR)
    np.testing.assert_allclose(m, g * (1 - B1), rtol=1e-15)
    np.testing.assert_allclose(v, g * g * (1 - B2), rtol=1e-15)
    move = LR * np.sign(g) / (1 + EPS / (np.sqrt(1 - B2) * np.abs(g)))
    np.testing.assert_allclose(w0 - w, move, rtol=1e-12)
    w32, m32, v32 = T.sparse32(w0, z, z, g, 1, LR)
    assert w32.dtype == np.float32
    np.testing.assert_allclose(w32, w, rtol=3e-7)
    np.testing.assert_allclose(m32, m, rtol=3e-7)
    np.testing.assert_allclose(v32, v, rtol=3e-7)
    with pytest.raises(ValueError):
        T.sparse32(w0, z, z, g, 0, LR)


def test_sparse_constant_gradient_closed_form():
    """A constant gradient: m_t = g (1 - b1^t), v_t = g^2 (1 - b2^t), so the bias correction in
    alpha cancels and step t moves w by lr sign(g) / (1 + eps / (sqrt(1 - b2^t) |g|))."""
    g = np.array([0.75, -0.125, 9.0])
    w = np.array([0.0, 1.0, -2.0])
    m = v = np.zeros_like(w)
    w0, moved = w.copy(), np.zeros_like(w)
    for t in range(1, 21):
        w, m, v = T.sparse64(w, m, v, g, t, LR)
        np.testing.assert_allclose(m, g * (1 - B1 ** t), rtol=1e-13)
        np.testing.assert_allclose(v, g * g * (1 - B2 ** t), rtol=1e-13)
        moved += LR * np.sign(g) / (1 + EPS / (np.sqrt(1 - B2 ** t) * np.abs(g)))
        np.testing.assert_allclose(w0 - w, moved, rtol=1e-11)


def test_sparse_clip_and_constraint():
    """clipvalue bounds g before the moments; the rule is unconstrained unless asked; the dense
    and the sparse order are the same function in exact arithmetic."""
    w0 = np.array([1.0, -1.0, 9.9999], np.float32)
    z = np.zeros_like(w0)
    big = np.array([37.0, -1e3, -50.0], np.float32)
    at = np.array([10.0, -10.0, -10.0], np.float32)
    a = T.sparse32(w0, z, z, big, 1, LR, clipvalue=10.0)
    b = T.sparse32(w0, z, z, at, 1, LR, clipvalue=None)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0][2] > 10.0                                   # free: past max_weight
    c = T.sparse32(w0, z, z, big, 1, LR, clipvalue=10.0, max_weight=10.0, constrain=True)
    assert c[0][2] == np.float32(10.0) and c[0][:2].tobytes() == a[0][:2].tobytes()
    nan = T.sparse32(w0, z, z, np.array([np.nan, 1.0, 1.0], np.float32), 1, LR, clipvalue=10.0)
    assert np.isnan(nan[0][0]) and np.isnan(nan[1][0])      # a NaN passes the clip
    rng = np.random.default_rng(0)
    w, g1, g2 = rng.standard_normal((3, 50))
    m = v = np.zeros(50)
    wd, md, vd = w, m, v
    for t, g in ((1, g1), (2, g2)):
        w, m, v = T.sparse64(w, m, v, g, t, LR, clipvalue=1.5)
        wd, md, vd = A.step64(wd, md, vd, g, t, LR, clipvalue=1.5, constrain=False)
    np.testing.assert_allclose(w, wd, rtol=1e-12)
    np.testing.assert_allclose(v, vd, rtol=1e-12)


def test_sparse_nan_goes_to_one_under_the_constraint():
    """ClipWeight maps a NaN weight to 1.0 before the clip (the kernel's `w != w ? 1 : w`), in
    the sparse order exactly as in step32; m and v stay NaN.  An inf gradient is clipped."""
    w0 = np.array([0.3, -0.7, 9.9995, 2.0], np.float32)
    z = np.zeros_like(w0)
    g = np.array([np.nan, 0.5, -np.inf, np.inf], np.float32)
    a = T.sparse32(w0, z, z, g, 1, LR, clipvalue=10.0, max_weight=10.0, constrain=True)
    b = A.step32(w0, z, z, g, 1, LR, clipvalue=10.0, max_weight=10.0, constrain=True)
    for w, m, v in (a, b):
        assert w[0] == 1.0 and np.isnan(m[0]) and np.isnan(v[0])
        assert w[2] == np.float32(10.0) and np.isfinite(w[1:]).all() and w[3] < w0[3]
    free = T.sparse32(w0, z, z, g, 1, LR, clipvalue=10.0, constrain=False)
    assert np.isnan(free[0][0]) and free[0][2] > 10.0


# ------------------------------------------------------------------ the grouped pack, the fold
def test_grouped_pack_restated():
    # no groups: adam_oracle.pack_ref
    w = np.arange(1, 70 * 17 + 1, dtype=np.float32).reshape(70, 17) / 8
    for fmt in ("bf16", "bf16x3"):
        assert (T.grouped_pack(w, fmt, 64, 128) == A.pack_ref(w, 128, 64, fmt)).all()
    # attention_output's shape: k_group 10 -> 32; k' = 8 .. 15 is two real columns and six pads
    w = np.arange(1, 30 * 24 + 1, dtype=np.float32).reshape(30, 24)
    out = T.grouped_pack(w, "f32", 64, 128, k_group=10, k_group_p=32)
    assert out.shape == (64, 128)
    assert (out[5, 8:16] == [w[8, 5], w[9, 5], 0, 0, 0, 0, 0, 0]).all()
    assert (out[5, 32:42] == w[10:20, 5]).all() and not out[5, 42:64].any()
    assert not out[24:].any() and not out[:, 96:].any()
    # query's shape into the middle third of a shared buffer: n_group 10 -> 32, row offset 96
    w = np.arange(1, 24 * 30 + 1, dtype=np.float32).reshape(24, 30)
    fill = np.full((288, 64), 7.0, np.float32)
    out = T.grouped_pack(w, "f32", 288, 64, n_group=10, n_group_p=32, row_offset=96, fill=fill)
    assert (out[96 + 32 + 3, :24] == w[:, 13]).all() and not out[96 + 32 + 3, 24:].any()
    assert (out[:96] == 7).all() and (out[96 + 10:96 + 32] == 7).all() and (out[192:] == 7).all()
    x3 = T.grouped_pack(w, "bf16x3", 288, 64, n_group=10, n_group_p=32, row_offset=96)
    hi, lo = A.split(w[:, 13])
    assert (x3[131, :24] == hi).all() and (x3[131, 64:88] == hi).all()
    assert (x3[131, 128:152] == lo).all()
    v = T.grouped_vector(np.arange(1, 31), 288, n_group=10, n_group_p=32, offset=96)
    assert v[96 + 64 + 9] == 30 and v[96 + 10] == 0 and v.sum() == 465


def test_fold_restated_on_designed_values():
    """Integer-valued operands: the float64 sums are exact, so the restatement is the kernel's
    answer whatever the order.  colsum comes from the ROUNDED stored product."""
    w = np.zeros((4, 8), np.float32)
    w[0] = [1, 2, 3, 4, 5, 6, 0, 0]
    w[1] = [257, 0, 0, 0, 0, 0, 0, 0]                # 257 rounds to 256 in bf16
    gamma = np.array([1, 1, 2, 2, 1, 1, 0, 0], np.float32)
    beta = np.array([1, -1, 1, -1, 2, 0, 0, 0], np.float32)
    bias = np.array([0.5, 1.0, 0.0, -2.0], np.float32)
    wo, bo, cs = T.fold(w, gamma, beta, bias)
    assert (A.bf16_value(wo[0]) == [1, 2, 6, 8, 5, 6, 0, 0]).all()
    assert bo.tolist() == [0.5 + (1 - 2 + 3 - 4 + 10), 1.0 + 257, 0.0, -2.0]
    assert cs.tolist() == [28.0, 256.0, 0.0, 0.0]
    wo32, _, cs32 = T.fold(w, gamma, beta, None, fmt="f32")
    assert wo32.dtype == np.float32 and cs32[1] == 257.0


# ------------------------------------------------------------------ the C-ABI, no device
@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


NEW = ("vtd_train_plan_bytes", "vtd_train_plan_upload", "vtd_train_step", "vtd_fold_plan_upload",
       "vtd_fold_layernorm_batch")


def test_new_symbols_are_declared_and_the_version_stays(L):
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert L.lib.vtd_abi_version() == 17 and L.ABI_VERSION == 17
    # the existing table entry keeps its layout, the new one extends it
    assert ctypes.sizeof(L.VtdAdamTensor) == 56
    assert L.VtdTrainTensor.k_group.offset == 56 and ctypes.sizeof(L.VtdTrainTensor) == 88
    assert ctypes.sizeof(L.VtdFoldJob) == 72


def _tensor(L, **kw):
    base = dict(w=16, m=32, v=48, g=64, packed=128, kind=L.ADAM_MATRIX, K=30, N=24, ld=128,
                k_group=10, k_group_p=32, n_group=24, n_group_p=24, row_offset=0,
                packed_dtype=L.TRAIN_PACK_MODE, constrain=1, rule=L.TRAIN_RULE_DENSE)
    base.update(kw)
    return L.VtdTrainTensor(**base)


def test_train_plan_argument_checks_need_no_device(L):
    nbytes, tiles = ctypes.c_size_t(), ctypes.c_int()

    def plan(t, n=1, dtype=L.BF16):
        arr = (L.VtdTrainTensor * 1)(t) if t is not None else None
        return L.lib.vtd_train_plan_bytes(arr, n, dtype, ctypes.byref(nbytes), ctypes.byref(tiles))

    assert plan(_tensor(L)) == 0
    assert tiles.value == 2 and nbytes.value > 0           # K_p = 128: two tiles of packed k'
    assert plan(_tensor(L, ld=384), dtype=L.BF16X3) == 0 and tiles.value == 2
    assert plan(_tensor(L, packed_dtype=L.TRAIN_PACK_F32), dtype=L.BF16X3) == 0 and tiles.value == 2
    assert plan(_tensor(L, ld=96)) == 0 and tiles.value == 2     # 2 * 32 + 10 = 74 <= 96
    none = dict(packed=None, packed_dtype=L.TRAIN_PACK_NONE, ld=0, k_group=0, n_group=0)
    assert plan(_tensor(L, **none), dtype=L.F32) == 0 and tiles.value == 1
    vec = dict(kind=L.ADAM_VECTOR, K=0, N=600, ld=0, n_group=10, n_group_p=32, row_offset=64)
    assert plan(_tensor(L, **vec)) == 0 and tiles.value == 3
    assert plan(_tensor(L, **dict(vec, rule=L.TRAIN_RULE_SPARSE, constrain=0))) == 0
    bad = [
        ("null table", (None,), {}, b"null"),
        ("n = 0", (_tensor(L),), dict(n=0), b"positive"),
        ("null w", (_tensor(L, w=None),), {}, b"null"),
        ("null g", (_tensor(L, g=None),), {}, b"null"),
        ("K = 0", (_tensor(L, K=0),), {}, b"size"),
        ("N < 0", (_tensor(L, N=-3),), {}, b"size"),
        ("bad kind", (_tensor(L, kind=7),), {}, b"kind"),
        ("misaligned m", (_tensor(L, m=36),), {}, b"aligned"),
        ("bad rule", (_tensor(L, rule=2),), {}, b"rule"),
        ("bad packed_dtype", (_tensor(L, packed_dtype=3),), {}, b"packed_dtype"),
        ("NONE with a destination", (_tensor(L, packed_dtype=L.TRAIN_PACK_NONE),), {}, b"NONE"),
        ("a format without a destination", (_tensor(L, packed=None),), {}, b"NONE"),
        ("mode format in f32", (_tensor(L),), dict(dtype=L.F32), b"dtype"),
        ("mode format in fp8", (_tensor(L),), dict(dtype=L.FP8), b"dtype"),
        ("k_group = 0", (_tensor(L, k_group=0),), {}, b"k group"),
        ("k_group_p < k_group", (_tensor(L, k_group_p=8),), {}, b"k group"),
        ("K % k_group", (_tensor(L, k_group=7),), {}, b"k group"),
        ("n_group = 0", (_tensor(L, n_group=0),), {}, b"n group"),
        ("n_group_p < n_group", (_tensor(L, n_group=12, n_group_p=8),), {}, b"n group"),
        ("N % n_group", (_tensor(L, n_group=5, n_group_p=8),), {}, b"n group"),
        ("vector N % n_group", (_tensor(L, **dict(vec, n_group=7)),), {}, b"n group"),
        ("row_offset < 0", (_tensor(L, row_offset=-1),), {}, b"row_offset"),
        ("ld < last k'", (_tensor(L, ld=72),), {}, b"ld too small"),
        ("ld < 3 K_p", (_tensor(L, ld=216),), dict(dtype=L.BF16X3), b"ld too small"),
        ("ld % 3", (_tensor(L, ld=385),), dict(dtype=L.BF16X3), b"multiple of 3"),
        ("K_p % 8", (_tensor(L, ld=100),), {}, b"K_p % 8"),
        ("misaligned packed", (_tensor(L, packed=130),), {}, b"aligned"),
        ("misaligned vector packed", (_tensor(L, **dict(vec, packed=130)),), {}, b"aligned"),
    ]
    for what, args, kw, word in bad:
        assert plan(*args, **kw) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
    arr = (L.VtdTrainTensor * 1)(_tensor(L))
    assert L.lib.vtd_train_plan_bytes(arr, 1, L.BF16, None, ctypes.byref(tiles)) == -1
    assert L.lib.vtd_train_plan_bytes(arr, 1, L.BF16, ctypes.byref(nbytes), None) == -1
    assert plan(_tensor(L)) == 0
    need = nbytes.value
    for what, args, word in [
            ("null plan", (arr, 1, L.BF16, None, need, None), b"null plan_dev"),
            ("misaligned plan", (arr, 1, L.BF16, 24, need, None), b"aligned"),
            ("small plan", (arr, 1, L.BF16, 256, need - 1, None), b"plan_bytes"),
            ("bad tensor", ((L.VtdTrainTensor * 1)(_tensor(L, rule=9)), 1, L.BF16, 256, need, None),
             b"rule")]:
        assert L.lib.vtd_train_plan_upload(*args) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(L.lib.vtd_train_plan_upload(*args), "vtd_train_plan_upload")


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", None])
def test_adam_table_plans_as_its_train_form(L, mode):
    """vtd_adam_tensor is the ungrouped, always-constrained, dense-rule form of vtd_train_tensor:
    for every tensor of tests/test_gpu_adam.py SPECS, alone and all in one table, in each dtype
    that file uses (None: VTD_F32 without destinations), vtd_adam_plan_bytes and
    vtd_train_plan_bytes over the train form written out here give the same tiles and bytes.
    The pointers are never dereferenced."""
    from tests.test_gpu_adam import SPECS, up64
    dtype = {"bf16": L.BF16, "bf16x3": L.BF16X3, None: L.F32}[mode]
    pieces = {"bf16": 1, "bf16x3": 3, None: 0}[mode]
    adam, train = [], []
    for i, (shape, kp) in enumerate(SPECS):
        at = 4096 * (i + 1)
        ptrs = dict(w=at, m=at + 16, v=at + 32, g=at + 48, packed=at + 64 if mode else None)
        if len(shape) == 2:
            K, N = shape
            k_p = kp or up64(K)
            dims = dict(kind=L.ADAM_MATRIX, K=K, N=N, ld=pieces * k_p)
        else:
            K, N, k_p = 0, shape[0], 0
            dims = dict(kind=L.ADAM_VECTOR, K=0, N=N, ld=0)
        adam.append(L.VtdAdamTensor(**ptrs, **dims))
        train.append(L.VtdTrainTensor(
            **ptrs, **dims, k_group=K, k_group_p=k_p if mode else 0, n_group=N, n_group_p=N,
            row_offset=0, packed_dtype=L.TRAIN_PACK_MODE if mode else L.TRAIN_PACK_NONE,
            constrain=1, rule=L.TRAIN_RULE_DENSE))

    def plans(which):
        out = []
        for entry, kind, table in ((L.lib.vtd_adam_plan_bytes, L.VtdAdamTensor, adam),
                                   (L.lib.vtd_train_plan_bytes, L.VtdTrainTensor, train)):
            nbytes, tiles = ctypes.c_size_t(), ctypes.c_int()
            arr = (kind * len(which))(*[table[i] for i in which])
            assert entry(arr, len(which), dtype, ctypes.byref(nbytes), ctypes.byref(tiles)) == 0, \
                L.lib.vtd_last_error()
            out.append((tiles.value, nbytes.value))
        return out

    for which in [[i] for i in range(len(SPECS))] + [list(range(len(SPECS)))]:
        a, t = plans(which)
        assert a == t and a[0] > 0 and a[1] > 0, (which, a, t)
    # 130 x 6 with K_p = 256: four K tiles with a destination (one is pure padding), else three
    assert plans([2])[0][0] == (4 if mode else 3)


def test_train_step_argument_checks_need_no_device(L):
    ok = dict(plan=256, n=1, tiles=2, t=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, clip=10.0,
              constrain=1, max_weight=10.0)

    def step(**kw):
        a = dict(ok, **kw)
        return L.lib.vtd_train_step(a["plan"], a["n"], a["tiles"], a["t"], a["lr"], a["b1"],
                                    a["b2"], a["eps"], a["clip"], a["constrain"],
                                    a["max_weight"], None)

    for what, kw, word in [("null plan", dict(plan=None), b"null"),
                           ("n = 0", dict(n=0), b"non-positive"),
                           ("tiles = 0", dict(tiles=0), b"non-positive"),
                           ("t = 0", dict(t=0), b"starts at 1"),
                           ("max_weight 0", dict(max_weight=0.0), b"max_weight"),
                           ("max_weight nan", dict(max_weight=float("nan")), b"max_weight")]:
        assert step(**kw) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(step(**kw), "vtd_train_step")


def _job(L, **kw):
    base = dict(w32=64, gamma=128, beta=192, bias_in=256, w_out=320, bias_out=384, colsum=448,
                N=64, K=64, ldw=64, ldo=64)
    base.update(kw)
    return L.VtdFoldJob(**base)


def test_fold_batch_argument_checks_need_no_device(L):
    rows = ctypes.c_int()

    def upload(job, n=1, dtype=L.BF16, dev=512, nbytes=72, rows_out=True):
        arr = (L.VtdFoldJob * 1)(job) if job is not None else None
        return L.lib.vtd_fold_plan_upload(arr, n, dtype, dev, nbytes,
                                          ctypes.byref(rows) if rows_out else None, None)

    for what, kw, word in [
            ("null table", dict(job=None), b"null"),
            ("null max_rows", dict(job=_job(L), rows_out=False), b"null"),
            ("n = 0", dict(job=_job(L), n=0), b"n_jobs"),
            ("split-bf16", dict(job=_job(L), dtype=L.BF16X3), b"dtype"),
            ("fp8", dict(job=_job(L), dtype=L.FP8), b"dtype"),
            ("null w32", dict(job=_job(L, w32=None)), b"null pointer"),
            ("null gamma", dict(job=_job(L, gamma=None)), b"null pointer"),
            ("null colsum", dict(job=_job(L, colsum=None)), b"null pointer"),
            ("N = 0", dict(job=_job(L, N=0)), b"shape"),
            ("ldw < K", dict(job=_job(L, ldw=32)), b"shape"),
            ("ldo < K", dict(job=_job(L, ldo=8)), b"shape"),
            ("null plan", dict(job=_job(L), dev=None), b"null plan_dev"),
            ("misaligned plan", dict(job=_job(L), dev=520), b"aligned"),
            ("small plan", dict(job=_job(L), nbytes=71), b"plan_bytes")]:
        assert upload(**kw) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
    for what, args, word in [("null plan", (None, 1, 64, L.BF16, None), b"null"),
                             ("n = 0", (512, 0, 64, L.BF16, None), b"non-positive"),
                             ("rows = 0", (512, 1, 0, L.BF16, None), b"non-positive"),
                             ("dtype", (512, 1, 64, L.BF16X3, None), b"dtype")]:
        assert L.lib.vtd_fold_layernorm_batch(*args) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
