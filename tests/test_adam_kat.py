"""Known answers for the Adam step's yardstick (tests/adam_oracle.py step32 / step64), the step
schedule, and the host side of the feature without a GPU: optimizers.Adam's argument checks and
every VTD_ERR_INVALID_ARG case of vtd_adam_plan_bytes / vtd_adam_plan_upload / vtd_adam_step,
which must answer before any device call (the pointers here are never dereferenced)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import adam_oracle as A

B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))      # the fp32 betas, as doubles
EPS = float(np.float32(1e-7))
U = 2.0 ** -24                                                 # fp32 unit roundoff


def zeros(x):
    return np.zeros_like(x)


# ------------------------------------------------------------------ known answers
def test_first_step_closed_form():
    """m1 = g (1 - b1), v1 = g^2 (1 - b2), alpha = lr sqrt(1 - b2) / (1 - b1), so
    dw = -lr g sqrt(1 - b2) / (sqrt(1 - b2) |g| + eps); with eps = 0 it is -lr sign(g)."""
    g = np.array([3.0, -0.25, 1e-2, -40.0, 7e2])
    w = np.array([0.5, -1.0, 2.0, 0.0, -3.0])
    lr = 1e-3
    w1, _, _ = A.step64(w, zeros(w), zeros(w), g, 1, lr, constrain=False)
    s = math.sqrt(1.0 - B2)
    np.testing.assert_allclose(w1 - w, -lr * g * s / (s * np.abs(g) + EPS), rtol=1e-12)
    w0, _, _ = A.step64(w, zeros(w), zeros(w), g, 1, lr, epsilon=0.0, constrain=False)
    np.testing.assert_allclose(w0 - w, -lr * np.sign(g), rtol=1e-12)
    w32, _, _ = A.step32(w, zeros(w), zeros(w), g, 1, lr, epsilon=0.0, constrain=False)
    assert w32.dtype == np.float32
    np.testing.assert_allclose(w32 - w.astype(np.float32), -lr * np.sign(g), rtol=1e-3)


def test_constant_gradient_closed_forms():
    g = np.array([2.0, -0.5, 1e-3])
    w, m, v = np.zeros(3), np.zeros(3), np.zeros(3)
    for t in range(1, 51):
        w, m, v = A.step64(w, m, v, g, t, 1e-3, constrain=False)
        np.testing.assert_allclose(m, g * (1.0 - B1 ** t), rtol=1e-12)
        np.testing.assert_allclose(v, g * g * (1.0 - B2 ** t), rtol=1e-12)


@pytest.mark.parametrize("step", [A.step32, A.step64])
def test_clipvalue(step):
    w = np.array([0.1, -0.2], np.float32)
    big, ten = np.array([1e3, -1e3], np.float32), np.array([10.0, -10.0], np.float32)
    a = step(w, zeros(w), zeros(w), big, 1, 1e-3, clipvalue=10)
    b = step(w, zeros(w), zeros(w), ten, 1, 1e-3, clipvalue=10)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # clipvalue=None leaves g alone: m1 = g (1 - b1)
    _, m, _ = step(w, zeros(w), zeros(w), big, 1, 1e-3, clipvalue=None)
    np.testing.assert_allclose(m, big.astype(np.float64) * (1.0 - B1), rtol=1e-6)
    _, m, _ = step(w, zeros(w), zeros(w), big, 1, 1e-3, clipvalue=10)
    np.testing.assert_allclose(m, ten.astype(np.float64) * (1.0 - B1), rtol=1e-6)


@pytest.mark.parametrize("step", [A.step32, A.step64])
def test_nan_gradient_sets_the_weight_to_one_for_good(step):
    """ClipWeight maps NaN to 1.0 (vtd.py:209-236); m and v stay NaN, so every later step does
    the same.  The reference's behaviour, restated."""
    w = np.array([0.3, -0.7], np.float32)
    g = np.array([np.nan, 0.5], np.float32)
    w1, m1, v1 = step(w, zeros(w), zeros(w), g, 1, 1e-3, clipvalue=10)
    assert w1[0] == 1.0 and np.isnan(m1[0]) and np.isnan(v1[0])
    assert np.isfinite(w1[1]) and w1[1] < w[1]
    w2, m2, v2 = step(w1, m1, v1, np.array([0.1, 0.1], np.float32), 2, 1e-3, clipvalue=10)
    assert w2[0] == 1.0 and np.isnan(m2[0]) and np.isnan(v2[0])
    # without the constraint the NaN reaches the weight
    w3, _, _ = step(w, zeros(w), zeros(w), g, 1, 1e-3, clipvalue=10, constrain=False)
    assert np.isnan(w3[0])


@pytest.mark.parametrize("step", [A.step32, A.step64])
def test_max_weight_clips_exactly(step):
    w = np.array([9.9995, -9.9995, 3.0], np.float32)
    g = np.array([-1.0, 1.0, 1.0], np.float32)            # pushes |w| up by lr = 1e-3
    w1, _, _ = step(w, zeros(w), zeros(w), g, 1, 1e-3, max_weight=10, constrain=True)
    np.testing.assert_array_equal(w1[:2], np.array([10.0, -10.0], w1.dtype))
    assert abs(float(w1[2]) - (3.0 - 1e-3)) < 1e-6
    free, _, _ = step(w, zeros(w), zeros(w), g, 1, 1e-3, max_weight=10, constrain=False)
    assert free[0] > 10.0 and free[1] < -10.0


# ------------------------------------------------------------------ step32 against step64
def test_step32_tracks_step64_within_the_rounding_bound():
    """20 steps, N(0, 1) weights, gradient magnitudes 1e-9 .. 1e3.  Each element's gradient
    keeps its sign and varies by a factor in [0.5, 1.5], so m and v are convex combinations of
    same-signed terms and every bound below is a first-order rounding count, u = 2^-24:

      m' = m + (g - m) c: three roundings (sub, mul, add).  Both c |g - m| and (1 - c) |m| are
        <= |m'| for same-signed g, m, so each adds at most u |m'| and the carried error shrinks
        by (1 - c) m / m' <= 1; c = 1 - b1 is exact in fp32 for b1 in [0.5, 1] (Sterbenz) and
        both runs use the fp32 betas.  After t steps: |m32 - m64| <= 3 t u |m64|.
      v' = v + (g g - v) c: one more rounding for g g: 4 t u |v64|.
      d = (m alpha) / (sqrt(v) + eps): m (3 t u), alpha (u, rounded to fp32 once), the product
        (u), sqrt(v) (half of v's: 2 t u, plus its own u), the sum with eps (u), the quotient
        (u): |d32 - d64| <= (5 t + 5) u |d64|.
      w' = w - d: one rounding, u |w'|: half an ulp of w.
    The w bound is the sum of these over the steps, with |d64| and |w64| taken from the
    float64 run (|d| is a few lr, so per step this is some tens of lr 2^-23 plus half an ulp
    of w).  A factor 1.01 covers the second-order terms."""
    rng = np.random.default_rng(5)
    n, steps, lr = 4096, 20, 1e-3
    w0 = rng.standard_normal(n).astype(np.float32)
    mag = (10.0 ** rng.uniform(-9, 3, n)) * rng.choice([-1.0, 1.0], n)
    w32, m32, v32 = w0, zeros(w0), zeros(w0)
    w64, m64, v64 = w0.astype(np.float64), np.zeros(n), np.zeros(n)
    w_bound = np.zeros(n)
    worst = dict(m=0.0, v=0.0, w=0.0)
    for t in range(1, steps + 1):
        g = (mag * rng.uniform(0.5, 1.5, n)).astype(np.float32)
        before = w64
        w32, m32, v32 = A.step32(w32, m32, v32, g, t, lr)
        w64, m64, v64 = A.step64(w64, m64, v64, g, t, lr)
        d64 = np.abs(w64 - before)
        w_bound = w_bound + 1.01 * U * ((5 * t + 5) * d64 + np.abs(w64))
        em = np.abs(m32 - m64) / np.abs(m64)
        ev = np.abs(v32 - v64) / np.abs(v64)
        worst["m"] = max(worst["m"], float((em / (3 * t * U)).max()))
        worst["v"] = max(worst["v"], float((ev / (4 * t * U)).max()))
        worst["w"] = max(worst["w"], float((np.abs(w32 - w64) / w_bound).max()))
        assert np.all(em <= 1.01 * 3 * t * U), (t, em.max())
        assert np.all(ev <= 1.01 * 4 * t * U), (t, ev.max())
        assert np.all(np.abs(w32 - w64) <= w_bound), t
    print("fractions of the bounds used:", worst)
    assert np.abs(w32 - w0).max() > 10 * lr          # the weights moved: the test saw updates


# ------------------------------------------------------------------ the step schedule
@pytest.fixture(scope="module")
def vtd():
    import vision_transformer_detector_amd as m
    return m


def test_learning_rate_step_decay_follows_the_notebook(vtd):
    """The notebook's 1000 / 9000 / 1000 x 0.1 schedule from 8e-5."""
    sched = functools.partial(vtd.learning_rate_step_decay, epochs_first_lr_decay=1000,
                              epochs_second_lr_decay=9000, epochs_third_lr_decay=1000,
                              rate_lr_decay=0.1)
    vtd._allowed_decay_times.assign(3)
    lr, changes = 8e-5, {}
    for epoch in range(12502):
        new = sched(epoch, lr)
        if new != lr:
            changes[epoch] = new
        lr = new
    assert list(changes) == [1000, 10000, 11000]
    np.testing.assert_allclose(list(changes.values()), [8e-6, 8e-7, 8e-8], rtol=1e-12)
    assert int(vtd._allowed_decay_times.numpy()) == 0
    # the counter is spent: the same epochs decay nothing now
    assert sched(1000, 8e-5) == 8e-5 and sched(10000, 8e-5) == 8e-5
    # and with two decays allowed the third is skipped
    vtd._allowed_decay_times.assign(2)
    assert sched(1000, 1.0) == 0.1 and sched(10000, 1.0) == 0.1 and sched(11000, 1.0) == 1.0
    assert sched(999, 1.0) == 1.0
    vtd._allowed_decay_times.assign(3)


# ------------------------------------------------------------------ host checks, no device
def test_adam_arguments(vtd):
    opt = vtd.optimizers.Adam()
    assert (opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon, opt.clipvalue,
            opt.iterations) == (1e-3, 0.9, 0.999, 1e-7, None, 0)
    opt = vtd.optimizers.Adam(learning_rate=8e-5, clipvalue=10)
    assert opt.learning_rate == 8e-5 and opt.clipvalue == 10.0
    opt.learning_rate = 1e-5
    assert opt.learning_rate == 1e-5 and opt.lr == 1e-5
    for kw in (dict(amsgrad=True), dict(clipnorm=1.0), dict(global_clipnorm=1.0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            vtd.optimizers.Adam(**kw)
    with pytest.raises(ValueError, match="clipvalue"):
        vtd.optimizers.Adam(clipvalue=-1)
    with pytest.raises(ValueError, match="no optimizer"):
        vtd.optimizers.resolve(None)
    with pytest.raises(ValueError, match="unsupported optimizer"):
        vtd.optimizers.resolve("sgd")
    assert isinstance(vtd.optimizers.resolve("adam"), vtd.optimizers.Adam)


@pytest.fixture(scope="module")
def L():
    from vision_transformer_detector_amd import _lib
    return _lib


def _tensor(L, **kw):
    base = dict(w=16, m=32, v=48, g=64, packed=128, kind=L.ADAM_MATRIX, K=70, N=17, ld=128)
    base.update(kw)
    return L.VtdAdamTensor(**base)


def test_adam_abi_is_declared_and_the_version_stays(L):
    for name in ("vtd_adam_plan_bytes", "vtd_adam_plan_upload", "vtd_adam_step"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert L.lib.vtd_abi_version() == 17


def test_adam_plan_argument_checks_need_no_device(L):
    nbytes, tiles = ctypes.c_size_t(), ctypes.c_int()

    def plan(t, n=1, dtype=L.BF16):
        arr = (L.VtdAdamTensor * 1)(t) if t is not None else None
        return L.lib.vtd_adam_plan_bytes(arr, n, dtype, ctypes.byref(nbytes), ctypes.byref(tiles))

    assert plan(_tensor(L)) == 0
    # 70 x 17 with K_p = 128: two K tiles of 64, one N tile
    assert tiles.value == 2 and nbytes.value > 0
    assert plan(_tensor(L, ld=384), dtype=L.BF16X3) == 0 and tiles.value == 2
    assert plan(_tensor(L, packed=None, ld=0), dtype=L.F32) == 0 and tiles.value == 2
    assert plan(_tensor(L, kind=L.ADAM_VECTOR, K=0, N=300, ld=0)) == 0 and tiles.value == 2
    bad = [
        ("null table", (None,), {}, b"null"),
        ("n = 0", (_tensor(L),), dict(n=0), b"positive"),
        ("null w", (_tensor(L, w=None),), {}, b"null"),
        ("null m", (_tensor(L, m=None),), {}, b"null"),
        ("null v", (_tensor(L, v=None),), {}, b"null"),
        ("null g", (_tensor(L, g=None),), {}, b"null"),
        ("K = 0", (_tensor(L, K=0),), {}, b"size"),
        ("N < 0", (_tensor(L, N=-3),), {}, b"size"),
        ("vector N = 0", (_tensor(L, kind=L.ADAM_VECTOR, N=0),), {}, b"size"),
        ("bad kind", (_tensor(L, kind=7),), {}, b"kind"),
        ("misaligned w", (_tensor(L, w=20),), {}, b"aligned"),
        ("ld < K", (_tensor(L, ld=64),), {}, b"ld too small"),
        ("ld < 3 K", (_tensor(L, ld=192),), dict(dtype=L.BF16X3), b"ld too small"),
        ("ld % 3", (_tensor(L, ld=385),), dict(dtype=L.BF16X3), b"multiple of 3"),
        ("K_p % 8", (_tensor(L, ld=100),), {}, b"K_p % 8"),
        ("misaligned packed", (_tensor(L, packed=130),), {}, b"aligned"),
        ("f32 packed", (_tensor(L),), dict(dtype=L.F32), b"dtype"),
        ("fp8 packed", (_tensor(L),), dict(dtype=L.FP8), b"dtype"),
        ("f32 packed vector", (_tensor(L, kind=L.ADAM_VECTOR),), dict(dtype=L.F32), b"dtype"),
    ]
    for what, args, kw, word in bad:
        assert plan(*args, **kw) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
    arr = (L.VtdAdamTensor * 1)(_tensor(L))
    assert L.lib.vtd_adam_plan_bytes(arr, 1, L.BF16, None, ctypes.byref(tiles)) == -1
    assert L.lib.vtd_adam_plan_bytes(arr, 1, L.BF16, ctypes.byref(nbytes), None) == -1
    assert plan(_tensor(L)) == 0
    need = nbytes.value
    for what, args, word in [
            ("null plan", (arr, 1, L.BF16, None, need, None), b"null plan_dev"),
            ("misaligned plan", (arr, 1, L.BF16, 24, need, None), b"aligned"),
            ("small plan", (arr, 1, L.BF16, 256, need - 1, None), b"plan_bytes"),
            ("bad tensor", ((L.VtdAdamTensor * 1)(_tensor(L, g=None)), 1, L.BF16, 256, need, None),
             b"null")]:
        assert L.lib.vtd_adam_plan_upload(*args) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(L.lib.vtd_adam_plan_upload(*args), "vtd_adam_plan_upload")


def test_adam_step_argument_checks_need_no_device(L):
    ok = dict(plan=256, n=1, tiles=2, t=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, clip=10.0,
              constrain=1, max_weight=10.0)

    def step(**kw):
        a = dict(ok, **kw)
        return L.lib.vtd_adam_step(a["plan"], a["n"], a["tiles"], a["t"], a["lr"], a["b1"],
                                   a["b2"], a["eps"], a["clip"], a["constrain"],
                                   a["max_weight"], None)

    for what, kw, word in [("null plan", dict(plan=None), b"null"),
                           ("n = 0", dict(n=0), b"non-positive"),
                           ("tiles = 0", dict(tiles=0), b"non-positive"),
                           ("tiles < 0", dict(tiles=-4), b"non-positive"),
                           ("t = 0", dict(t=0), b"starts at 1"),
                           ("t < 0", dict(t=-2), b"starts at 1"),
                           ("max_weight 0", dict(max_weight=0.0), b"max_weight"),
                           ("max_weight nan", dict(max_weight=float("nan")), b"max_weight")]:
        assert step(**kw) == -1, what
        assert word in L.lib.vtd_last_error(), (what, L.lib.vtd_last_error())
        with pytest.raises(ValueError):
            L.check(step(**kw), "vtd_adam_step")
