"""tests/ln_designs.py on the CPU: the generator's own claims, the route table, and the power of
the designed-row suite (tests/test_gpu_layernorm_designed.py) to notice a wrong kernel.

A numpy emulation of the kernels' arithmetic (ln_designs.emulate: the lane layouts, the
butterfly, the masks, fp32 throughout) passes every case of the GPU tables under the same checks
the device output meets, and fails them for each seeded defect.

Why the suite is needed: test_gpu_kernels.test_layernorm holds f32 output to
1e-5 max(1, |y|.max()) on N(1, 3) rows.  At D = 4096 a column left out of the row sum moves the
mean by x[c] / 4096 and every y by about x[c] / 12288, under that tolerance whenever
|x[c]| < ~0.5: test_present_tolerance_misses_a_dropped_column counts those (row, column) pairs
on that test's own data (about one in eight).  On an order-free row the same defect makes the mean
inexact, and the mean must be bit-exact.
"""
import numpy as np
import pytest

from tests import ln_designs as LD

XDT_ROWS = [(t, r) for t in ("f32", "bf16") for r in (1, 11)]
ISSUE_D = (1, 4, 28, 30, 63, 256, 260, 768, 1040, 2048, 3072, 4096, 4100)


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
def test_order_free_rows_are_order_free(xdt):
    """sum(k) == 0, no zero k, the 2^24 rules, bf16 numbers; then mean == m bit for bit and one
    value of q in every lane layout and in plain forward / reverse / pairwise fp32 sums."""
    for D in ISSUE_D:
        c = LD.Case(xdt, len(LD.ORDER_FREE[xdt]), D, ldx=-(-D // 16) * 16 + 16,
                    kinds=[("of", i) for i in range(len(LD.ORDER_FREE[xdt]))])
        for r, (m, h) in enumerate(LD.ORDER_FREE[xdt]):
            k = c.k[r]
            assert k.sum() == 0 and (D == 1 or np.abs(k).min() >= 1)
            assert np.abs(k).max() <= LD.k_cap(D) <= 64
            LD.check_order_free(k, m, h, xdt == "bf16")
            x = c.x[r]
            q64 = float((h * k.astype(np.float64)) ** 2 @ np.ones(D))
            for order in (x, x[::-1], np.sort(x)):
                s = np.float32(0)
                for v in order:
                    s = np.float32(s + v)
                assert np.float32(s / np.float32(D)) == np.float32(m)
                d = order - np.float32(m)
                q = np.float32(0)
                for v in d:
                    q = np.float32(q + v * v)
                assert float(q) == q64
            assert np.float32(x.sum(dtype=np.float32) / np.float32(D)) == np.float32(m)
        layouts = [("layernorm_generic_kernel", 0)]
        if D % 4 == 0 and D <= 4096:
            layouts.append(("layernorm_kernel", 16))
        if D % 8 == 0 and D <= 2048:
            layouts.append(("ln_stats_kernel", 4))
        if D % 16 == 0 and D <= 4096:
            layouts.append(("layernorm16_kernel", 4))
        stats = [LD.emulate(c, *lay)[:2] for lay in layouts]
        mean64, rstd64, _, _ = c.ref64()
        for mean, rstd in stats:
            assert np.array_equal(mean, c.exact_mean)
            assert np.array_equal(rstd, stats[0][1])          # the same bits in every layout
            assert (np.abs(rstd - rstd64) <= LD.U22 * rstd64).all()


def test_generator_refuses_rows_that_are_not_exact():
    k = np.array([3, -2, -1, 5, -5])
    LD.check_order_free(k, 16.0, 0.125)
    with pytest.raises(AssertionError, match="sum"):
        LD.check_order_free(np.array([3, -2, 1]), 0.0, 0.125)
    with pytest.raises(AssertionError, match="zero k"):
        LD.check_order_free(np.array([3, -3, 0]), 0.0, 0.125)
    with pytest.raises(AssertionError, match="2\\^24"):
        LD.check_order_free(np.resize([64, -64], 4100), 0.0, 0.125)
    with pytest.raises(AssertionError, match="2\\^24"):
        LD.check_order_free(np.resize([1, -1], 4096), 1024.0, 0.125)
    with pytest.raises(AssertionError, match="bf16"):
        LD.check_order_free(np.array([1, -1]), 256.0, 0.125, bf16=True)
    with pytest.raises(AssertionError, match="power of two"):
        LD.check_order_free(k, 0.0, 0.3)
    assert LD.k_cap(4096) == 64 and LD.k_cap(4100) == 63


def test_gamma_beta_and_memory_image():
    c = LD.Case("bf16", 11, 264, x_off=4, g_off=1)
    assert len(set(c.gamma)) > 4 and len(set(c.beta)) > 4
    assert np.array_equal(c.gamma * 16, np.round(c.gamma * 16)) and c.gamma.min() >= 0.5
    assert np.array_equal(c.beta * 8, np.round(c.beta * 8)) and np.abs(c.beta).max() <= 1
    xr = c.x_rows()
    assert np.array_equal(xr[:, :264], c.x.astype(np.float64)) and np.isnan(xr[:, 264:]).all()
    assert np.isnan(LD.bf16_value(c.x_body().ravel()[:4])).all()
    g = c.vec_body(c.gamma)
    assert np.isnan(g[0]) and len(g) == 265
    kinds = [k for k, _ in c.kinds]
    assert {"of", "const", "gen", "hi"} <= set(kinds)
    assert len({tuple(r) for r in c.x}) == 11               # no two rows alike


# ------------------------------------------------------------------ the route table
def test_routes_of_the_tables_and_coverage():
    want_nv = {"f32": dict(zip(LD.LN_D["f32"]["vec"], (1, 1, 2, 2, 3, 3, 4, 4, 8, 8, 16, 16))),
               "bf16": dict(zip(LD.LN_D["bf16"]["vec"], (1, 2, 3, 4, 8, 16)))}
    want_nc = dict(zip(LD.LN_D["bf16"]["ln16"], (1, 1, 2, 2, 4, 4, 4)))
    want_stats = {8: 1, 512: 1, 520: 2, 1024: 2, 1032: 4, 2048: 4}
    want_mis = {("f32", 256, 2, 0): ("layernorm_generic_kernel", 0),
                ("f32", 256, 0, 1): ("layernorm_generic_kernel", 0),
                ("bf16", 1024, 4, 0): ("layernorm_kernel", 4),
                ("bf16", 4096, 4, 0): ("layernorm_kernel", 16),
                ("bf16", 768, 4, 0): ("layernorm_kernel", 3),
                ("bf16", 512, 0, 0): ("layernorm_kernel", 2),
                ("bf16", 256, 1, 0): ("layernorm_generic_kernel", 0),
                ("bf16", 256, 0, 1): ("layernorm_generic_kernel", 0)}
    reached = set()
    per_input = set()
    for xdt, rows in XDT_ROWS:
        for c in LD.ln_cases(xdt, rows):
            aligned = not (c.x_off or c.g_off or (c.D, c.ldx) == (512, 524))
            pads = set()
            for call in LD.calls(c):
                k, n = call["route"]
                reached.add((k, n))
                per_input.add((xdt, k, n))
                if call["entry"] == "layernorm":
                    pads.add(call["P"] - c.D)
                    assert call["P"] != c.ldx                # ldx != ldy
                    if not aligned:
                        assert (k, n) == want_mis[(xdt, c.D, c.x_off, c.g_off)], (c, k, n)
                    elif c.D in LD.LN_D[xdt]["generic"]:
                        assert k == "layernorm_generic_kernel"
                    elif c.D in want_nv[xdt]:
                        assert (k, n) == ("layernorm_kernel", want_nv[xdt][c.D]), (c, k, n)
                    elif xdt == "bf16" and c.D in want_nc:
                        assert (k, n) == ("layernorm16_kernel", want_nc[c.D]), (c, k, n)
                elif call["entry"] == "layernorm_stats" and aligned:
                    if c.D in want_stats:
                        assert (k, n) == ("ln_stats_kernel", want_stats[c.D]), (c, k, n)
                    elif c.D in (30, 2056, 4096):
                        assert k == "ln_stats_generic_kernel"
                elif call["entry"] == "layernorm_mx8" and aligned:
                    for name, ds in LD.MX_D.items():
                        if c.D in ds:
                            assert k == name, (c, k)
            assert pads == {0, 4, 100}
            if xdt == "f32" and c.x_off == 2:
                assert c.route("layernorm_stats")[0] == "ln_stats_generic_kernel"
    for c in LD.mx_const_cases():
        k, n = c.route("layernorm_mx8", Kq=LD.mx_kq(c))
        reached.add((k, n))
        per_input.add((c.xdt, k, n))
    for s, _, _ in LD.FIN_UNROLLED:
        reached.add(LD.route("layernorm_stats_finalize", slots=s))
    for s, _ in LD.FIN_GENERIC:
        reached.add(LD.route("layernorm_stats_finalize", slots=s))
    missing = [i for i in LD.INSTANTIATIONS if i not in reached]
    assert not missing, missing
    # both fused kernels with both input dtypes at every NC / NV; the 4-column LayerNorm with
    # bf16 input beyond NV 1; the statistics kernels with both inputs
    for xdt in ("f32", "bf16"):
        for k, ns in (("layernorm16_mx8_kernel", (1, 2, 4)), ("layernorm_mx8_kernel", (2, 4, 8, 16)),
                      ("ln_stats_kernel", (1, 2, 4)), ("layernorm_kernel", (1, 2, 3, 4, 8, 16))):
            for n in ns:
                assert (xdt, k, n) in per_input, (xdt, k, n)
    # the fused and the plain dispatcher agree on the lane layout for bf16 input only
    assert LD.route("layernorm", "f32", 1024, 1032, P=1024)[0] == "layernorm_kernel"
    assert LD.route("layernorm_mx8", "f32", 1024, 1032, Kq=1024)[0] == "layernorm16_mx8_kernel"
    assert LD.route("layernorm", "bf16", 1024, 1032, P=1024, out="bf16")[0] == "layernorm16_kernel"
    assert LD.route("layernorm_mx8", "bf16", 1024, 1032, Kq=1024)[0] == "layernorm16_mx8_kernel"


# ------------------------------------------------------------------ the emulation under the checks
def run_checks(c, fault=None, reps=None):
    """Every check the device output of case c meets, on the emulation's output instead."""
    reps = {} if reps is None else reps
    f32_out = None
    for call in LD.calls(c):
        k, n = call["route"]
        rep = reps.setdefault(call["entry"], LD.Report())
        if call["entry"] == "layernorm_stats":
            mean, rstd, _ = LD.emulate(c, k, n, fault=fault)
            LD.check_stats(c, np.stack([mean, rstd], axis=1), rep, kernel=(k, n))
        elif call["entry"] == "layernorm":
            _, _, y = LD.emulate(c, k, n, fault=fault)
            if call["out"] == "f32":
                f32_out = y
                LD.check_y(c, "f32", y, rep, kernel=(k, n))
            elif call["out"] == "bf16":
                LD.check_y(c, "bf16", LD.bf16_bits(y), rep, kernel=(k, n))
            else:
                assert np.array_equal(LD.split_expected(y, call["P"]),
                                      LD.split_expected(f32_out, call["P"]))
        else:
            _, _, y = LD.emulate(c, k, n, fault=fault)
            q, s = LD.emulate_mx(y, call["Kq"], fault)
            _, _, yu = LD.emulate(c, *c.route("layernorm", P=c.D, out="bf16"))
            qu, su = LD.mx_expected(LD.bf16_value(LD.bf16_bits(yu)), call["Kq"])
            keep = c.designed
            assert np.array_equal(q[keep], qu[keep]) and np.array_equal(s[keep], su[keep]), \
                "fused != unfused on designed rows"
    return reps


@pytest.mark.parametrize("xdt,rows", XDT_ROWS)
def test_emulation_passes_every_case(xdt, rows):
    reps = {}
    for c in LD.ln_cases(xdt, rows):
        run_checks(c, reps=reps)
    for entry, rep in reps.items():
        print(f"{xdt} rows {rows} {entry}: {rep}")
        assert rep.designed <= 1
    if rows == 11:
        assert reps["layernorm"].general > 0 and reps["layernorm_stats"].rstd_total > 0


def mx_const_check(c, fault=None):
    Kq = LD.mx_kq(c)
    k, n = c.route("layernorm_mx8", Kq=Kq)
    _, _, y = LD.emulate(c, k, n, fault=fault)
    q, s = LD.emulate_mx(y, Kq, fault)
    want_q, want_s = LD.mx_expected(np.broadcast_to(c.beta, (c.rows, c.D)), Kq)
    assert np.array_equal(s, want_s), "scale bytes differ"
    assert np.array_equal(q, want_q), "e4m3 bytes differ"
    return want_q, want_s


def test_mx_constant_rows_design():
    seen = set()
    for c in LD.mx_const_cases():
        q, s = mx_const_check(c)
        seen |= set(s.ravel().tolist())
        nb = -(-c.D // 32)
        assert (q[:, c.D:] == 0).all() and (s[:, nb:] == 1).all()
        beta = c.beta.astype(np.float64)
        for j in range(c.D // 32):
            blk = np.abs(beta[32 * j:32 * j + 32])
            assert blk.argmax() == j % 32 and (np.delete(blk, j % 32) < blk.max()).all() \
                or blk.max() == 0
        if c.D >= 1024:
            am = np.abs(np.resize(beta, (c.D // 32, 32))).max(axis=1)
            assert 7.0 in am and 7.03125 in am and 0.0 in am and 256.0 in am
            sub = np.abs(LD.MX.decode_e4m3(q[0, :c.D]))
            assert ((sub > 0) & (sub < 2.0 ** -6)).any()   # e4m3 subnormals are produced
    assert 1 in seen and len(seen) > 8


FAULT_CASES = [("f32", 4096), ("f32", 772), ("f32", 30), ("bf16", 3072), ("bf16", 776)]


@pytest.mark.parametrize("fault", LD.FAULTS)
def test_every_seeded_fault_is_caught(fault):
    caught = 0
    if fault == "amax_over_16":
        for c in LD.mx_const_cases():
            if c.rows == 11 and c.D in (1024, 3072, 4096):   # a maximum in the upper 16 columns
                with pytest.raises(AssertionError):
                    mx_const_check(c, fault)
                caught += 1
        assert caught >= 4
        return
    for xdt, D in FAULT_CASES:
        c = LD.Case(xdt, 11, D)
        run_checks(c)
        try:
            run_checks(c, fault)
        except AssertionError:
            caught += 1
    # a pad column can be read only where the instantiation's span exceeds D (not at D = 4096)
    assert caught == len(FAULT_CASES) - (fault == "pad_column_read")


def test_present_tolerance_misses_a_dropped_column():
    """test_gpu_kernels.test_layernorm's data and tolerance at D = 4096 (f32 in, f32 out): a
    float64 LayerNorm that leaves column c out of one row's sum passes whenever x[r, c] is
    small."""
    torch = pytest.importorskip("torch")
    D, rows = 4096, 37
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(rows, D, generator=g) * 3 + 1).double().numpy()
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).double().numpy()
    beta = (0.1 * torch.randn(D, generator=g)).double().numpy()

    def ln(mean):
        d = x - mean[:, None]
        return d / np.sqrt((d * d).mean(axis=1) + 1e-3)[:, None] * gamma + beta

    exp = ln(x.mean(axis=1))
    tol = 1e-5 * max(1, np.abs(exp).max())
    cols = range(0, D, 16)
    passed = sum(int((np.abs(ln((x.sum(axis=1) - x[:, c]) / D) - exp).max(axis=1) < tol).sum())
                 for c in cols)
    print(f"{passed} of {rows * len(cols)} (row, dropped column) pairs pass the present "
          f"tolerance {tol:.3g}")
    assert passed > rows * len(cols) // 20
    # the designed rows notice the same defect in every column: the mean stops being exact
    c = LD.Case("f32", 11, D)
    with pytest.raises(AssertionError, match="must be exact"):
        mean, rstd, _ = LD.emulate(c, "ln_stats_generic_kernel", 0, fault="column_dropped")
        LD.check_stats(c, np.stack([mean, rstd], axis=1))


# ------------------------------------------------------------------ finalize and fold designs
def test_finalize_partials_design():
    rep = LD.Report()
    for s, r, _ in LD.FIN_UNROLLED:
        p = LD.Partials(r, s)
        p.check(p.np32(), rep)
    for s, r in LD.FIN_GENERIC:
        p = LD.Partials(r, s, seed=1)
        p.check(p.np32(), rep)
    assert rep.designed <= 1
    g = LD.Partials(300, 12, general=True)
    g.check(g.np32(), rep)
    # a merge that forgets the between-block term is caught
    p = LD.Partials(300, 16)
    bad = p.np32()
    m2 = p.m2.sum(axis=0)
    bad[:, 1] = np.float32(1) / np.sqrt(m2 / np.float32(p.D) + np.float32(LD.EPS))
    with pytest.raises(AssertionError):
        p.check(bad)


def test_fold_design_is_exact():
    for N, K, ldw, ldo in LD.FOLD_SHAPES:
        f = LD.Fold(N, K, ldw, ldo)
        for with_bias in (False, True):
            for bf16 in (False, True):
                w_out, bias, colsum = f.expected(with_bias, bf16)
                assert w_out.shape == (N, ldo) and (w_out[:, K:] == 0).all()
                assert np.array_equal(colsum.astype(np.float64), w_out.astype(np.float64).sum(1))
        assert len(np.unique(f.gamma)) > 1 or K == 1
