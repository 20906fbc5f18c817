"""vtd_train_step and vtd_fold_layernorm_batch on the GPU, direct calls on designed tables.

Every tensor's w, m, v equal tests/adam_oracle.py step32 (tests/train_oracle.py sparse32 for the
sparse-order rule) bit for bit over three chained steps, and its destination equals, as a whole
buffer, (a) the numpy restatement tests/train_oracle.py grouped_pack / grouped_vector laid over
the sentinel the buffer held, and (b) on the rows that are images of a real column, what the
library's own vtd_pack_dense / vtd_pack_vector (+ vtd_split_bf16x3 role 1) make of the updated
master.  0xA5 guards stand round every buffer; rows the step must not touch (pad rows inside a
group, the other parts of a shared buffer) hold a sentinel.  Every case runs with the
destination in bf16, split-bf16 and fp32.  The weights are spaced 1 / 128 apart, far more than
three updates of lr = 1e-3 move them, so a misplaced element shows.

Cases (K, N): 20 x 10 in groups of 5 -> 32 at row 96 of a 192-row buffer (a phase-1 pair of
columns spans a group boundary; the other parts' rows stay); 24 x 30 in groups of 10 -> 32
(tiny_mish's query); 30 x 24 with K in groups of 10 -> 32 (its attention_output: runs of 8
packed columns across pads, K_p = 96 no multiple of the tile); 130 x 200 in groups of 40 -> 64
(several tiles both ways, ragged last tiles, the notebook's key_dim); vectors of 30 in groups of
10 -> 32 at offset 32, of 600 and of 1; a position embedding of 50 under the sparse-order rule
without the constraint; a vector of 130 under the sparse-order rule WITH the constraint on the
hostile inputs of tests/test_gpu_adam.py (NaN, inf and denormal gradients, weights within one
update of +-10), where NaN results are compared by position (same_f32), everything else by bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_oracle as A
from tests import train_oracle as T
from tests.test_gpu_adam import Buf, inputs, same_f32

pytestmark = pytest.mark.gpu

LR = 1e-3
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
FORMATS = ["bf16", "bf16x3", "f32"]
# name -> K, N, destination rows (or vector size), K_p, groups / offset, rule, constrain
SPECS = {
    "pair": dict(K=20, N=10, rows=192, kp=64, ng=5, ngp=32, off=96),
    "query": dict(K=24, N=30, rows=96, kp=64, ng=10, ngp=32),
    "attn_out": dict(K=30, N=24, rows=64, kp=96, kg=10, kgp=32),
    "multi": dict(K=130, N=200, rows=320, kp=192, ng=40, ngp=64),
    "plain": dict(K=70, N=17, rows=64, kp=128),
    "vec_groups": dict(N=30, rows=160, ng=10, ngp=32, off=32),
    "vec600": dict(N=600, rows=640),
    "vec1": dict(N=1, rows=64),
    "pos": dict(N=50, rows=50, sparse=True, free=True),
    "sparse_hostile": dict(N=130, rows=192, sparse=True, hostile=True),
    "master_only": dict(K=66, N=6, rows=0),
}


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


def data(spec, rng):
    shape = (spec["K"], spec["N"]) if "K" in spec else (spec["N"],)
    n = int(np.prod(shape))
    w = ((rng.permutation(n) % 2001 - 1000) / 128.0).astype(np.float32)
    gs = [((10.0 ** rng.uniform(-5, 1.3, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
          .reshape(shape) for _ in range(3)]
    return w.reshape(shape), gs


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_table(L, dev, names, fmt, max_weight=10.0, constrain=True, seed=0):
    rng = np.random.default_rng(seed)
    dtype = L.BF16X3 if fmt == "bf16x3" else L.BF16
    pieces = 3 if fmt == "bf16x3" else 1
    st = L.stream_ptr()
    S = []
    for name in names:
        spec = SPECS[name]
        w, gs = inputs((spec["N"],), rng) if spec.get("hostile") else data(spec, rng)
        z = np.zeros_like(w)
        s = dict(spec, name=name, w=w, m=z, v=z, gs=gs, bw=Buf(w, dev), bm=Buf(z, dev),
                 bv=Buf(z, dev), bg=Buf(gs[0], dev), dst=None)
        if spec["rows"]:
            if "K" in spec and fmt != "f32":
                s["before"] = np.full((spec["rows"], pieces * spec["kp"]), SENT16, np.uint16)
            elif "K" in spec:
                s["before"] = np.full((spec["rows"], spec["kp"]), SENT32, np.uint32)
            else:
                s["before"] = np.full(spec["rows"], SENT32, np.uint32)
            s["dst"] = Buf(s["before"], dev)
        S.append(s)
    table = (L.VtdTrainTensor * len(S))()
    for d, s in zip(table, S):
        d.w, d.m, d.v, d.g = s["bw"].ptr, s["bm"].ptr, s["bv"].ptr, s["bg"].ptr
        d.N = s["N"]
        d.constrain = 0 if s.get("free") else 1
        d.rule = L.TRAIN_RULE_SPARSE if s.get("sparse") else L.TRAIN_RULE_DENSE
        if "K" in s:
            d.kind, d.K = L.ADAM_MATRIX, s["K"]
        else:
            d.kind = L.ADAM_VECTOR
        if s["dst"] is None:
            d.packed_dtype = L.TRAIN_PACK_NONE
            continue
        d.packed = s["dst"].ptr
        d.packed_dtype = L.TRAIN_PACK_F32 if fmt == "f32" else L.TRAIN_PACK_MODE
        d.n_group, d.n_group_p = s.get("ng", s["N"]), s.get("ngp", s["N"])
        d.row_offset = s.get("off", 0)
        if "K" in s:
            d.ld = (pieces if fmt != "f32" else 1) * s["kp"]
            d.k_group, d.k_group_p = s.get("kg", s["K"]), s.get("kgp", s["kp"])
    need, tiles = ctypes.c_size_t(), ctypes.c_int()
    L.check(L.lib.vtd_train_plan_bytes(table, len(S), dtype, ctypes.byref(need),
                                       ctypes.byref(tiles)), "plan_bytes")
    plan = Buf(np.zeros(need.value, np.uint8), dev)
    L.check(L.lib.vtd_train_plan_upload(table, len(S), dtype, plan.ptr, need.value, st), "upload")
    for step in (1, 2, 3):
        for s in S:
            s["bg"].write(s["gs"][step - 1])
        L.check(L.lib.vtd_train_step(plan.ptr, len(S), tiles.value, step, LR, 0.9, 0.999, 1e-7,
                                     10.0, int(constrain), max_weight if constrain else 0.0, st),
                "vtd_train_step")
        for s in S:
            rule = T.sparse32 if s.get("sparse") else A.step32
            s["w"], s["m"], s["v"] = rule(s["w"], s["m"], s["v"], s["gs"][step - 1], step, LR,
                                          clipvalue=10.0, max_weight=max_weight,
                                          constrain=constrain and not s.get("free"))
            equal = same_f32 if s.get("hostile") else same      # NaN results: by position
            for key, buf in (("w", "bw"), ("m", "bm"), ("v", "bv")):
                assert equal(s[buf].read(), s[key]), (s["name"], key, step)
            assert same(s["bg"].read(), s["gs"][step - 1]), (s["name"], "g", step)
    plan.read()                                                     # its guards
    out = []
    for s in S:
        out += [s["bw"].read().tobytes(), s["bm"].read().tobytes(), s["bv"].read().tobytes()]
        if s["dst"] is None:
            continue
        got = s["dst"].read()
        out.append(got.tobytes())
        N, rows, off = s["N"], s["rows"], s.get("off", 0)
        ng, ngp = s.get("ng", N), s.get("ngp", N)
        if "K" not in s:
            want = T.grouped_vector(s["w"], rows, ng, ngp, off, fill=s["before"].view(np.float32))
            equal = same_f32 if s.get("hostile") else same
            assert equal(got.view(np.float32), want), (s["name"], "vector destination")
            lib = torch.zeros(rows, dtype=torch.float32, device=dev)
            L.check(L.lib.vtd_pack_vector(s["bw"].ptr, N, ng, ngp, lib.data_ptr(), off, st),
                    "pack_vector")
            at = off + T.grouped_index(np.arange(N), ng, ngp)
            assert same(got.view(np.float32)[at], lib.cpu().numpy()[at]), (s["name"], "library")
            continue
        K, kp = s["K"], s["kp"]
        kg, kgp = s.get("kg", K), s.get("kgp", kp)
        fill = s["before"].view(np.float32) if fmt == "f32" else s["before"]
        want = T.grouped_pack(s["w"], fmt, rows, kp, kg, kgp, ng, ngp, off, fill=fill)
        got = got.view(np.float32) if fmt == "f32" else got
        assert same(got, want), (s["name"], fmt, "destination != the numpy restatement")
        # the library's own pack of the updated device master, on the rows the step owns
        prow = off + T.grouped_index(np.arange(N), ng, ngp)
        if fmt == "bf16":
            lib = torch.zeros((rows, kp), dtype=torch.int16, device=dev)
            L.check(L.lib.vtd_pack_dense(s["bw"].ptr, K, N, kg, kgp, ng, ngp, lib.data_ptr(), kp,
                                         off, L.BF16, st), "pack_dense")
            lib = lib.cpu().numpy().view(np.uint16)
        else:
            f32 = torch.zeros((rows, kp), dtype=torch.float32, device=dev)
            L.check(L.lib.vtd_pack_dense(s["bw"].ptr, K, N, kg, kgp, ng, ngp, f32.data_ptr(), kp,
                                         off, L.F32, st), "pack_dense")
            if fmt == "f32":
                lib = f32.cpu().numpy()
            else:
                lib = torch.zeros((rows, 3 * kp), dtype=torch.int16, device=dev)
                L.check(L.lib.vtd_split_bf16x3(f32.data_ptr(), rows, kp, kp, lib.data_ptr(),
                                               3 * kp, 1, st), "split_bf16x3")
                lib = lib.cpu().numpy().view(np.uint16)
        assert same(got[prow], lib[prow]), (s["name"], fmt, "destination != the library's pack")
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_whole_table_in_one_launch_twice(L, cuda, fmt):
    a = run_table(L, cuda, list(SPECS), fmt)
    b = run_table(L, cuda, list(SPECS), fmt)
    assert a == b, "two runs from the same state differ"


@pytest.mark.parametrize("name", [n for n in SPECS if n != "master_only"])
def test_each_tensor_alone(L, cuda, name):
    for fmt in FORMATS:
        run_table(L, cuda, [name], fmt, seed=3)
    run_table(L, cuda, [name], "bf16", constrain=False, seed=4)


def test_flag_and_rule_are_per_tensor(L, cuda):
    """max_weight = 0.01, far inside the weights' range: the constrained tensors are clipped to
    it, the position embedding (constrain 0) is not, and its sparse-order moments differ in bits
    from the dense rule's on the same inputs (so run_table's comparison tells the rules apart)."""
    for fmt in FORMATS:
        run_table(L, cuda, ["pos", "vec_groups", "attn_out"], fmt, max_weight=0.01)
    rng = np.random.default_rng(0)
    w, gs = data(SPECS["pos"], rng)
    a = b = (w, np.zeros_like(w), np.zeros_like(w))
    for t, g in enumerate(gs, 1):
        a = T.sparse32(*a, g, t, LR, clipvalue=10.0, max_weight=0.01, constrain=False)
        b = A.step32(*b, g, t, LR, clipvalue=10.0, max_weight=0.01, constrain=True)
    assert np.abs(a[0]).max() > 1.0 and np.abs(b[0]).max() <= np.float32(0.01)
    assert a[1].tobytes() != b[1].tobytes() or a[2].tobytes() != b[2].tobytes()


# ------------------------------------------------------------------ the batched fold
def test_fold_table_equals_single_folds(L, cuda):
    """Two jobs of different N_p in one launch against two vtd_fold_layernorm calls, bit for bit
    (random fp32 values: the order of the fp64 sums matters); the first job again on small
    integers, where the sums are exact, against the numpy restatement."""
    st = L.stream_ptr()
    rng = np.random.default_rng(5)
    for integers in (False, True):
        jobs_in = []
        for n_p, k_p, k in ((64, 64, 50), (192, 128, 128)):
            if integers:
                w = rng.integers(-8, 9, (n_p, k_p)).astype(np.float32)
                gamma = rng.integers(-4, 5, k_p).astype(np.float32)
                beta = rng.integers(-4, 5, k_p).astype(np.float32)
                bias = rng.integers(-9, 10, n_p).astype(np.float32) / 2
            else:
                w = rng.standard_normal((n_p, k_p)).astype(np.float32)
                gamma = (1 + 0.3 * rng.standard_normal(k_p)).astype(np.float32)
                beta = (0.3 * rng.standard_normal(k_p)).astype(np.float32)
                bias = rng.standard_normal(n_p).astype(np.float32)
            w[:, k:] = 0
            gamma[k:] = 0
            beta[k:] = 0
            jobs_in.append(dict(w=w, gamma=gamma, beta=beta, bias=bias))
        table = (L.VtdFoldJob * 2)()
        bufs = []
        for j, d in zip(table, jobs_in):
            n_p, k_p = d["w"].shape
            b = dict(w=Buf(d["w"], cuda), gamma=Buf(d["gamma"], cuda), beta=Buf(d["beta"], cuda),
                     bias=Buf(d["bias"], cuda),
                     wo=Buf(np.full((n_p, k_p), SENT16, np.uint16), cuda),
                     bo=Buf(np.full(n_p, SENT32, np.uint32), cuda),
                     cs=Buf(np.full(n_p, SENT32, np.uint32), cuda))
            j.w32, j.gamma, j.beta, j.bias_in = b["w"].ptr, b["gamma"].ptr, b["beta"].ptr, b["bias"].ptr
            j.w_out, j.bias_out, j.colsum = b["wo"].ptr, b["bo"].ptr, b["cs"].ptr
            j.N, j.K, j.ldw, j.ldo = n_p, k_p, k_p, k_p
            bufs.append(b)
        plan = Buf(np.zeros(ctypes.sizeof(table), np.uint8), cuda)
        rows = ctypes.c_int()
        L.check(L.lib.vtd_fold_plan_upload(table, 2, L.BF16, plan.ptr, ctypes.sizeof(table),
                                           ctypes.byref(rows), st), "fold_plan_upload")
        assert rows.value == 192
        L.check(L.lib.vtd_fold_layernorm_batch(plan.ptr, 2, rows.value, L.BF16, st), "fold batch")
        plan.read()
        for d, b in zip(jobs_in, bufs):
            n_p, k_p = d["w"].shape
            wo = torch.zeros((n_p, k_p), dtype=torch.int16, device=cuda)
            bo = torch.zeros(n_p, dtype=torch.float32, device=cuda)
            cs = torch.zeros(n_p, dtype=torch.float32, device=cuda)
            L.check(L.lib.vtd_fold_layernorm(b["w"].ptr, n_p, k_p, k_p, b["gamma"].ptr,
                                             b["beta"].ptr, b["bias"].ptr, wo.data_ptr(), k_p,
                                             L.BF16, bo.data_ptr(), cs.data_ptr(), st), "fold")
            got_w, got_b, got_c = b["wo"].read(), b["bo"].read(), b["cs"].read()
            assert same(got_w, wo.cpu().numpy().view(np.uint16)), n_p
            assert same(got_b.view(np.float32), bo.cpu().numpy()), n_p
            assert same(got_c.view(np.float32), cs.cpu().numpy()), n_p
            for key in ("w", "gamma", "beta", "bias"):
                assert same(b[key].read(), d[key]), key
            if integers:
                rw, rb, rc = T.fold(d["w"], d["gamma"], d["beta"], d["bias"])
                assert same(got_w, rw) and same(got_b.view(np.float32), rb)
                assert same(got_c.view(np.float32), rc)
