"""vtd_adam_step on the GPU against tests/adam_oracle.py, bit for bit: w, m, v equal step32 as raw
uint32 (NaN by isnan), the packed operands equal pack_ref and what vtd_pack_dense
(+ vtd_split_bf16x3 role 1) makes of the updated master, g is unchanged, nothing outside the
documented region is written (0xA5 guards round every buffer, a sentinel in the packed rows
the step must not touch), and two runs from the same state give the same bytes.

Shapes (K, N): 64 x 64 one whole tile; 70 x 17 ragged both ways with rows that are not 16-B
aligned; 130 x 6 N under one vector and three K tiles, here with K_p = 256 so that a fourth K
tile holds only zero padding; 1 x 1 with K_p = 72 (not a multiple of the tile); 200 x 136
several tiles both ways; biases of 17 and 130."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_oracle as A

pytestmark = pytest.mark.gpu

GUARD = 256                       # bytes of 0xA5 on each side (keeps the 16-B alignment)
SENTINEL = 0x5A
LR = 1e-3
# (shape, K_p or None for round_up(K, 64))
SPECS = [((64, 64), None), ((70, 17), None), ((130, 6), 256), ((1, 1), 72), ((200, 136), None),
         ((17,), None), ((130,), None)]
IDS = ["64x64", "70x17", "130x6", "1x1", "200x136", "bias17", "bias130"]
MODES = {"bf16": 1, "bf16x3": 3}


def up64(n):
    return -(-n // 64) * 64


@pytest.fixture(scope="module")
def L(cuda):
    from vision_transformer_detector_amd import _lib
    return _lib


class Buf:
    """A device buffer inside 0xA5 guards."""

    def __init__(self, content, dev):
        content = np.ascontiguousarray(content)
        self.dtype, self.shape = content.dtype, content.shape
        raw = np.full(content.nbytes + 2 * GUARD, 0xA5, np.uint8)
        raw[GUARD:GUARD + content.nbytes] = content.view(np.uint8).reshape(-1)
        self.n = content.nbytes
        self.t = torch.from_numpy(raw).to(dev)
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def write(self, content):
        content = np.ascontiguousarray(content, self.dtype)
        assert content.nbytes == self.n
        self.t[GUARD:GUARD + self.n].copy_(torch.from_numpy(content.view(np.uint8).reshape(-1)))

    def read(self):
        raw = self.t.cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + self.n:] == 0xA5).all(), "guard hit"
        return raw[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()


def inputs(shape, rng):
    """Weights with values within one update (lr) of +-10, gradients with values beyond +-10,
    exact zeros, denormals, a NaN and an inf; three gradient sets for steps 1, 2, 3."""
    n = int(np.prod(shape))
    w = (3.0 * rng.standard_normal(n)).astype(np.float32)
    near = np.array([10.0 - 2e-4, -10.0 + 2e-4, 9.9995, -9.9999, 10.0, -10.0], np.float32)
    gs = []
    for _ in range(3):
        g = ((10.0 ** rng.uniform(-6, 1.3, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        gs.append(g)
    if n > 1:
        k = min(len(near), n // 2)
        w[:k] = near[:k]
        for g in gs:                                 # push the near-limit weights outwards
            g[:k] = -np.sign(near[:k]) * np.abs(g[:k])
        special = np.array([np.nan, np.inf, 0.0, -0.0, 1e-40, -3e-42, 30.0, -1e3, -np.inf, 12.5],
                           np.float32)
        k2 = min(len(special), n - k)
        for i, g in enumerate(gs):
            g[n - k2:] = np.roll(special, i)[:k2]
    else:
        w[0], gs[0][0], gs[1][0], gs[2][0] = 9.9995, -37.0, 1e-40, 0.25
    return w.reshape(shape), [g.reshape(shape) for g in gs]


def same_f32(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    return bool((np.isnan(got) == nan).all()
                and (got.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all())


def same_bf16(got, ref):
    nan = A.bf16_isnan(ref)
    return bool((A.bf16_isnan(got) == nan).all() and (got[~nan] == ref[~nan]).all())


def run_table(L, dev, which, mode, clip, constrain, seed=0):
    """Three chained steps of the tensors `which` (indices into SPECS) in one table; checks
    every step against step32 and the packed outputs at the end.  Returns the final bytes."""
    rng = np.random.default_rng(seed)
    dtype = {"bf16": L.BF16, "bf16x3": L.BF16X3, None: L.F32}[mode]
    pieces = MODES.get(mode, 0)
    T = []
    for i in which:
        shape, kp = SPECS[i]
        w, gs = inputs(shape, rng)
        t = dict(shape=shape, w=w, m=np.zeros_like(w), v=np.zeros_like(w), gs=gs,
                 bw=Buf(w, dev), bm=Buf(np.zeros_like(w), dev), bv=Buf(np.zeros_like(w), dev),
                 bg=Buf(gs[0], dev), packed=None)
        if mode is not None:
            if len(shape) == 2:
                t["kp"], t["np"] = kp or up64(shape[0]), up64(shape[1])
                t["packed"] = Buf(np.full((t["np"], pieces * t["kp"]), SENTINEL * 0x0101,
                                          np.uint16), dev)
            else:
                t["np"] = up64(shape[0])
                t["packed"] = Buf(np.full(t["np"], SENTINEL * 0x01010101, np.uint32), dev)
        T.append(t)
    table = (L.VtdAdamTensor * len(T))()
    for d, t in zip(table, T):
        d.w, d.m, d.v, d.g = t["bw"].ptr, t["bm"].ptr, t["bv"].ptr, t["bg"].ptr
        d.packed = t["packed"].ptr if t["packed"] is not None else None
        if len(t["shape"]) == 2:
            d.kind, d.K, d.N = L.ADAM_MATRIX, t["shape"][0], t["shape"][1]
            d.ld = pieces * t["kp"] if mode is not None else 0
        else:
            d.kind, d.K, d.N, d.ld = L.ADAM_VECTOR, 0, t["shape"][0], 0
    need, tiles = ctypes.c_size_t(), ctypes.c_int()
    L.check(L.lib.vtd_adam_plan_bytes(table, len(T), dtype, ctypes.byref(need),
                                      ctypes.byref(tiles)), "plan_bytes")
    plan = Buf(np.zeros(need.value, np.uint8), dev)
    st = L.stream_ptr()
    L.check(L.lib.vtd_adam_plan_upload(table, len(T), dtype, plan.ptr, need.value, st), "upload")
    for step in (1, 2, 3):
        for t in T:
            t["bg"].write(t["gs"][step - 1])
        L.check(L.lib.vtd_adam_step(plan.ptr, len(T), tiles.value, step, LR, 0.9, 0.999, 1e-7,
                                    clip or 0.0, int(constrain), 10.0 if constrain else 0.0, st),
                "vtd_adam_step")
        for i, t in zip(which, T):
            t["w"], t["m"], t["v"] = A.step32(t["w"], t["m"], t["v"], t["gs"][step - 1], step, LR,
                                              clipvalue=clip, max_weight=10.0, constrain=constrain)
            for key, buf in (("w", "bw"), ("m", "bm"), ("v", "bv")):
                assert same_f32(t[buf].read(), t[key]), (IDS[i], key, step)
            assert t["bg"].read().tobytes() == t["gs"][step - 1].tobytes(), (IDS[i], "g", step)
    plan.read()                                                     # its guards
    out = []
    for i, t in zip(which, T):
        out += [t["bw"].read().tobytes(), t["bm"].read().tobytes(), t["bv"].read().tobytes()]
        if t["packed"] is None:
            continue
        got = t["packed"].read()
        out.append(got.tobytes())
        N = t["shape"][-1]
        if len(t["shape"]) == 1:
            assert same_f32(got[:N].view(np.float32), t["w"]), (IDS[i], "packed bias")
            assert (got[N:] == SENTINEL * 0x01010101).all(), (IDS[i], "bias beyond N written")
            continue
        ref = A.pack_ref(t["w"], t["kp"], t["np"], mode)
        assert same_bf16(got[:N], ref[:N]), (IDS[i], "packed rows < N")
        assert (got[N:] == SENTINEL * 0x0101).all(), (IDS[i], "packed rows >= N written")
        # the unfused route on the updated device master: vtd_pack_dense (+ split, role 1)
        K, kp, np_ = t["shape"][0], t["kp"], t["np"]
        if mode == "bf16":
            un = torch.zeros((np_, kp), dtype=torch.int16, device=dev)
            L.check(L.lib.vtd_pack_dense(t["bw"].ptr, K, N, K, K, N, N, un.data_ptr(), kp, 0,
                                         L.BF16, st), "pack_dense")
        else:
            f32 = torch.zeros((np_, kp), dtype=torch.float32, device=dev)
            un = torch.zeros((np_, 3 * kp), dtype=torch.int16, device=dev)
            L.check(L.lib.vtd_pack_dense(t["bw"].ptr, K, N, K, K, N, N, f32.data_ptr(), kp, 0,
                                         L.F32, st), "pack_dense")
            L.check(L.lib.vtd_split_bf16x3(f32.data_ptr(), np_, kp, kp, un.data_ptr(), 3 * kp, 1,
                                           st), "split_bf16x3")
        un = un.cpu().numpy().view(np.uint16)
        assert same_bf16(got[:N], un[:N]), (IDS[i], "fused != vtd_pack_dense of the new master")
        finite = np.isfinite(t["w"])
        if finite.all():
            assert got[:N].tobytes() == un[:N].tobytes(), IDS[i]
    return out


SETTINGS = [(mode, clip, constrain) for mode in ("bf16", "bf16x3") for clip in (10.0, None)
            for constrain in (True, False)]


@pytest.mark.parametrize("mode,clip,constrain", SETTINGS + [(None, 10.0, True)],
                         ids=lambda v: str(v))
def test_whole_table_in_one_launch(L, cuda, mode, clip, constrain):
    a = run_table(L, cuda, range(len(SPECS)), mode, clip, constrain)
    b = run_table(L, cuda, range(len(SPECS)), mode, clip, constrain)
    assert a == b, "two runs from the same state differ"


@pytest.mark.parametrize("index", range(len(SPECS)), ids=IDS)
def test_each_tensor_alone(L, cuda, index):
    for mode in ("bf16", "bf16x3"):
        run_table(L, cuda, [index], mode, 10.0, True, seed=index)
        run_table(L, cuda, [index], mode, None, False, seed=index)
    run_table(L, cuda, [index], None, 10.0, True, seed=index)


def test_inputs_cover_the_cases():
    """The generated data really holds what the docstring of inputs() promises."""
    w, gs = inputs((70, 17), np.random.default_rng(0))
    g = gs[0].reshape(-1)
    assert np.isnan(g).any() and np.isinf(g).any() and (g == 0).any()
    assert (np.abs(g[np.isfinite(g)]) > 10).any()
    tiny = np.abs(g[np.isfinite(g) & (g != 0)])
    assert (tiny < np.finfo(np.float32).tiny).any()
    assert ((10.0 - np.abs(w.reshape(-1))) < LR).any()
