"""Cost of the in-kernel dropout mask: us per call of vtd_attention_train_dropout,
vtd_attention_backward_dropout and the whole block (vtd_encoder_block_backward_dropout, forward +
backward, d 768, q 3) at rate 0 (the existing kernels) and rate 0.1 (the DROP instantiations), in
both operand modes, at C2's block (B 64, N 196, 12 heads x 64).  The method
of tools/attn_bwd_bench.py: device events around every call, 3 warm-up calls, `--rounds`
interleaved rounds of `--reps` calls; the dropout cost is the ratio to the rate-0 figure of the
same run.
  python tools/dropout_bench.py [--reps 10] [--rounds 3] [--out FILE.jsonl]"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_transformer_detector_amd import _lib as L  # noqa: E402
from tools.attn_bwd_bench import timed  # noqa: E402

B, N, H, DKP = 64, 196, 12, 64
D_MODEL, MLP_Q = 768, 3


def calls_of(mode, rate, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x3 = mode == "x3"
    code = L.BF16X3 if x3 else L.BF16
    tdt = torch.float32 if x3 else torch.bfloat16
    inner, ld = H * DKP, 3 * H * DKP
    qkv = (torch.randn(B * N, ld, generator=g, device=dev) * 1.5).to(tdt)
    do = torch.randn(B * N, inner, generator=g, device=dev).to(tdt)
    ldo, ldd = (2 * inner, 2 * ld) if x3 else (inner, ld)
    out = torch.empty(B * N, ldo, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * H * N, device=dev, dtype=torch.float32)
    dqkv = torch.empty(B * N, ldd, device=dev, dtype=torch.bfloat16)
    n = L.c_size_t(0)
    L.check(L.lib.vtd_attention_backward_workspace_bytes(B, N, H, DKP, code, ctypes.byref(n)))
    ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
    st, scale = L.stream_ptr(), 1 / math.sqrt(DKP)
    drop = L.VtdDropout(seed=1, step=0, site=0, rate=rate)
    keep = (qkv, do, out, lse, dqkv, ws, drop)
    return {
        "train": lambda: L.check(L.lib.vtd_attention_train_dropout(
            qkv.data_ptr(), B, N, H, DKP, ld, scale, out.data_ptr(), ldo, lse.data_ptr(), code, st,
            ctypes.byref(drop))),
        "backward": lambda: L.check(L.lib.vtd_attention_backward_dropout(
            qkv.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), B, N, H, DKP, ld, ldo,
            inner, scale, dqkv.data_ptr(), ldd, code, ws.data_ptr(), n.value, st,
            ctypes.byref(drop))),
    }, keep


def block_call(mode, rate, dev):
    """The whole block, forward + backward, through vtd_encoder_block_backward_dropout."""
    from vision_transformer_detector_amd import encoder
    g = torch.Generator(device=dev).manual_seed(1)
    w = []
    for shape in encoder.weight_shapes(D_MODEL, H, DKP, MLP_Q):
        if len(shape) == 1 or shape == (H, DKP):
            t = 0.05 * torch.randn(shape, generator=g, device=dev)
        else:
            t = torch.randn(shape, generator=g, device=dev) / (shape[0] if len(shape) == 2 else D_MODEL) ** 0.5
        w.append(t)
    w[0] += 1.0
    w[10] += 1.0
    x = torch.randn(B, N, D_MODEL, generator=g, device=dev)
    dy = torch.randn(B, N, D_MODEL, generator=g, device=dev)
    dims = encoder.block_dims(B, N, D_MODEL, H, DKP, MLP_Q, False, "bf16x3" if mode == "x3" else "bfloat16")
    ws = torch.empty(encoder.workspace_bytes(dims), device=dev, dtype=torch.uint8)
    out = (torch.empty_like(x), [torch.empty_like(t) for t in w], torch.empty_like(x))
    drop = L.VtdBlockDropout(seed=1, step=0, site_base=0, rate=rate)
    return (lambda: encoder.run(x, w, dims, dy=dy, ws=ws, out=out, drop=drop)), (w, x, dy, ws, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the records to this JSON-lines file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    calls, keep = {}, []
    for mode in ("x3", "bf16"):
        for rate in (0.0, 0.1):
            c, k = calls_of(mode, rate, dev)
            keep.append(k)
            calls.update({(mode, what, rate): f for what, f in c.items()})
            f, k = block_call(mode, rate, dev)
            keep.append(k)
            calls[(mode, "block_forward_backward", rate)] = f
    for (mode, what, rate), f in calls.items():     # the forward first: the backward reads its O
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {n: [] for n in calls}
    for _ in range(a.rounds):
        for n, f in calls.items():
            us[n].append(timed(f, a.reps))
    recs = []
    for (mode, what, rate), v in us.items():
        base = us[(mode, what, 0.0)]
        recs.append({"bench": "dropout", "B": B, "N": N, "heads": H, "dkp": DKP, "impl": mode,
                     "call": what, "rate": rate, "us_mean": round(sum(v) / len(v), 1),
                     "us_min": round(min(v), 1), "us_max": round(max(v), 1), "rounds": a.rounds,
                     "reps": a.reps, "ratio_to_rate0": round(sum(v) / sum(base), 3)})
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
