"""Attention backward micro-benchmark through the C-ABI: us per call of vtd_attention_train
and vtd_attention_backward, in both operand modes, at
  C2    B 256, N 196, 12 heads x 64
  long  B 32, N 1600, 12 heads x 64
next to (a) the same build's vtd_attention on the shape and (b) the backward of
torch.nn.functional.scaled_dot_product_attention in bf16 on the same device, if it runs there.
Device events around every call, 3 warm-up calls, `--rounds` interleaved rounds of `--reps`
calls each: the spread is over the rounds' means.
  python tools/attn_bwd_bench.py [--reps 10] [--rounds 3] [--shapes C2,long] [--out FILE.json]"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_transformer_detector_amd import _lib as L  # noqa: E402

SHAPES = {"C2": (256, 196, 12, 64), "long": (32, 1600, 12, 64)}


def timed(call, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = 0.0
    for _ in range(reps):
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        ms += t0.elapsed_time(t1)
    return 1e3 * ms / reps


def library_calls(mode, B, N, H, dkp, dev):
    """{name: call} for vtd_attention, vtd_attention_train, vtd_attention_backward."""
    g = torch.Generator(device=dev).manual_seed(0)
    x3 = mode == "x3"
    code = L.BF16X3 if x3 else L.BF16
    tdt = torch.float32 if x3 else torch.bfloat16
    inner, ld = H * dkp, 3 * H * dkp
    qkv = (torch.randn(B * N, ld, generator=g, device=dev) * 1.5).to(tdt)
    do = torch.randn(B * N, inner, generator=g, device=dev).to(tdt)
    ldo = 2 * inner if x3 else inner
    ldd = 2 * ld if x3 else ld
    out = torch.empty(B * N, ldo, device=dev, dtype=torch.bfloat16)
    out2 = torch.empty_like(out)
    lse = torch.empty(B * H * N, device=dev, dtype=torch.float32)
    dqkv = torch.empty(B * N, ldd, device=dev, dtype=torch.bfloat16)
    n = L.c_size_t(0)
    L.check(L.lib.vtd_attention_backward_workspace_bytes(B, N, H, dkp, code, ctypes.byref(n)))
    ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
    st, scale = L.stream_ptr(), 1 / math.sqrt(dkp)
    keep = (qkv, do, out, out2, lse, dqkv, ws)
    return {
        "attention": lambda: L.check(L.lib.vtd_attention(
            qkv.data_ptr(), B, N, H, dkp, ld, scale, out2.data_ptr(), ldo, code, st)),
        "train": lambda: L.check(L.lib.vtd_attention_train(
            qkv.data_ptr(), B, N, H, dkp, ld, scale, out.data_ptr(), ldo, lse.data_ptr(), code, st)),
        "backward": lambda: L.check(L.lib.vtd_attention_backward(
            qkv.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), B, N, H, dkp, ld, ldo,
            inner, scale, dqkv.data_ptr(), ldd, code, ws.data_ptr(), n.value, st)),
    }, keep


def sdpa_backward_call(B, N, H, dkp, dev):
    """The backward alone of torch's scaled_dot_product_attention in bf16 (graph retained)."""
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = ((torch.randn(B, H, N, dkp, generator=g, device=dev) * 1.5).to(torch.bfloat16)
               .requires_grad_(True) for _ in range(3))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    do = torch.randn(B, H, N, dkp, generator=g, device=dev).to(torch.bfloat16)
    return lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2,long")
    ap.add_argument("--out", default=None, help="also write the results as one JSON file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for name in a.shapes.split(","):
        B, N, H, dkp = SHAPES[name]
        calls, keep = {}, []
        for mode in ("x3", "bf16"):
            c, k = library_calls(mode, B, N, H, dkp, dev)
            keep.append(k)
            calls.update({f"{mode}:{n}": f for n, f in c.items()})
        try:
            calls["torch_sdpa_bf16:backward"] = sdpa_backward_call(B, N, H, dkp, dev)
            calls["torch_sdpa_bf16:backward"]()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001  (reported, not hidden: the comparison is optional)
            calls.pop("torch_sdpa_bf16:backward", None)
            print(json.dumps({"shape": name, "torch_sdpa_bf16": f"did not run: {e}"}), flush=True)
        for f in calls.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        us = {n: [] for n in calls}
        for _ in range(a.rounds):
            for n, f in calls.items():
                us[n].append(timed(f, a.reps))
        for n, v in us.items():
            who, what = n.split(":")
            products = {"attention": 2, "train": 2}.get(what, 8 if who == "x3" else 7)
            if who.startswith("torch"):
                products = 5
            rec = {"shape": name, "B": B, "N": N, "heads": H, "dkp": dkp, "impl": who, "call": what,
                   "us_mean": round(sum(v) / len(v), 1), "us_min": round(min(v), 1),
                   "us_max": round(max(v), 1), "rounds": a.rounds, "reps": a.reps,
                   "mfma_products": products,
                   "tflops": round(products * 2.0 * B * H * N * N * dkp / (sum(v) / len(v)) / 1e6, 1)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
