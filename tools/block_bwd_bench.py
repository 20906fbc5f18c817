"""Encoder-block backward micro-benchmark through the C-ABI.  The rows it measures now are the
LayerNorm backward's: us per call of vtd_layernorm_backward at
  C2    rows 256 * 196, D 768
  long  rows 32 * 1600, D 768
with and without `add`, with and without dgamma / dbeta, next to the backward of
torch.nn.functional.layer_norm on the same device and shapes.  The yardstick is bytes moved over
time: x, dy (and add) read once and dx written once, 16 B per element with add and 12 B without.
Device events around every call, 3 warm-up calls, `--rounds` interleaved rounds of `--reps`
calls each: the spread is over the rounds' means (the method of tools/attn_bwd_bench.py).
  python tools/block_bwd_bench.py [--reps 10] [--rounds 3] [--shapes C2,long] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_transformer_detector_amd import _lib as L  # noqa: E402

SHAPES = {"C2": (256 * 196, 768), "long": (32 * 1600, 768)}
EPS = 1e-3


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


def library_calls(rows, D, dev):
    """{name: (call, bytes per element)} for the four forms of vtd_layernorm_backward."""
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(rows, D, generator=g, device=dev)
    dy = torch.randn(rows, D, generator=g, device=dev)
    add = torch.randn(rows, D, generator=g, device=dev)
    gamma = 1 + 0.1 * torch.randn(D, generator=g, device=dev)
    dx = torch.empty_like(x)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    stat = torch.empty(rows, 2, device=dev)
    st = L.stream_ptr()
    L.check(L.lib.vtd_layernorm_stats(x.data_ptr(), L.F32, rows, D, D, EPS, stat.data_ptr(), st))
    n = L.c_size_t(0)
    L.check(L.lib.vtd_layernorm_backward_workspace_bytes(rows, D, ctypes.byref(n)))
    ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
    keep = (x, dy, add, gamma, dx, dg, db, stat, ws)

    def form(with_add, with_params):
        return lambda: L.check(L.lib.vtd_layernorm_backward(
            x.data_ptr(), D, stat.data_ptr(), gamma.data_ptr(), dy.data_ptr(), D,
            add.data_ptr() if with_add else None, D, rows, D, dx.data_ptr(), D,
            dg.data_ptr() if with_params else None, db.data_ptr() if with_params else None,
            ws.data_ptr(), n.value, st))

    return {"vtd:add+params": (form(True, True), 16), "vtd:params": (form(False, True), 12),
            "vtd:add": (form(True, False), 16), "vtd:dx_only": (form(False, False), 12),
            "vtd:stats": (lambda: L.check(L.lib.vtd_layernorm_stats(
                x.data_ptr(), L.F32, rows, D, D, EPS, stat.data_ptr(), st)), 4)}, keep


def torch_calls(rows, D, dev):
    """The backward alone of torch's layer_norm (graph retained): all three gradients, and dx
    alone.  Neither adds a residual gradient, so both move 12 B per element."""
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(rows, D, generator=g, device=dev).requires_grad_(True)
    dy = torch.randn(rows, D, generator=g, device=dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g, device=dev)).requires_grad_(True)
    beta = torch.zeros(D, device=dev).requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (D,), gamma, beta, eps=EPS)
    return {"torch:params": (lambda: torch.autograd.grad(y, (x, gamma, beta), dy,
                                                         retain_graph=True), 12),
            "torch:dx_only": (lambda: torch.autograd.grad(y, (x,), dy, retain_graph=True), 12)}


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
        rows, D = SHAPES[name]
        calls, keep = library_calls(rows, D, dev)
        calls.update(torch_calls(rows, D, dev))
        for f, _ in calls.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        us = {n: [] for n in calls}
        for _ in range(a.rounds):
            for n, (f, _) in calls.items():
                us[n].append(timed(f, a.reps))
        for n, v in us.items():
            who, what = n.split(":")
            mean = sum(v) / len(v)
            per = calls[n][1]
            rec = {"kernel": "layernorm_backward", "shape": name, "rows": rows, "D": D,
                   "impl": who, "call": what, "us_mean": round(mean, 1), "us_min": round(min(v), 1),
                   "us_max": round(max(v), 1), "rounds": a.rounds, "reps": a.reps,
                   "bytes_per_element": per,
                   "tb_per_s": round(per * rows * D / mean / 1e6, 2)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        del calls, keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
