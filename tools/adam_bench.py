#!/usr/bin/env python3
"""Timing of the head's optimizer step on the C2 head (presets.VIT_B16_224), bf16 and bf16x3.

  fused    optimizers.Adam.apply in scope "head": one vtd_train_step launch over the head's
           table -- Adam + ClipWeight + the re-pack of the packed operands
  unfused  vtd_adam_step over a master-only table (the same kernel through the vtd_adam_*
           entries, no destinations), then per tensor vtd_pack_dense (in bf16x3: to an fp32
           staging matrix, then vtd_split_bf16x3) / vtd_pack_vector

A and B alternate in rounds inside one process (device events around `--iters` calls each);
the medians and the spread over the rounds are reported, with the achieved TB/s against the
algorithmic byte count: per parameter 16 B in + 12 B out + 2 B (bf16) or 6 B (bf16x3) packed.

--train also times the whole Model.train_head_on_batch at batch 64 with cached features against
the route without the optimizer kernel: head_gradients + Adam in numpy on the host +
set_weights (which re-packs the whole model).

One JSON line per measurement on stdout.  Needs a HIP device; there is no CPU path.
"""
import argparse
import ctypes
import functools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vision_transformer_detector_amd as vtd                      # noqa: E402
from vision_transformer_detector_amd import _lib as L             # noqa: E402


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                   # us per call


def unfused_route(model, opt):
    """The same update without the fusion: a master-only table, then the pack calls."""
    st = opt._state_for(model)
    w = model._head_master()
    table = (L.VtdAdamTensor * len(w))()
    for d, (n, t) in zip(table, w.items()):
        d.w, d.m, d.v, d.g = (t.data_ptr(), st.m[n].data_ptr(), st.v[n].data_ptr(),
                              st.grads[n].data_ptr())
        d.packed = None
        if t.dim() == 2:
            d.kind, d.K, d.N, d.ld = L.ADAM_MATRIX, t.shape[0], t.shape[1], 0
        else:
            d.kind, d.K, d.N, d.ld = L.ADAM_VECTOR, 0, t.numel(), 0
    need, tiles = ctypes.c_size_t(), ctypes.c_int()
    L.check(L.lib.vtd_adam_plan_bytes(table, len(w), model.dtype, ctypes.byref(need),
                                      ctypes.byref(tiles)), "plan_bytes")
    plan = torch.empty(need.value, dtype=torch.uint8, device=model.device)
    L.check(L.lib.vtd_adam_plan_upload(table, len(w), model.dtype, plan.data_ptr(), need.value,
                                       L.stream_ptr()), "plan_upload")
    x3 = model.dtype == L.BF16X3
    packed = {n: model._train_packed[n]["t"] for n in w}
    staging = {}
    for n, t in w.items():
        if t.dim() == 2 and x3:
            rows_p, ld = packed[n].shape
            staging[n] = torch.zeros((rows_p, ld // 3), dtype=torch.float32, device=model.device)

    def run():
        s = L.stream_ptr()
        L.check(L.lib.vtd_adam_step(plan.data_ptr(), len(w), tiles.value, 1, 1e-3, 0.9, 0.999,
                                    1e-7, 10.0, 1, 10.0, s), "adam_step")
        for n, t in w.items():
            p = packed[n]
            if t.dim() == 1:
                L.check(L.lib.vtd_pack_vector(t.data_ptr(), t.numel(), t.numel(), t.numel(),
                                              p.data_ptr(), 0, s), "pack_vector")
                continue
            K, N = t.shape
            if x3:
                f32 = staging[n]
                L.check(L.lib.vtd_pack_dense(t.data_ptr(), K, N, K, K, N, N, f32.data_ptr(),
                                             f32.shape[1], 0, L.F32, s), "pack_dense")
                L.check(L.lib.vtd_split_bf16x3(f32.data_ptr(), f32.shape[0], f32.shape[1],
                                               f32.shape[1], p.data_ptr(), p.shape[1], 1, s),
                        "split")
            else:
                L.check(L.lib.vtd_pack_dense(t.data_ptr(), K, N, K, K, N, N, p.data_ptr(),
                                             p.shape[1], 0, L.BF16, s), "pack_dense")
    return run, plan


def host_route(model, images, labels, feats, state, lr=1e-3):
    """head_gradients + Adam in numpy + set_weights: what a caller had to write before."""
    out5, grads = model.head_gradients(images, labels, encoded=feats)
    wd = model.get_weight_dict()
    state["t"] += 1
    t = state["t"]
    alpha = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    for n in model.head_weight_names():
        g = np.clip(grads[n].cpu().numpy(), -10, 10)
        m = state["m"].setdefault(n, np.zeros_like(g))
        v = state["v"].setdefault(n, np.zeros_like(g))
        m += (g - m) * np.float32(0.1)
        v += (g * g - v) * np.float32(0.001)
        wd[n] = np.clip(wd[n] - np.float32(alpha) * m / (np.sqrt(v) + np.float32(1e-7)), -10, 10)
    model.set_weights(wd)
    torch.cuda.synchronize()
    return out5


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_bench: no HIP device (there is no CPU path)")
    kw = dict(vtd.presets.VIT_B16_224)
    for mode in ("bfloat16", "bf16x3"):
        model = vtd.create_vision_transformer_detector(**kw, dtype=mode, device="cuda:0")
        opt = vtd.optimizers.Adam(learning_rate=1e-3, clipvalue=10)
        model.compile(optimizer=opt, loss=functools.partial(vtd.my_custom_loss))
        params = sum(t.numel() for t in model._head_master().values())
        nbytes = params * (28 + (6 if mode == "bf16x3" else 2))
        fused = functools.partial(opt.apply, model)
        unfused, _plan = unfused_route(model, opt)
        for fn in (fused, unfused):                                   # warm up both
            timed(fn, 20)
        a, b = [], []
        for _ in range(args.rounds):
            a.append(timed(fused, args.iters))
            b.append(timed(unfused, args.iters))
        for name, v in (("fused", a), ("unfused", b)):
            med = statistics.median(v)
            print(json.dumps(dict(what="adam_step", route=name, mode=mode, head_params=params,
                                  us=round(med, 2), us_min=round(min(v), 2),
                                  us_max=round(max(v), 2), bytes=nbytes,
                                  tb_per_s=round(nbytes / med * 1e-6, 3))), flush=True)
        if not args.train:
            continue
        rng = np.random.default_rng(0)
        images = torch.from_numpy(rng.uniform(-1, 1, (args.batch, *kw["input_shape"]))
                                  .astype(np.float32)).to("cuda:0")
        labels = np.tile(np.array([0, -8, -8, -8, -8, -8], np.float32), (args.batch, 17, 1))
        labels[:, 0] = [1, 3, 300, 300, 100, 120]
        feats = model.encode(images)
        step = functools.partial(model.train_head_on_batch, None, labels, encoded=feats)
        timed(step, 5)
        dev = [timed(step, 50) for _ in range(3)]
        state = dict(t=0, m={}, v={})
        host_route(model, None, labels, feats, state)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_route(model, None, labels, feats, state)
            host.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps(dict(what="train_head_on_batch", mode=mode, batch=args.batch,
                              device_us=round(statistics.median(dev), 1),
                              device_steps_per_s=round(1e6 / statistics.median(dev), 1),
                              host_route_us=round(statistics.median(host), 1),
                              host_route_steps_per_s=round(1e6 / statistics.median(host), 2))),
              flush=True)


if __name__ == "__main__":
    main()
