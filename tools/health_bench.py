#!/usr/bin/env python3
"""Timing of the numerical-health pass at C2 (presets.VIT_B16_224, 180 M parameters, scope "all").

  weight_stats     Model.weight_stats(): the vtd_tensor_stats launch pair over the device masters
                   plus the one host read of the records (host clock; the read synchronises)
  gradient_stats   optimizers.Adam.gradient_stats(model) over the gradient buffers, likewise
  launch_pair      the two kernels alone (device events around `--iters` launch pairs), with the
                   achieved GB/s against the bytes the pass must read: 4 per element
  host_route       what a caller had before: max(np.amax(w) for w in model.get_weights()) after a
                   training step, which reads every stepped weight back to the host

The device routes alternate in rounds inside one process; medians and the spread over the rounds
are reported.  One JSON line per measurement on stdout.  Needs a HIP device; there is no CPU path.
"""
import argparse
import contextlib
import functools
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vision_transformer_detector_amd as vtd                      # noqa: E402


def host_clock(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters                 # us per call


def device_clock(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                   # us per call


def report(what, v, **extra):
    med = statistics.median(v)
    print(json.dumps(dict(what=what, us=round(med, 1), us_min=round(min(v), 1),
                          us_max=round(max(v), 1), **extra)), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mode", default="bfloat16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("health_bench: no HIP device (there is no CPU path)")
    kw = dict(vtd.presets.VIT_B16_224)
    model = vtd.create_vision_transformer_detector(**kw, dtype=args.mode, device="cuda:0")
    opt = vtd.optimizers.Adam(learning_rate=1e-4, clipvalue=10)
    model.compile(optimizer=opt, loss=functools.partial(vtd.my_custom_loss))
    rng = np.random.default_rng(0)
    images = torch.from_numpy(rng.uniform(-1, 1, (args.batch, *kw["input_shape"]))
                              .astype(np.float32)).to("cuda:0")
    labels = np.tile(np.array([0, -8, -8, -8, -8, -8], np.float32), (args.batch, 17, 1))
    labels[:, 0] = [1, 3, 300, 300, 100, 120]
    model.train_on_batch(images, labels)
    params = model.count_params()
    nbytes = 4 * params

    ws = model.weight_stats()
    gs = opt.gradient_stats(model)
    print(json.dumps(dict(what="check", params=params, tensors=len(ws),
                          weights_finite=all(s.finite for s in ws.values()),
                          weights_max=max(s.max for s in ws.values()),
                          gradients_finite=all(s.finite for s in gs.values()),
                          global_norm=opt.global_norm(model))), flush=True)
    wplan = model._health_plan[1]
    gplan = opt._state.health_plans["g"]
    routes = (("weight_stats", lambda: model.weight_stats(), host_clock),
              ("gradient_stats", lambda: opt.gradient_stats(model), host_clock),
              ("launch_pair_weights", wplan.launch, device_clock),
              ("launch_pair_gradients", gplan.launch, device_clock))
    for _, fn, clock in routes:                                       # warm up
        clock(fn, 5)
    times = {name: [] for name, _, _ in routes}
    for _ in range(args.rounds):
        for name, fn, clock in routes:
            times[name].append(clock(fn, args.iters))
    for name, _, _ in routes:
        med = statistics.median(times[name])
        extra = dict(mode=args.mode, params=params, chunks=wplan.chunks)
        if name.startswith("launch_pair"):
            extra.update(bytes=nbytes, gb_per_s=round(nbytes / med * 1e-3, 1))
        report(name, times[name], **extra)

    host = []
    for _ in range(3):
        model.train_on_batch(images, labels)                          # the masters move ahead
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top = max(np.amax(w) for w in model.get_weights())
        host.append((time.perf_counter() - t0) * 1e6)
    report("host_route", host, mode=args.mode, params=params, max_weight=float(top))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):                   # its messages are not JSON
        top_dev = vtd.check_weights(model)
    print(json.dumps(dict(what="check_weights", us=round((time.perf_counter() - t0) * 1e6, 1),
                          max_weight=float(top_dev), same_as_host_route=bool(top_dev == top))),
          flush=True)
    step = [device_clock(lambda: model.train_on_batch(images, labels), 5) for _ in range(3)]
    report("train_on_batch", step, mode=args.mode, batch=args.batch)


if __name__ == "__main__":
    main()
