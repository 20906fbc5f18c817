"""Whole-model training step benchmark: Model.train_on_batch and its optimizer step.

Rows (one JSON object per line on stdout and, with --out, appended to a file):
  step        optimizers.Adam.apply in scope "all" alone -- the vtd_train_step launch plus, where
              the model is packed with the LayerNorm fold, the vtd_fold_layernorm_batch launch --
              ms per step and achieved TB/s over the bytes the two launches must move: w, m, v,
              g read and w, m, v written (28 B per parameter), every packed destination written,
              and for the fold the fp32 staging read and the folded operand written.
  state       the training state in bytes per parameter: device masters, moments, gradient
              buffers, fold staging, plans.
  train       Model.train_on_batch per batch size: ms per step, and the optimizer's share of it
              (the "step" row's time over this one).
  host_route  the route without the device step, timed by the wall clock with a device
              synchronisation at both ends: Model.gradients, the gradients copied to the host,
              tests/adam_oracle.py step32 in numpy (train_oracle.host_step), set_weights.

Device events around every call, `--warmup` calls first, `--rounds` rounds of `--reps` calls;
the spread given is over the rounds' means.
  python tools/train_bench.py [--preset vit_b16_224] [--modes bf16x3,bfloat16]
                              [--batches 64,256] [--reps 10] [--rounds 3] [--host-route 1]
                              [--out FILE.jsonl]"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vision_transformer_detector_amd as vtd  # noqa: E402
from vision_transformer_detector_amd import _lib as L  # noqa: E402
from vision_transformer_detector_amd.presets import PRESETS  # noqa: E402


def timed(call, reps, rounds, warmup):
    """(mean ms, [per-round mean ms])."""
    for _ in range(warmup):
        call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    means = []
    for _ in range(rounds):
        ms = 0.0
        for _ in range(reps):
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms += t0.elapsed_time(t1)
        means.append(ms / reps)
    return sum(means) / len(means), means


def labels(batch, rng):
    """(B, 17, 6) labels in the loss's format: a few positives with boxes inside the image."""
    y = np.zeros((batch, L.MAX_DETECT, 6), np.float32)
    y[:, :5, 0] = 1.0
    y[:, :5, 1] = rng.integers(0, 80, (batch, 5)) / 79.0
    y[:, :5, 2:4] = rng.uniform(0.3, 0.7, (batch, 5, 2))
    y[:, :5, 4:6] = rng.uniform(0.1, 0.4, (batch, 5, 2))
    return y


def step_bytes(model, state):
    """Bytes the step and the fold must move (see the module doc)."""
    params = model.count_params()
    packed = 0
    for n, where in model._train_packed.items():
        t = where["t"] if where["fold"] is None else None
        count = int(np.prod(model.weight_shapes[n]))
        if t is None:
            packed += 4 * count                       # fp32 staging (real elements)
        else:
            packed += t.element_size() * count * (3 if model.dtype == L.BF16X3 and
                                                  n.endswith("/kernel") else 1)
    fold = sum(s.numel() * 4 + s.numel() * 2 for s in state.staging)
    return 28 * params + packed + fold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="vit_b16_224")
    ap.add_argument("--modes", default="bf16x3,bfloat16")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-route", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = PRESETS[args.preset]
    rng = np.random.default_rng(0)

    def emit(row):
        row = dict(preset=args.preset, **row)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for mode in args.modes.split(","):
        model = vtd.create_vision_transformer_detector(**kw, dtype=mode, device=dev)
        opt = vtd.optimizers.Adam(8e-5, clipvalue=10)
        model.compile(optimizer=opt, loss=functools.partial(vtd.my_custom_loss))
        params = model.count_params()
        grads = opt.gradient_buffers(model, scope="all")
        g = torch.Generator(device=dev).manual_seed(1)
        for t in grads.values():
            t.copy_(1e-3 * torch.randn(t.shape, generator=g, device=dev))
        state = opt._state
        nbytes = step_bytes(model, state)
        ms, means = timed(lambda: opt.apply(model, scope="all"), args.reps, args.rounds,
                          args.warmup)
        emit(dict(row="step", mode=mode, params=params, bytes=nbytes, ms=ms, ms_rounds=means,
                  tb_per_s=nbytes / (ms * 1e-3) / 1e12, tiles=state.tiles,
                  fold_jobs=state.fold_jobs))
        step_ms = ms
        per = lambda tensors: sum(t.numel() * t.element_size() for t in tensors) / params
        emit(dict(row="state", mode=mode, params=params,
                  masters_B_per_param=per(list(model._encoder_master().values()) +
                                          list(model._head_master().values())),
                  moments_B_per_param=per(list(state.m.values()) + list(state.v.values())),
                  gradients_B_per_param=per(state.grads.values()),
                  fold_staging_B_per_param=per(state.staging),
                  plans_bytes=state.plan.numel() + (state.fold_plan.numel() if state.fold_jobs
                                                    else 0)))
        for batch in (int(b) for b in args.batches.split(",")):
            x = torch.rand((batch,) + tuple(kw["input_shape"]), generator=g, device=dev) * 2 - 1
            y = torch.from_numpy(labels(batch, rng)).to(dev)
            model.set_weights(model.get_weight_dict())          # fresh moments per batch size
            ms, means = timed(lambda: model.train_on_batch(x, y), args.reps, args.rounds,
                              args.warmup)
            emit(dict(row="train", mode=mode, batch=batch, ms=ms, ms_rounds=means,
                      optimizer_share=step_ms / ms))
            if not args.host_route:
                continue
            sys.path.insert(0, ROOT)
            from tests import train_oracle as T
            names = model.weight_names()
            w = model.get_weight_dict()
            m = {n: np.zeros_like(w[n]) for n in names}
            v = {n: np.zeros_like(w[n]) for n in names}
            parts = dict(gradients=0.0, to_host=0.0, numpy_step=0.0, set_weights=0.0)
            steps = 2
            for t in range(1, steps + 1):
                torch.cuda.synchronize()
                a = time.perf_counter()
                _, gr = model.gradients(x, y)
                torch.cuda.synchronize()
                b = time.perf_counter()
                gh = {n: gr[n].cpu().numpy() for n in names}
                c = time.perf_counter()
                for n in names:
                    w[n], m[n], v[n] = T.host_step(n, w[n], m[n], v[n], gh[n], t, 8e-5)
                d = time.perf_counter()
                model.set_weights(w)
                torch.cuda.synchronize()
                e = time.perf_counter()
                for key, dt in zip(parts, (b - a, c - b, d - c, e - d)):
                    parts[key] += 1e3 * dt / steps
            emit(dict(row="host_route", mode=mode, batch=batch, ms=sum(parts.values()),
                      ms_parts=parts, steps=steps))
        del model, opt, state, grads


if __name__ == "__main__":
    main()
