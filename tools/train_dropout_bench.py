"""What dropout costs a whole-model training step: Model.train_on_batch on a dropout=None model
against the same model built with `dropout` and compiled with a `dropout_seed`, in one process.

Both models are built first; then `--rounds` rounds, each `--reps` steps of the plain model
followed by `--reps` steps of the dropout model, device events around every step, after
`--warmup` steps of each.  One JSON object per (mode, batch) on stdout and, with --out, appended
to a file: ms per step of both (mean and the rounds' means) and their ratio.
  python tools/train_dropout_bench.py [--preset vit_b16_224] [--modes bf16x3,bfloat16]
                                      [--batches 64] [--rate 0.1] [--reps 10] [--rounds 3]
                                      [--out FILE.jsonl]"""
import argparse
import functools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vision_transformer_detector_amd as vtd  # noqa: E402
from vision_transformer_detector_amd.presets import PRESETS  # noqa: E402
from tools.train_bench import labels  # noqa: E402


def step_ms(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="vit_b16_224")
    ap.add_argument("--modes", default="bf16x3,bfloat16")
    ap.add_argument("--batches", default="64")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(PRESETS[args.preset])
    rng = np.random.default_rng(0)
    g = torch.Generator(device=dev).manual_seed(1)
    for mode in args.modes.split(","):
        models = {}
        for name, extra, seed in (("plain", dict(dropout=None), None),
                                  ("dropout", dict(dropout=args.rate), args.seed)):
            m = vtd.create_vision_transformer_detector(**dict(kw, **extra), dtype=mode, device=dev)
            m.compile(optimizer=vtd.optimizers.Adam(8e-5, clipvalue=10),
                      loss=functools.partial(vtd.my_custom_loss), dropout_seed=seed)
            models[name] = m
        for batch in (int(b) for b in args.batches.split(",")):
            x = torch.rand((batch,) + tuple(kw["input_shape"]), generator=g, device=dev) * 2 - 1
            y = torch.from_numpy(labels(batch, rng)).to(dev)
            rounds = {name: [] for name in models}
            for name, m in models.items():
                for _ in range(args.warmup):
                    m.train_on_batch(x, y)
            for _ in range(args.rounds):
                for name, m in models.items():
                    ms = [step_ms(lambda: m.train_on_batch(x, y)) for _ in range(args.reps)]
                    rounds[name].append(sum(ms) / len(ms))
            mean = {name: sum(v) / len(v) for name, v in rounds.items()}
            row = dict(preset=args.preset, row="train_dropout", mode=mode, batch=batch,
                       rate=args.rate, reps=args.reps, plain_ms=mean["plain"],
                       plain_ms_rounds=rounds["plain"], dropout_ms=mean["dropout"],
                       dropout_ms_rounds=rounds["dropout"],
                       ratio=mean["dropout"] / mean["plain"],
                       steps_taken=models["dropout"].optimizer.iterations)
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del models


if __name__ == "__main__":
    main()
