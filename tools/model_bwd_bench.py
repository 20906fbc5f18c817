"""Cost of the whole-model gradients on the device (DESIGN.md "Whole-model gradients") at
ViT-B/16 @224 (C2), batch 64 and 256, in both operand modes:
 1. Model.gradients in ms per call, beside the sum of its parts at the same shapes in the same
    session: the stem forward and backward (vtd_stem_backward), one block's forward-only and
    forward + backward call (vtd_encoder_block_backward, times the depth) and the head pass
    (head_gradients on cached features);
 2. the stem in us per call, and for stem_grad_rows_kernel the GB/s over the bytes it moves
    (dx0 read, the G operand and the row sums written), from the library's profiler: the
    "other" class of a stem backward call without x0 is that kernel, the one-block batch
    reduce of the row sums and the events around both: an upper bound on the kernel's time.
Device events around every call, `--warmup` warm-up calls, `--rounds` interleaved rounds of
`--reps` calls each; mean and range are over the rounds' means (the method of
tools/block_bwd_bench.py).  Needs a HIP device.
  python tools/model_bwd_bench.py [--batches 64,256] [--reps 10] [--rounds 3] [--out FILE.json]"""
import argparse
import ctypes
import functools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vision_transformer_detector_amd as vtd  # noqa: E402
from vision_transformer_detector_amd import _lib as L  # noqa: E402
from vision_transformer_detector_amd import encoder, stem  # noqa: E402


def timed(call, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = 0.0
    for _ in range(reps):
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        ms += t0.elapsed_time(t1)
    return ms / reps


def labels(rng, B):
    y = np.full((B, 17, 6), -8.0, np.float32)
    y[..., 0] = 0.0
    y[:, :5, 0] = 1.0
    y[:, :5, 1] = rng.integers(0, 80, (B, 5))
    y[:, :5, 2:4] = rng.uniform(60, 548, (B, 5, 2))
    y[:, :5, 4:6] = rng.uniform(8, 300, (B, 5, 2))
    return y


def profiled_other_us(call, reps):
    """us per call in the profiler's "other" class (launch-time events, one stream)."""
    L.check(L.lib.vtd_profile_reset())
    L.check(L.lib.vtd_profile_enable(1))
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    L.check(L.lib.vtd_profile_enable(0))
    ms = (ctypes.c_double * L.PROF_CLASSES)()
    nl = (ctypes.c_int64 * L.PROF_CLASSES)()
    fl = (ctypes.c_double * L.PROF_CLASSES)()
    L.check(L.lib.vtd_profile_read(ms, nl, fl, L.PROF_CLASSES))
    return 1e3 * ms[4] / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", default="vit_b16_224")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_bwd_bench needs a HIP device")
    dev = torch.device("cuda:0")
    kw = vtd.presets.PRESETS[a.preset]
    rng = np.random.default_rng(0)
    records = []
    for B in [int(b) for b in a.batches.split(",")]:
        for mode in ("bfloat16", "bf16x3"):
            model = vtd.create_vision_transformer_detector(**kw, dtype=mode, device=dev)
            model.compile(loss=functools.partial(vtd.my_custom_loss))
            d, reps_enc = model.dims, kw["encoder_repeat_times"]
            H, W, C = model.input_shape
            images = torch.from_numpy(rng.uniform(-1, 1, (B, H, W, C)).astype(np.float32)).to(dev)
            y = labels(rng, B)
            sw = list(model.stem_weights().values())
            bw = list(model.encoder_block_weights(0).values())
            sdims = stem.stem_dims(B, H, W, C, kw["patch_size"], d.d, mode)
            bdims = encoder.block_dims(B, d.tokens, d.d, kw["encoder_num_heads"],
                                       kw["encoder_key_dim"], kw["encoder_mlp_quantities"],
                                       kw["use_mish"], mode)
            sws = torch.empty(stem.workspace_bytes(sdims), dtype=torch.uint8, device=dev)
            bws = torch.empty(encoder.workspace_bytes(bdims), dtype=torch.uint8, device=dev)
            g = torch.Generator(device=dev).manual_seed(1)
            x0 = torch.empty((B, d.tokens, d.d), device=dev)
            dx = torch.randn((B, d.tokens, d.d), generator=g, device=dev) * 1e-3
            sout = (x0, [torch.empty_like(t) for t in sw])
            bout = (torch.empty_like(x0), [torch.empty_like(t) for t in bw], torch.empty_like(x0))
            stem.run(images, sw, sdims, ws=sws, out=sout)
            calls = {
                "gradients": lambda: model.gradients(images, y),
                "stem_forward": lambda: stem.run(images, sw, sdims, ws=sws, out=sout),
                "stem_backward": lambda: stem.run(images, sw, sdims, dx0=dx, want_x0=False,
                                                  ws=sws, out=sout),
                "block_forward": lambda: encoder.run(x0, bw, bdims, ws=bws, out=bout),
                "block_forward_backward": lambda: encoder.run(x0, bw, bdims, dy=dx, want_y=False,
                                                              ws=bws, out=bout),
                "head_pass": lambda: model.head_gradients(None, y, encoded=x0),
            }
            for call in calls.values():
                for _ in range(a.warmup):
                    call()
            torch.cuda.synchronize()
            means = {n: [] for n in calls}
            for _ in range(a.rounds):
                for n, call in calls.items():
                    means[n].append(timed(call, a.reps))
            res = {n: {"ms_mean": float(np.mean(v)), "ms_min": min(v), "ms_max": max(v)}
                   for n, v in means.items()}
            parts = [means["stem_forward"][r] + means["stem_backward"][r] + means["head_pass"][r]
                     + reps_enc * (means["block_forward"][r] + means["block_forward_backward"][r])
                     for r in range(a.rounds)]
            res["sum_of_parts"] = {"ms_mean": float(np.mean(parts)), "ms_min": min(parts),
                                   "ms_max": max(parts)}
            rows_us = profiled_other_us(calls["stem_backward"], a.reps)
            R, dp = B * d.tokens, -(-d.d // 64) * 64
            moved = R * d.d * 4 + R * dp * (4 if mode == "bf16x3" else 2) + R * 4
            res["stem_grad_rows"] = {"us": rows_us, "bytes": moved, "GBps": moved / rows_us / 1e3}
            records.append({"preset": a.preset, "batch": B, "mode": mode, "reps": a.reps,
                            "rounds": a.rounds, "depth": reps_enc, "results": res})
            print(json.dumps(records[-1]), flush=True)
            del model, sws, bws, calls, images, x0, dx, sout, bout
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
