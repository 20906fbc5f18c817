"""Cost of the validation loss on the device (DESIGN.md "Validation loss"):
 1. us per vtd_loss launch at (256, 17) with from_logits=1, device events around 200
    launches after a warm-up; beside it vtd_decode + vtd_loss with from_logits=0;
 2. wall time of Model.evaluate over 4 batches of 256 at ViT-B/16 @224 in bf16 against four
    bare forward calls + four MeanAveragePrecision.update_state calls and one result read,
    alternating the two, several rounds.
Needs a HIP device; prints one JSON line."""
import argparse
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vision_transformer_detector_amd as vtd  # noqa: E402
from vision_transformer_detector_amd import loss as VL  # noqa: E402


def labels_and_logits(rng, batch, boxes=17):
    y = np.full((batch, boxes, 6), -8.0, np.float32)
    y[..., 0] = 0.0
    for b in range(batch):
        n = int(rng.integers(0, boxes + 1))
        y[b, :n, 0] = 1.0
        y[b, :n, 1] = rng.integers(0, 80, n)
        y[b, :n, 2:4] = rng.uniform(60, 548, (n, 2))
        y[b, :n, 4:6] = rng.uniform(8, 300, (n, 2))
    return y, rng.normal(0, 2, (batch, boxes, 6)).astype(np.float32)


def events_us(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    y, logits = labels_and_logits(rng, a.batch)
    yt, lg = torch.from_numpy(y).to(dev), torch.from_numpy(logits).to(dev)
    fused, plain = VL.loss_params(), VL.loss_params(use_transform_predictions=False)
    running = torch.zeros(2, dtype=torch.float64, device=dev)
    out = {"shape": [a.batch, 17], "launches": a.launches}
    # the binding's own calls (one output allocation per launch, as evaluate runs them)
    out["loss_from_logits_us"] = events_us(lambda: VL._launch(yt, lg, fused, running),
                                           a.launches, a.warmup)
    out["decode_plus_loss_us"] = events_us(
        lambda: VL._launch(yt, vtd.transform_predictions(lg), plain, running),
        a.launches, a.warmup)

    model = vtd.create_vision_transformer_detector(**vtd.presets.VIT_B16_224, dtype="bfloat16",
                                                   device=dev)
    n = a.batch * a.batches
    images = torch.from_numpy(rng.uniform(-1, 1, (n, 224, 224, 3)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(labels_and_logits(rng, n)[0]).to(dev)
    metric = vtd.MeanAveragePrecision(device=dev)
    model.compile(loss=functools.partial(vtd.my_custom_loss, coefficient=9, exponent=2,
                                         weight_ciou=4.5), metrics=[metric])

    def evaluate():
        return model.evaluate(images, labels, batch_size=a.batch)

    def bare():
        metric.reset_state()
        for i in range(0, n, a.batch):
            metric.update_state(labels[i:i + a.batch], model.forward(images[i:i + a.batch]))
        return metric.result().item()

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for fn in (evaluate, bare, evaluate, bare):          # warm-up: workspace, code objects
        fn()
    ev, ba = [], []
    for _ in range(a.rounds):
        ev.append(wall(evaluate))
        ba.append(wall(bare))
    # the two are timed back to back in each round: the paired differences cancel the drift
    # between rounds that the two medians keep
    paired = sorted((e - b) * 1e3 for e, b in zip(ev, ba))
    out.update(rounds=a.rounds, evaluate_min_ms=min(ev), bare_min_ms=min(ba),
               evaluate_median_ms=float(np.median(ev)), bare_median_ms=float(np.median(ba)),
               evaluate_spread_ms=[min(ev), max(ev)], bare_spread_ms=[min(ba), max(ba)],
               paired_difference_median_us=float(np.median(paired)),
               paired_difference_quartiles_us=[paired[len(paired) // 4],
                                               paired[(3 * len(paired)) // 4]],
               loss_launches_us=a.batches * out["loss_from_logits_us"],
               evaluate_result=evaluate(), bare_ap=bare())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
