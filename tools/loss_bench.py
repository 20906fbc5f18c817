"""Cost of the validation loss on the device (DESIGN.md "Validation loss"):
 1. us per vtd_loss launch at (256, 17) with from_logits=1, device events around 200
    launches after a warm-up; beside it vtd_decode + vtd_loss with from_logits=0, one
    vtd_loss_grad launch (the value and d loss / d logits), and forward + backward of the
    same loss written in torch operations on the device (what a user would write without
    the gradient kernel), all measured the same way;
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


def torch_ops_loss(y, logits, coefficient=4.0, exponent=2.0, weight_classification=0.0074,
                   weight_ciou=10.0):
    """my_custom_loss in torch operations on the device, masks instead of boolean indexing
    so that nothing synchronises; r_diou without the sqrt of the centre distance."""
    eps, keps = 1e-8, 1e-7
    scale = torch.tensor([1.0, 79.0, 608.0, 608.0, 608.0, 608.0], device=logits.device)
    d = torch.sigmoid(logits) * scale
    t, p = y[..., 0], d[..., 0]
    pc = torch.clamp(p, keps, 1 - keps)
    bce = -(t * torch.log(pc + keps) + (1 - t) * torch.log(1 - pc + keps))
    bce = torch.pow(1 - (t * p + (1 - t) * (1 - p)), 2) * bce
    pos = torch.isclose(t, torch.ones_like(t))
    count = pos.sum().clamp(min=1)
    cls = torch.pow(coefficient * torch.abs(d[..., 1] - y[..., 1]), exponent)
    lb = torch.where(pos[..., None], y[..., 2:], torch.ones_like(y[..., 2:]))
    pb = torch.where(pos[..., None], d[..., 2:], torch.ones_like(d[..., 2:]))
    hor = torch.stack([lb[..., 1] - lb[..., 2] / 2, lb[..., 1] + lb[..., 2] / 2,
                       pb[..., 1] - pb[..., 2] / 2, pb[..., 1] + pb[..., 2] / 2], -1)
    ver = torch.stack([lb[..., 0] - lb[..., 3] / 2, lb[..., 0] + lb[..., 3] / 2,
                       pb[..., 0] - pb[..., 3] / 2, pb[..., 0] + pb[..., 3] / 2], -1)
    cond = ((ver[..., 0] < ver[..., 3]) & (ver[..., 1] > ver[..., 2]) &
            (hor[..., 0] < hor[..., 3]) & (hor[..., 1] > hor[..., 2]))[..., None]
    hs = torch.sort(torch.where(cond, hor, torch.zeros_like(hor)), -1).values
    vs = torch.sort(torch.where(cond, ver, torch.zeros_like(ver)), -1).values
    inter = (hs[..., 2] - hs[..., 1]) * (vs[..., 2] - vs[..., 1])
    iou = inter / (pb[..., 3] * pb[..., 2] + lb[..., 3] * lb[..., 2] - inter + eps)
    ho, vo = torch.sort(hor, -1).values, torch.sort(ver, -1).values
    eh, ew = ho[..., 3] - ho[..., 0], vo[..., 3] - vo[..., 0]
    dx, dy = lb[..., 0] - pb[..., 0], lb[..., 1] - pb[..., 1]
    r_diou = (dx * dx + dy * dy) / torch.square(torch.sqrt(eh * eh + ew * ew) + eps)
    v = torch.square(torch.atan(lb[..., 3] / (lb[..., 2] + eps)) -
                     torch.atan(pb[..., 3] / (pb[..., 2] + eps))) * 4 / 9.869605
    ciou = 1 - iou + r_diou + v / ((1 - iou) + v + eps) * v
    return (bce.mean() + (cls * pos).sum() / count * weight_classification +
            (ciou * pos).sum() / count * weight_ciou)


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
    ap.add_argument("--loss-only", action="store_true", help="skip the Model.evaluate part")
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
    out["loss_grad_us"] = events_us(lambda: VL._launch_grad(yt, lg, fused), a.launches, a.warmup)
    leaf = lg.clone().requires_grad_()

    def torch_ops():
        leaf.grad = None
        torch_ops_loss(yt, leaf).backward()

    out["torch_ops_forward_backward_us"] = events_us(torch_ops, a.launches, a.warmup)
    ours, theirs = VL._launch_grad(yt, lg, fused), (torch_ops_loss(yt, leaf), leaf.grad)
    out["torch_ops_agreement"] = [abs(ours[0][0].item() - theirs[0].item()),
                                  (ours[1] - theirs[1]).abs().max().item()]
    if a.loss_only:
        print(json.dumps(out))
        return

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
