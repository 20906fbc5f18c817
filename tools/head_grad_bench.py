"""Cost of the head backward on the device (DESIGN.md "Head backward"), at ViT-B/16 @224 (C2),
batch 256 by default, in both operand modes:
 1. vtd_head_backward end to end (training forward + backward) and its forward-only call,
    beside the inference forward's head section (Model.forward minus Model.encode), device
    events around `--calls` calls after a warm-up;
 2. vtd_gemm_wgrad per head layer shape at the msplit vtd_gemm_wgrad_choice picks, against
    torch.matmul(X.T, G) in bf16 on the same shapes (the yardstick), with the achieved FLOP/s
    and the share of the 2.5 PF bf16 MFMA peak (VTD_BF16X3 runs three products per logical
    one: its share counts the 3x);
 3. the msplit choice for head2 (8704 x 4352, M = B * 17) and Dense(17) (768 x 17, M = B *
    196) with one neighbour on each side.
Needs a HIP device; prints one JSON line."""
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

PEAK_BF16 = 2.5e15


def events_us(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def operand(x32, dtype):
    M, K = x32.shape
    P = -(-K // 64) * 64
    if dtype == L.BF16:
        op = torch.zeros((M, P), dtype=torch.bfloat16, device=x32.device)
        op[:, :K] = x32.to(torch.bfloat16)
        return op, P
    op = torch.empty((M, 2 * P), dtype=torch.bfloat16, device=x32.device)
    L.check(L.lib.vtd_split_bf16x3(x32.data_ptr(), M, K, K, op.data_ptr(), 2 * P, 0,
                                   L.stream_ptr()), "split")
    return op, 2 * P


def wgrad_case(M, K, N, dtype, msplits, calls, warmup, dev, with_torch):
    g = torch.Generator(device="cpu").manual_seed(K + N)
    x32 = torch.randn((M, K), generator=g).to(dev)
    g32 = (torch.randn((M, N), generator=g) * 0.05).to(dev)
    xop, ldx = operand(x32, dtype)
    gop, ldg = operand(g32, dtype)
    dW = torch.empty((K, N), dtype=torch.float32, device=dev)
    db = torch.empty((N,), dtype=torch.float32, device=dev)
    out = {"M": M, "K": K, "N": N, "choice": L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype), "us": {}}
    for ms in msplits:
        if not 1 <= ms <= min(-(-M // 32), 256):
            continue
        nbytes = ms * (K + 1) * N * 4 if ms > 1 else 0
        part = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)

        def run():
            L.check(L.lib.vtd_gemm_wgrad(M, K, N, xop.data_ptr(), ldx, gop.data_ptr(), ldg, dtype,
                                         dW.data_ptr(), N, db.data_ptr(), part.data_ptr(), nbytes,
                                         ms, L.stream_ptr()), "vtd_gemm_wgrad")
        out["us"][str(ms)] = events_us(run, calls, warmup)
    best = out["us"].get(str(out["choice"]))
    if best:
        products = 3 if dtype == L.BF16X3 else 1
        out["tflops_logical"] = 2.0 * M * K * N / best / 1e6
        out["share_of_bf16_peak"] = products * 2.0 * M * K * N / (best * 1e-6) / PEAK_BF16
    if with_torch:
        xb, gb = x32.to(torch.bfloat16), g32.to(torch.bfloat16)
        out["torch_matmul_bf16_us"] = events_us(lambda: torch.matmul(xb.T, gb), calls, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", default="vit_b16_224")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_grad_bench needs a HIP device")
    dev = torch.device("cuda:0")
    kw = vtd.presets.PRESETS[a.preset]
    rng = np.random.default_rng(0)
    out = {"preset": a.preset, "batch": a.batch, "calls": a.calls, "modes": {}}
    B = a.batch
    for mode, dtype in (("bfloat16", L.BF16), ("bf16x3", L.BF16X3)):
        model = vtd.create_vision_transformer_detector(**kw, dtype=mode, device=dev)
        model.compile(loss=functools.partial(vtd.my_custom_loss))
        d = model.dims
        images = torch.from_numpy(
            rng.uniform(-1, 1, (B, *model.input_shape)).astype(np.float32)).to(dev)
        y = np.full((B, 17, 6), -8.0, np.float32)
        y[..., 0] = 0.0
        y[:, :5, 0] = 1.0
        y[:, :5, 1] = rng.integers(0, 80, (B, 5))
        y[:, :5, 2:4] = rng.uniform(60, 548, (B, 5, 2))
        y[:, :5, 4:6] = rng.uniform(8, 300, (B, 5, 2))
        enc = model.encode(images)
        res = {}
        res["forward_us"] = events_us(lambda: model.forward(images), a.calls, a.warmup)
        res["encode_us"] = events_us(lambda: model.encode(images), a.calls, a.warmup)
        res["head_forward_section_us"] = res["forward_us"] - res["encode_us"]
        # head_gradients = forward-only call + vtd_loss_grad + the full call
        res["head_gradients_us"] = events_us(
            lambda: model.head_gradients(None, y, encoded=enc), a.calls, a.warmup)
        cfg = model.config(B)
        need = ctypes.c_size_t()
        L.check(L.lib.vtd_head_backward_workspace_bytes(ctypes.byref(cfg), ctypes.byref(need)), "ws")
        res["workspace_bytes"] = need.value
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        wdev = model._head_master()
        grads = {n: torch.empty_like(t) for n, t in wdev.items()}
        denc = torch.empty_like(enc)
        P, G = L.VtdHeadParams(), L.VtdHeadGrads()
        for S, src in ((P, wdev), (G, grads)):
            S.w_det, S.b_det = src["dense/kernel"].data_ptr(), src["dense/bias"].data_ptr()
            for j in range(d.n_head):
                S.w_head[j] = src[f"dense_{j + 1}/kernel"].data_ptr()
                S.b_head[j] = src[f"dense_{j + 1}/bias"].data_ptr()
            S.w_final = src["MLP_Head_no_Sigmoid/kernel"].data_ptr()
            S.b_final = src["MLP_Head_no_Sigmoid/bias"].data_ptr()
        G.d_encoded = denc.data_ptr()
        dl = torch.from_numpy(rng.normal(0, 1e-3, (B, 17, 6)).astype(np.float32)).to(dev)
        lg = torch.empty((B, 17, 6), dtype=torch.float32, device=dev)

        def call(dlogits):
            L.check(L.lib.vtd_head_backward(ctypes.byref(cfg), ctypes.byref(P), enc.data_ptr(),
                                            dlogits, lg.data_ptr(), ctypes.byref(G), ws.data_ptr(),
                                            ws.numel(), L.stream_ptr()), "vtd_head_backward")
        res["head_backward_us"] = events_us(lambda: call(dl.data_ptr()), a.calls, a.warmup)
        res["head_training_forward_us"] = events_us(lambda: call(None), a.calls, a.warmup)
        # the weight gradient per head shape
        HR, R = B * 17, B * d.tokens
        shapes = [("dense", R, d.d, 17)]
        k = d.tokens
        for j in range(d.n_head):
            shapes.append((f"dense_{j + 1}", HR, k, d.head_units[j]))
            k = d.head_units[j]
        shapes.append(("MLP_Head_no_Sigmoid", HR, k, 6))
        res["wgrad"] = {}
        for name, M, K, N in shapes:
            c = L.lib.vtd_gemm_wgrad_choice(M, K, N, dtype)
            sweep = {c}
            if name in ("dense", "dense_2"):
                sweep |= {max(1, c // 2), c * 2} if c > 1 else {2, 4}
            res["wgrad"][name] = wgrad_case(M, K, N, dtype, sorted(sweep), a.calls, a.warmup, dev,
                                            with_torch=True)
        out["modes"][mode] = res
        del model, ws, grads, wdev
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
