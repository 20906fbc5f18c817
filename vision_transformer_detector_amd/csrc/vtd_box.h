// Box arithmetic shared by the metric (vtd_metrics.hip) and the loss (vtd_loss.hip): both
// restate the reference's float32 operation order and must read the same iou_one.
// vtd_metrics.hip is compiled with -ffp-contract=off; vtd_loss.hip cannot be (its fused
// decode must give vtd_decode's bits, and expf expands differently under -ffp-contract=fast,
// which also overrides the in-file pragma), so every product that feeds an add passes
// through rounded(): with contraction off it changes nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace vtd {

// The value as rounded to float32, opaque to the compiler: an empty asm statement the
// register passes through, so a product cannot be contracted into an FMA with the add or
// subtract that consumes it.
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// iou_calculator for one pair of (x, y, h, w) boxes (vtd.py:792-873).  For intersecting
// boxes the reference's "sort the 4 edges, take 2nd - 3rd" equals min(far) - max(near).
__device__ __forceinline__ float iou_one(float lx, float ly, float lh, float lw, float px,
                                         float py, float ph, float pw) {
#pragma clang fp contract(off)
  const float ll = lx - lw / 2.f, lr = lx + lw / 2.f;
  const float pl = px - pw / 2.f, pr = px + pw / 2.f;
  const float lt = ly - lh / 2.f, lb = ly + lh / 2.f;
  const float pt = py - ph / 2.f, pb = py + ph / 2.f;
  const bool cond = (ll < pr) && (lr > pl) && (lt < pb) && (lb > pt);
  const float ih = cond ? fminf(lb, pb) - fmaxf(lt, pt) : 0.f;
  const float iw = cond ? fminf(lr, pr) - fmaxf(ll, pl) : 0.f;
  const float inter = rounded(ih * iw);
  const float pa = rounded(pw * ph);
  const float la = rounded(lw * lh);
  const float uni = (pa + la) - inter;
  return inter / (uni + 1e-8f);
}

__device__ __forceinline__ bool isclose(float a, float b) {    // tf.experimental.numpy
#pragma clang fp contract(off)
  return fabsf(a - b) <= 1e-8f + 1e-5f * fabsf(b);
}

}  // namespace vtd
