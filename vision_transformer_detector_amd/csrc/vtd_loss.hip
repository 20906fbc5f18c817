// Validation loss on the device: ciou_calculator / diagonal_calculator
// (vision_transformer_detector.py:878-1015) and my_custom_loss (vtd.py:1122-1265).
//
// B x boxes slots (256 x 17 = 4,352 at the bench batch) of a few dozen flops and ten
// transcendentals each: the launch is latency-bound, so ONE workgroup (1024 threads, the
// most a workgroup holds: 4.25 trips over the bench batch) strides over the slots.  Every
// per-slot value is float32 arithmetic in the reference's operation order.  The file is
// compiled like vtd_elementwise.hip (-ffp-contract=fast) so that the inlined
// decode_transform gives vtd_decode's bits -- expf expands differently with contraction
// off -- and that mode ignores contraction pragmas, so every product that feeds an add or
// a subtract goes through rounded() (vtd_box.h) and no FMA can replace the reference's two
// roundings.  The three sums are accumulated in fp64 in a fixed order -- thread t takes
// slots t, t + 1024, ... in ascending order, the 64 lanes of a wave combine in a fixed
// butterfly, thread 0 adds the 16 wave partials in wave order -- with no float atomics and
// no dependence on a grid size, so a result is bit-identical from run to run.
// The gradient kernels (loss_grad_kernel, ciou_grad_kernel, decode_grad_kernel) follow the
// same rules; their per-slot derivatives are in vtd_box_grad.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "vtd_box.h"
#include "vtd_box_grad.h"
#include "vtd_common.h"

namespace vtd {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;

// ciou_calculator for one pair of (x, y, h, w) boxes (vtd.py:946-1015); returns the CIoU
// loss and stores the DIoU (the get_diou=True result) and diagonal_calculator's length.
__device__ __forceinline__ float ciou_one(const float* l, const float* p, float* diou,
                                          float* diag) {
  const float lx = l[0], ly = l[1], lh = l[2], lw = l[3];
  const float px = p[0], py = p[1], ph = p[2], pw = p[3];
  const float iou = iou_one(lx, ly, lh, lw, px, py, ph, pw);
  // rho: reduce_euclidean_norm of the centre deltas (vtd.py:969-971)
  const float dx = lx - px, dy = ly - py;
  const float rho = sqrtf(rounded(dx * dx) + rounded(dy * dy));
  // diagonal_calculator (vtd.py:899-941): the sorted edges' last - first = max - min
  const float ll = lx - lw / 2.f, lr = lx + lw / 2.f;
  const float pl = px - pw / 2.f, pr = px + pw / 2.f;
  const float lt = ly - lh / 2.f, lb = ly + lh / 2.f;
  const float pt = py - ph / 2.f, pb = py + ph / 2.f;
  const float eh = fmaxf(fmaxf(lt, lb), fmaxf(pt, pb)) - fminf(fminf(lt, lb), fminf(pt, pb));
  const float ew = fmaxf(fmaxf(ll, lr), fmaxf(pl, pr)) - fminf(fminf(ll, lr), fminf(pl, pr));
  const float c = sqrtf(rounded(eh * eh) + rounded(ew * ew));
  const float q = rho / (c + 1e-8f);
  const float r_diou = rounded(q * q);
  const float al = atanf(lw / (lh + 1e-8f));
  const float ap = atanf(pw / (ph + 1e-8f));
  // tf.square(np.pi) squares the float32 pi (vtd.py:992-994)
  constexpr float kPi = 3.14159265358979323846f;
  constexpr float kPiSq = kPi * kPi;
  const float da = al - ap;
  const float v = ((da * da) * 4.f) / kPiSq;
  const float alpha = v / (((1.f - iou) + v) + 1e-8f);
  const float r_ciou = r_diou + rounded(alpha * v);
  *diou = iou - r_diou;
  *diag = c;
  return (1.f - iou) + r_ciou;
}

// what: 0 = the CIoU loss, 1 = the DIoU, 2 = the enclosing box's diagonal
__global__ void ciou_kernel(const float* __restrict__ lab, const float* __restrict__ pred,
                            int64_t n, int stride, int what, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float diou, diag;
    const float loss = ciou_one(lab + i * stride + stride - 4, pred + i * stride + stride - 4,
                                &diou, &diag);
    out[i] = what == 2 ? diag : (what == 1 ? diou : loss);
  }
}

__device__ __forceinline__ double wave_sum_f64(double s) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// One slot of my_custom_loss (vtd.py:1122-1265): the objectness term, and for a positive slot
// the class and box terms and the decoded prediction.  Shared by loss_kernel and
// loss_grad_kernel, so both sum the same float32 bits.
struct SlotLoss {
  float p;             // the (decoded) objectness
  float bce, cls, box; // the three terms; cls and box only when positive
  float d[5];          // the (decoded) class and box, only when positive
  bool positive;
};
template <bool kLogits>
__device__ __forceinline__ SlotLoss slot_loss(const float* yt, const float* yp,
                                              const vtd_loss_params& prm) {
  SlotLoss r;
  // objectness: Keras binary cross-entropy, focal form with gamma 2 [upstream]
  const float y = yt[0];
  const float p = kLogits ? rounded(decode_transform(0, yp[0])) : yp[0];
  const float pc = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
  float bce = rounded(y * logf(pc + 1e-7f));
  bce = bce + rounded((1.f - y) * logf((1.f - pc) + 1e-7f));
  bce = -bce;
  if (prm.focal_binary_loss) {
    const float pt = rounded(y * p) + rounded((1.f - y) * (1.f - p));
    const float f = 1.f - pt;
    bce = (f * f) * bce;
  }
  r.p = p;
  r.bce = bce;
  // only positive slots reach the class and box terms: an empty row's -8 padding never
  // meets an atan or a division (vtd.py:1198-1247)
  r.positive = isclose(y, 1.f);
  if (!r.positive) return r;
#pragma unroll
  for (int f = 1; f < 6; ++f)
    r.d[f - 1] = kLogits ? rounded(decode_transform(f, yp[f])) : yp[f];
  const float ce = prm.coefficient * fabsf(r.d[0] - yt[1]);
  r.cls = prm.exponent == 2.f ? rounded(ce * ce) : powf(ce, prm.exponent);
  float diou, diag;
  r.box = ciou_one(yt + 2, r.d + 1, &diou, &diag);
  return r;
}

// The four fp64 sums of one workgroup in the fixed order (file comment); thread 0 then
// writes out[5] and returns the number of positive slots (other threads: unspecified).
__device__ __forceinline__ double loss_finish(double s_obj, double s_cls, double s_box,
                                              double s_cnt, int64_t n, int B,
                                              const vtd_loss_params& prm,
                                              float* __restrict__ out,
                                              double* __restrict__ running) {
  __shared__ double part[kWaves][4];
  s_obj = wave_sum_f64(s_obj);
  s_cls = wave_sum_f64(s_cls);
  s_box = wave_sum_f64(s_box);
  s_cnt = wave_sum_f64(s_cnt);
  if ((threadIdx.x & 63) == 0) {
    double* w = part[threadIdx.x >> 6];
    w[0] = s_obj; w[1] = s_cls; w[2] = s_box; w[3] = s_cnt;
  }
  __syncthreads();
  if (threadIdx.x != 0) return 0.0;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < kWaves; ++w)
    for (int k = 0; k < 4; ++k) t[k] += part[w][k];
  const float obj = (float)(t[0] / (double)n);
  const float cls = t[3] > 0.0 ? (float)(t[1] / t[3]) : 0.f;     // vtd.py:1249-1251
  const float box = t[3] > 0.0 ? (float)(t[2] / t[3]) : 0.f;
  const float total = (obj + rounded(cls * prm.weight_classification)) +
                      rounded(box * prm.weight_ciou);
  out[0] = total;
  out[1] = obj;
  out[2] = cls;
  out[3] = box;
  out[4] = (float)t[3];
  if (running) {           // the Keras loss metric: batch-size weighted mean [upstream]
    running[0] += (double)total * (double)B;
    running[1] += (double)B;
  }
  return t[3];
}

// my_custom_loss (vtd.py:1122-1265) over n = B * boxes slots of 6 floats.
template <bool kLogits>
__global__ __launch_bounds__(kThreads) void loss_kernel(const float* __restrict__ y_true,
                                                        const float* __restrict__ y_pred,
                                                        int64_t n, int B, vtd_loss_params prm,
                                                        float* __restrict__ out,
                                                        double* __restrict__ running) {
  double s_obj = 0.0, s_cls = 0.0, s_box = 0.0, s_cnt = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const SlotLoss r = slot_loss<kLogits>(y_true + i * 6, y_pred + i * 6, prm);
    s_obj += (double)r.bce;
    if (!r.positive) continue;
    s_cls += (double)r.cls;
    s_box += (double)r.box;
    s_cnt += 1.0;
  }
  loss_finish(s_obj, s_cls, s_box, s_cnt, n, B, prm, out, running);
}

// d transform_predictions / d logit in column f: scale_f s (1 - s) with s the decode's own
// sigmoid bits (decode_transform's first line).  The [0, 1] clip never closes on a sigmoid,
// and s (1 - s) is exactly 0 where the float32 sigmoid saturates to 1.
__device__ __forceinline__ float decode_slope(int f, float v) {
  const float s = 1.f / (1.f + expf(-v));
  return (s * (1.f - s)) * (f == 0 ? 1.f : (f == 1 ? 79.f : 608.f));
}

// my_custom_loss and d total / d y_pred in one launch.  The loop is loss_kernel's (the same
// out[5] bits) and also writes each slot's six derivatives UNSCALED: d term / d prediction,
// times the decode's slope (kLogits).  After the reduction thread 0 broadcasts the positive
// count through LDS and every thread rescales the slots it wrote itself (the same
// thread-to-slot assignment, so a thread only reads back its own stores) by 1 / n
// (objectness) or weight / positives (class, box) and *upstream (NULL = 1).  One writer per
// element, no atomics.
template <bool kLogits>
__global__ __launch_bounds__(kThreads) void loss_grad_kernel(
    const float* __restrict__ y_true, const float* __restrict__ y_pred, int64_t n, int B,
    vtd_loss_params prm, const float* __restrict__ upstream, float* __restrict__ out,
    float* grad) {
  double s_obj = 0.0, s_cls = 0.0, s_box = 0.0, s_cnt = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const float* yt = y_true + i * 6;
    const float* yp = y_pred + i * 6;
    float* g = grad + i * 6;
    const SlotLoss r = slot_loss<kLogits>(yt, yp, prm);
    s_obj += (double)r.bce;
    float g0 = objectness_grad(yt[0], r.p, prm.focal_binary_loss != 0);
    if (kLogits) g0 *= decode_slope(0, yp[0]);
    g[0] = g0;
    if (!r.positive) {
#pragma unroll
      for (int f = 1; f < 6; ++f) g[f] = 0.f;
      continue;
    }
    s_cls += (double)r.cls;
    s_box += (double)r.box;
    s_cnt += 1.0;
    float gb[4];
    float g1 = class_grad(r.d[0] - yt[1], prm.coefficient, prm.exponent);
    ciou_grad_one(yt + 2, r.d + 1, false, gb);
    if (kLogits) g1 *= decode_slope(1, yp[1]);
    g[1] = g1;
#pragma unroll
    for (int f = 0; f < 4; ++f)
      g[f + 2] = kLogits ? gb[f] * decode_slope(f + 2, yp[f + 2]) : gb[f];
  }
  __shared__ double positives;
  const double cnt0 = loss_finish(s_obj, s_cls, s_box, s_cnt, n, B, prm, out, nullptr);
  if (threadIdx.x == 0) positives = cnt0;
  __syncthreads();
  const double cnt = positives;
  const double up = upstream ? (double)*upstream : 1.0;
  const float k_obj = (float)(up / (double)n);
  const float k_cls = cnt > 0.0 ? (float)(up * (double)prm.weight_classification / cnt) : 0.f;
  const float k_box = cnt > 0.0 ? (float)(up * (double)prm.weight_ciou / cnt) : 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    float* g = grad + i * 6;
    g[0] *= k_obj;
    if (!isclose(y_true[i * 6], 1.f)) continue;       // channels 1..5 stay exactly 0
    g[1] *= k_cls;
#pragma unroll
    for (int f = 2; f < 6; ++f) g[f] *= k_box;
  }
}

// d ciou_calculator / d prediction, elementwise: grad[i][stride], the leading stride - 4
// channels 0, the last four times upstream[i] (NULL = 1).
__global__ void ciou_grad_kernel(const float* __restrict__ lab, const float* __restrict__ pred,
                                 int64_t n, int stride, int get_diou,
                                 const float* __restrict__ upstream, float* __restrict__ grad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float g[4];
    ciou_grad_one(lab + i * stride + stride - 4, pred + i * stride + stride - 4, get_diou != 0, g);
    const float up = upstream ? upstream[i] : 1.f;
    float* o = grad + i * stride;
    for (int k = 0; k < stride - 4; ++k) o[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[stride - 4 + k] = g[k] * up;
  }
}

// d vtd_decode: grad[i] = upstream[i] * scale_f s (1 - s) over n rows of 6 logits
__global__ void decode_grad_kernel(const float* __restrict__ logits,
                                   const float* __restrict__ upstream, int64_t n,
                                   float* __restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6) return;
  grad[i] = upstream[i] * decode_slope((int)(i % 6), logits[i]);
}

}  // namespace
}  // namespace vtd

using namespace vtd;

static int ciou_launch(const char* name, const float* label_bbox, const float* pred_bbox,
                       int64_t n, int stride, int what, float* out, void* stream) {
  VTD_CHECK_ARG(n >= 0 && stride >= 4, std::string(name) + ": n >= 0 and stride >= 4 required");
  if (n == 0) return VTD_OK;
  VTD_CHECK_ARG(label_bbox && pred_bbox && out, std::string(name) + ": null pointer");
  ProfScope ps((hipStream_t)stream, PROF_OTHER, 0.0);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(ciou_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, label_bbox,
                     pred_bbox, n, stride, what, out);
  VTD_LAUNCH_CHECK(name);
  return VTD_OK;
}

extern "C" int vtd_ciou(const float* label_bbox, const float* pred_bbox, int64_t n, int stride,
                        int get_diou, float* out, void* stream) {
  return ciou_launch("vtd_ciou", label_bbox, pred_bbox, n, stride, get_diou ? 1 : 0, out, stream);
}

extern "C" int vtd_diagonal(const float* label_bbox, const float* pred_bbox, int64_t n,
                            int stride, float* out, void* stream) {
  return ciou_launch("vtd_diagonal", label_bbox, pred_bbox, n, stride, 2, out, stream);
}

extern "C" int vtd_loss(const float* y_true, const float* y_pred, int B, int boxes,
                        const vtd_loss_params* p, float* out, double* running, void* stream) {
  VTD_CHECK_ARG(p, "vtd_loss: null params");
  VTD_CHECK_ARG(out, "vtd_loss: null output pointer");
  VTD_CHECK_ARG(B >= 0, "vtd_loss: B must be >= 0");
  VTD_CHECK_ARG(boxes >= 1, "vtd_loss: boxes per image must be >= 1");
  VTD_CHECK_ARG(std::isfinite(p->coefficient) && p->coefficient >= 0.f,
                "vtd_loss: coefficient must be finite and >= 0");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    VTD_HIP(hipMemsetAsync(out, 0, 5 * sizeof(float), s));
    return VTD_OK;
  }
  VTD_CHECK_ARG(y_true && y_pred, "vtd_loss: null input pointer");
  ProfScope ps(s, PROF_OTHER, 0.0);
  const int64_t n = (int64_t)B * boxes;
  if (p->from_logits)
    hipLaunchKernelGGL(loss_kernel<true>, dim3(1), dim3(kThreads), 0, s, y_true, y_pred, n, B,
                       *p, out, running);
  else
    hipLaunchKernelGGL(loss_kernel<false>, dim3(1), dim3(kThreads), 0, s, y_true, y_pred, n, B,
                       *p, out, running);
  VTD_LAUNCH_CHECK("vtd_loss");
  return VTD_OK;
}

extern "C" int vtd_loss_grad(const float* y_true, const float* y_pred, int B, int boxes,
                             const vtd_loss_params* p, const float* upstream, float* out5,
                             float* grad, void* stream) {
  VTD_CHECK_ARG(p, "vtd_loss_grad: null params");
  VTD_CHECK_ARG(out5, "vtd_loss_grad: null output pointer");
  VTD_CHECK_ARG(B >= 0, "vtd_loss_grad: B must be >= 0");
  VTD_CHECK_ARG(boxes >= 1, "vtd_loss_grad: boxes per image must be >= 1");
  VTD_CHECK_ARG(std::isfinite(p->coefficient) && p->coefficient >= 0.f,
                "vtd_loss_grad: coefficient must be finite and >= 0");
  // below 1 the class derivative is unbounded at a zero class error
  VTD_CHECK_ARG(std::isfinite(p->exponent) && p->exponent >= 1.f,
                "vtd_loss_grad: exponent must be finite and >= 1");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    VTD_HIP(hipMemsetAsync(out5, 0, 5 * sizeof(float), s));
    return VTD_OK;
  }
  VTD_CHECK_ARG(y_true && y_pred, "vtd_loss_grad: null input pointer");
  VTD_CHECK_ARG(grad, "vtd_loss_grad: null gradient pointer");
  ProfScope ps(s, PROF_OTHER, 0.0);
  const int64_t n = (int64_t)B * boxes;
  if (p->from_logits)
    hipLaunchKernelGGL(loss_grad_kernel<true>, dim3(1), dim3(kThreads), 0, s, y_true, y_pred, n,
                       B, *p, upstream, out5, grad);
  else
    hipLaunchKernelGGL(loss_grad_kernel<false>, dim3(1), dim3(kThreads), 0, s, y_true, y_pred, n,
                       B, *p, upstream, out5, grad);
  VTD_LAUNCH_CHECK("vtd_loss_grad");
  return VTD_OK;
}

extern "C" int vtd_ciou_grad(const float* label_bbox, const float* pred_bbox, int64_t n,
                             int stride, int get_diou, const float* upstream, float* grad,
                             void* stream) {
  VTD_CHECK_ARG(n >= 0 && stride >= 4, "vtd_ciou_grad: n >= 0 and stride >= 4 required");
  if (n == 0) return VTD_OK;
  VTD_CHECK_ARG(label_bbox && pred_bbox && grad, "vtd_ciou_grad: null pointer");
  ProfScope ps((hipStream_t)stream, PROF_OTHER, 0.0);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(ciou_grad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     label_bbox, pred_bbox, n, stride, get_diou ? 1 : 0, upstream, grad);
  VTD_LAUNCH_CHECK("vtd_ciou_grad");
  return VTD_OK;
}

extern "C" int vtd_decode_grad(const float* logits, const float* upstream, int64_t n,
                               float* grad, void* stream) {
  VTD_CHECK_ARG(n >= 0, "vtd_decode_grad: n must be >= 0");
  if (n == 0) return VTD_OK;
  VTD_CHECK_ARG(logits && upstream && grad, "vtd_decode_grad: null pointer");
  // the grid's x extent is 32 bits
  VTD_CHECK_ARG(n <= (int64_t)0x7fffffff * 256 / 6, "vtd_decode_grad: n too large");
  ProfScope ps((hipStream_t)stream, PROF_OTHER, 0.0);
  const int64_t total = n * 6;
  hipLaunchKernelGGL(decode_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, logits, upstream, n, grad);
  VTD_LAUNCH_CHECK("vtd_decode_grad");
  return VTD_OK;
}
