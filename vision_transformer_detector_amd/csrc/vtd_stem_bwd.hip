// vtd_stem_backward: the patch embedding (the reference's transformer_preprocessor,
// vtd.py:271-307) as a training forward and its backward.
//   x0[b N + n][j] = sum_k patches[b N + n][k] W[k][j] + bias[j] + pos[n]
// The forward is three launches that exist (vtd_extract_patches, transpose_op, one vtd_gemm with
// the bias and rowadd epilogue).  The backward is dW = patches^T dx0 and db = sum_rows dx0 (one
// vtd_gemm_wgrad) and dpos[n] = sum_b sum_j dx0[b N + n][j]; the two kernels here make the G
// operand of that product and the row sums in ONE pass over dx0, and reduce the row sums over
// the batch.  No atomics, one writer per element, every sum in a fixed order.
// vtd_stem_image_grad: d loss / d images = the adjoint of the extraction applied to dP = dx0 W^T
// (the same pass over dx0, the kernel in its Keras [K][N] form as Bt, one vtd_gemm, then
// stem_unpatch_kernel).
#include <algorithm>

#include "vtd_launch.h"

namespace vtd {

namespace {

// 8 fp32 values -> the operand form at columns c0 .. c0 + 7 of a row: bf16, or split-bf16
// [hi | lo] with P-wide pieces (the conversions of act_op_kernel, vtd_elementwise.hip)
__device__ __forceinline__ void store_g8(const float (&v)[8], bf16_t* yr, int c0, int P, bool x3) {
  uint4 hi, lo;
  hi.x = pack_bf16x2(v[0], v[1]); lo.x = pack_lo_bf16x2(v[0], v[1], hi.x);
  hi.y = pack_bf16x2(v[2], v[3]); lo.y = pack_lo_bf16x2(v[2], v[3], hi.y);
  hi.z = pack_bf16x2(v[4], v[5]); lo.z = pack_lo_bf16x2(v[4], v[5], hi.z);
  hi.w = pack_bf16x2(v[6], v[7]); lo.w = pack_lo_bf16x2(v[6], v[7], hi.w);
  *reinterpret_cast<uint4*>(yr + c0) = hi;
  if (x3) *reinterpret_cast<uint4*>(yr + P + c0) = lo;
}

// One wave per row m of dx0 fp32 [rows][D] (unpadded).  Lane l takes the 8-column chunks
// l, l + 64, ... of the P-wide output piece (P % 8 == 0, P >= D): it writes them in operand
// form, columns [D, P) as zero -- the row vtd_act_forward(VTD_ACT_NONE) writes -- and adds
// their values in column order into its own sum, which wave_sum then totals: rowsum[m].  Every
// add rounds once in fp32 (adding a pad's zero is exact).
// VEC: D % 4 == 0 and a 16-B aligned base, so every group of 4 columns lies wholly inside or
// outside the row and is one 16-B load.  The generic path loads the same values one by one:
// the same sums in the same order, the same bits.
template <bool VEC>
__global__ __launch_bounds__(256) void stem_grad_rows_kernel(const float* __restrict__ dx0,
                                                             int64_t rows, int D,
                                                             bf16_t* __restrict__ g, int ldg, int P,
                                                             int x3, float* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const int chunks = P / 8;
  for (int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); m < rows;
       m += (int64_t)gridDim.x * 4) {
    const float* xr = dx0 + m * D;
    bf16_t* gr = g + m * ldg;
    float s = 0.f;
    for (int ch = lane; ch < chunks; ch += 64) {
      const int c0 = ch * 8;
      float v[8];
      if constexpr (VEC) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (c0 < D) a = *reinterpret_cast<const f32x4*>(xr + c0);
        if (c0 + 4 < D) b = *reinterpret_cast<const f32x4*>(xr + c0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = a[j];
          v[4 + j] = b[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c0 + j < D ? xr[c0 + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
      store_g8(v, gr, c0, P, x3 != 0);
    }
    s = wave_sum(s);
    if (lane == 0) rowsum[m] = s;
  }
}

// dpos[n] = sum_b rowsum[b T + n]: one thread per token, b = 0 .. B - 1 in order; consecutive
// threads read consecutive floats.  The loads of 16 images are issued together and then added
// in order: the same sum, 16 times fewer memory round trips (one load per add took 79 us at
// B = 256, most of it latency).
__global__ __launch_bounds__(256) void stem_pos_reduce_kernel(const float* __restrict__ rowsum,
                                                              int B, int T,
                                                              float* __restrict__ dpos) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= T) return;
  const float* p = rowsum + n;
  float s = 0.f;
  int b = 0;
  for (; b + 16 <= B; b += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(int64_t)(b + j) * T];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; b < B; ++b) s += p[(int64_t)b * T];
  dpos[n] = s;
}

struct StemShape {
  int64_t rows;
  int B, H, W, C, p, D, Dp, T, P, Pp;
};
int stem_shape(const vtd_stem_dims* c, StemShape* s, const char* what) {
  const std::string w(what);
  VTD_CHECK_ARG(c, w + ": null dims");
  VTD_CHECK_ARG(c->batch > 0 && c->H > 0 && c->W > 0 && c->C > 0 && c->patch > 0 && c->d > 0,
                w + ": batch, H, W, C, patch, d must be > 0");
  if (c->dtype != VTD_BF16X3 && c->dtype != VTD_BF16)
    return fail(VTD_ERR_UNSUPPORTED, w + ": dims->dtype must be VTD_BF16X3 or VTD_BF16 (VTD_F32 "
                                         "and VTD_FP8 have no backward)");
  const int p = c->patch;
  const int64_t gh = ((int64_t)c->H + p - 1) / p, gw = ((int64_t)c->W + p - 1) / p;
  const int64_t T = gh * gw, P = (int64_t)p * p * c->C;
  VTD_CHECK_ARG(T < (int64_t)1 << 31 && (int64_t)c->batch * T < (int64_t)1 << 31,
                w + ": batch*tokens too large");
  VTD_CHECK_ARG(c->d < (1 << 24) && P < (1 << 24), w + ": d or patch*patch*C too large");
  s->rows = (int64_t)c->batch * T;
  s->B = c->batch; s->H = c->H; s->W = c->W; s->C = c->C; s->p = p; s->D = c->d;
  s->T = (int)T; s->P = (int)P;
  s->Dp = (int)round_up(s->D, VTD_KALIGN);
  s->Pp = (int)round_up(P, VTD_KALIGN);
  return VTD_OK;
}

// Workspace: buffers in use order, 256-B aligned.  `part`: the msplit partial planes of the
// weight gradient; gemm_wgrad_choice only grows with the rows, so the size is monotone in batch.
struct StemPlan {
  size_t patches, wt, gop, rowsum, part, part_bytes, total;
  int msplit;
};
StemPlan stem_plan(const StemShape& s, const Mode& m) {
  StemPlan p{};
  Arena ar;
  const size_t R = (size_t)s.rows;
  p.patches = ar.take(R * s.Pp * m.eop);
  p.wt = ar.take((size_t)s.Dp * m.kk(s.Pp) * 2);
  p.gop = ar.take(R * s.Dp * m.eop);
  p.rowsum = ar.take(R * 4);
  p.msplit = gemm_wgrad_choice((int)s.rows, s.P, s.D, m.op);
  p.part_bytes = p.msplit > 1 ? (size_t)p.msplit * (s.P + 1) * s.D * 4 : 0;
  p.part = ar.take(p.part_bytes);
  p.total = ar.off;
  return p;
}

int stem_grad_rows_launch(const float* dx0, int64_t rows, int D, void* g, int ldg, int P, bool x3,
                          float* rowsum, hipStream_t st) {
  const bool vec = D % 4 == 0 && reinterpret_cast<uintptr_t>(dx0) % 16 == 0;
  const int grid = (int)std::min<int64_t>((rows + 3) / 4, 65536);
  ProfScope ps(st, PROF_OTHER, 0.0);
  if (vec)
    hipLaunchKernelGGL(stem_grad_rows_kernel<true>, dim3(grid), dim3(256), 0, st, dx0, rows, D,
                       static_cast<bf16_t*>(g), ldg, P, x3 ? 1 : 0, rowsum);
  else
    hipLaunchKernelGGL(stem_grad_rows_kernel<false>, dim3(grid), dim3(256), 0, st, dx0, rows, D,
                       static_cast<bf16_t*>(g), ldg, P, x3 ? 1 : 0, rowsum);
  VTD_LAUNCH_CHECK("stem_grad_rows");
  return VTD_OK;
}

int stem_backward(const vtd_stem_dims* c, const vtd_stem_params* w, const float* images,
                  const float* dx0, float* x0, const vtd_stem_grads* g, void* ws_,
                  size_t ws_bytes, void* stream_) {
  StemShape s;
  if (int rc = stem_shape(c, &s, "stem_backward")) return rc;
  VTD_CHECK_ARG(w && images && ws_ && (dx0 ? g != nullptr : x0 != nullptr),
                "stem_backward: null pointer");
  VTD_CHECK_ARG(w->pos && w->w && w->b, "stem_backward: null weight pointer");
  if (dx0) VTD_CHECK_ARG(g->pos && g->w && g->b, "stem_backward: null gradient pointer");
  // the GEMM's epilogue reads the bias and writes x0 in 16-B vectors, the workspace holds
  // operand rows; everything else is read or written float by float
  auto al = [](const void* q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a == 0; };
  VTD_CHECK_ARG(al(ws_, 16) && al(x0, 16) && al(w->w, 16) && al(w->b, 16) && al(images, 4) &&
                    al(dx0, 4) && al(w->pos, 4) &&
                    (!dx0 || (al(g->pos, 4) && al(g->w, 4) && al(g->b, 4))),
                "stem_backward: misaligned pointer (workspace, x0, params->w, params->b: 16 "
                "bytes; every other array: 4)");
  const Mode m = mode_of(c->dtype);
  const StemPlan P = stem_plan(s, m);
  if (ws_bytes < P.total)
    return fail(VTD_ERR_WORKSPACE, "stem_backward: workspace too small (need " +
                                       std::to_string(P.total) + " bytes)");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(ws_);
  // the chain context (no padded bias, no input-gradient GEMM: no bias / wkn buffers)
  const Chain ch{st, ws, m, m.op, reinterpret_cast<float*>(ws + P.part), P.part_bytes, nullptr,
                 ws + P.wt, nullptr};
  const int R = (int)s.rows;
  void* patches = ws + P.patches;
  int rc;
  // ================= training forward
  if ((rc = patches_launch(images, s.B, s.H, s.W, s.C, s.p, patches, m.ka(s.Pp), m.op, st)))
    return rc;
  if (x0) {                            // (with dx0: only when the caller asks for x0)
    if ((rc = ch.conv_t(w->w, s.P, s.D, s.Pp, s.Dp))) return rc;
    vtd_epilogue e{};
    e.bias = w->b;
    e.rowadd = w->pos; e.rowadd_period = s.T; e.rowadd_ncols = s.D;
    e.act = VTD_ACT_NONE;
    e.out = x0; e.ldo = s.D; e.out_dtype = VTD_F32;
    if ((rc = ch.gemm(R, s.D, m.kk(s.Pp), patches, m.ka(s.Pp), ch.wt, 1, e,
                      2.0 * R * (double)s.P * s.D)))
      return rc;
  }
  if (!dx0) return VTD_OK;

  // ================= backward
  void* gop = ws + P.gop;
  float* rowsum = reinterpret_cast<float*>(ws + P.rowsum);
  if ((rc = stem_grad_rows_launch(dx0, s.rows, s.D, gop, m.ka(s.Dp), s.Dp, m.x3, rowsum, st)))
    return rc;
  if ((rc = ch.wgrad(R, s.P, s.D, patches, m.ka(s.Pp), gop, m.ka(s.Dp), g->w, s.D, g->b, P.msplit)))
    return rc;
  ProfScope ps(st, PROF_OTHER, 0.0);
  hipLaunchKernelGGL(stem_pos_reduce_kernel, dim3((unsigned)((s.T + 255) / 256)), dim3(256), 0, st,
                     rowsum, s.B, s.T, g->pos);
  VTD_LAUNCH_CHECK("stem_pos_reduce");
  return VTD_OK;
}

// ------------------------------------------------------------------ image gradient
// The adjoint of the SAME-padded patch extraction (patches_kernel, vtd_elementwise.hip): every
// image element was copied to exactly one patch column, so its gradient is that column of
//   dP fp32 [B T][ldp]:  dimg[b][y][x][c] = dP[b T + py gw + px][(ky p + kx) C + c],
//   py = (y + top) / p, ky = (y + top) % p, px = (x + left) / p, kx = (x + left) % p.
// One wave per image row (b, y): py and ky are the wave's, and along the row position
// i = x C + c the source is dP[b T + py gw + j / pC][ky pC + j % pC] with j = i + left C --
// runs of pC consecutive floats on both sides.  Lane l takes the positions l V, (l + 64) V, ...:
// consecutive lanes write consecutive addresses.  The pad columns of dP are never read, every
// element of dimg is written once, nothing else is.
// VEC (V = 4): W C, p C and left C are multiples of 4 and dimg is 16-B aligned (dP is, with
// ldp % 4 == 0), so every group of 4 positions lies inside one run and both sides are one
// aligned 16-B access.  The generic path (V = 1) moves the same values float by float.
template <bool VEC>
__global__ __launch_bounds__(256) void stem_unpatch_kernel(const float* __restrict__ dP, int ldp,
                                                           int64_t rows, int H, int64_t WC,
                                                           int pC, int p, int gw, int T, int top,
                                                           int64_t leftC,
                                                           float* __restrict__ dimg) {
  constexpr int V = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows;
       r += (int64_t)gridDim.x * 4) {
    const int64_t b = r / H;
    const int yy = (int)(r - b * H) + top;
    const int py = yy / p, ky = yy - py * p;
    const float* src = dP + (b * T + (int64_t)py * gw) * ldp + (int64_t)ky * pC;
    float* dst = dimg + r * WC;
    for (int64_t i = (int64_t)lane * V; i < WC; i += 64 * V) {
      const int64_t j = i + leftC, run = j / pC;
      const float* s = src + run * ldp + (j - run * pC);
      if constexpr (VEC)
        *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(s);
      else
        dst[i] = *s;
    }
  }
}

// Workspace of vtd_stem_image_grad: buffers in use order, 256-B aligned, each linear in the rows.
struct ImageGradPlan {
  size_t gop, rowsum, wkn, dp, total;
};
ImageGradPlan image_grad_plan(const StemShape& s, const Mode& m) {
  ImageGradPlan p{};
  Arena ar;
  const size_t R = (size_t)s.rows;
  p.gop = ar.take(R * s.Dp * m.eop);
  p.rowsum = ar.take(R * 4);                       // stem_grad_rows' second output: scratch here
  p.wkn = ar.take((size_t)s.Pp * m.kk(s.Dp) * 2);
  p.dp = ar.take(R * s.Pp * 4);
  p.total = ar.off;
  return p;
}

int stem_unpatch_launch(const float* dP, const StemShape& s, float* dimg, hipStream_t st) {
  const int64_t gh = ((int64_t)s.H + s.p - 1) / s.p, gw = ((int64_t)s.W + s.p - 1) / s.p;
  // pad_before = floor(pad / 2), as patches_launch splits it (pad < p)
  const int top = (int)(gh * s.p - s.H) / 2, left = (int)(gw * s.p - s.W) / 2;
  const int pC = s.p * s.C;
  const int64_t rows = (int64_t)s.B * s.H, WC = (int64_t)s.W * s.C, leftC = (int64_t)left * s.C;
  const bool vec = WC % 4 == 0 && pC % 4 == 0 && leftC % 4 == 0 && s.Pp % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(dimg) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(dP) % 16 == 0;
  const int grid = (int)std::min<int64_t>((rows + 3) / 4, 65536);
  ProfScope ps(st, PROF_OTHER, 0.0);
  if (vec)
    hipLaunchKernelGGL(stem_unpatch_kernel<true>, dim3(grid), dim3(256), 0, st, dP, s.Pp, rows,
                       s.H, WC, pC, s.p, (int)gw, s.T, top, leftC, dimg);
  else
    hipLaunchKernelGGL(stem_unpatch_kernel<false>, dim3(grid), dim3(256), 0, st, dP, s.Pp, rows,
                       s.H, WC, pC, s.p, (int)gw, s.T, top, leftC, dimg);
  VTD_LAUNCH_CHECK("stem_unpatch");
  return VTD_OK;
}

int stem_image_grad(const vtd_stem_dims* c, const float* w, const float* dx0, float* dimg,
                    void* ws_, size_t ws_bytes, void* stream_) {
  StemShape s;
  if (int rc = stem_shape(c, &s, "stem_image_grad")) return rc;
  VTD_CHECK_ARG(w && dx0 && dimg && ws_, "stem_image_grad: null pointer");
  // the workspace holds operand rows and dP, the kernel is converted in 16-B vectors; dx0 and
  // the images are read and written float by float where they are not 16-B aligned
  auto al = [](const void* q, uintptr_t a) { return reinterpret_cast<uintptr_t>(q) % a == 0; };
  VTD_CHECK_ARG(al(ws_, 16) && al(w, 16) && al(dx0, 4) && al(dimg, 4),
                "stem_image_grad: misaligned pointer (workspace, w: 16 bytes; dx0, dimages: 4)");
  const Mode m = mode_of(c->dtype);
  const ImageGradPlan P = image_grad_plan(s, m);
  if (ws_bytes < P.total)
    return fail(VTD_ERR_WORKSPACE, "stem_image_grad: workspace too small (need " +
                                       std::to_string(P.total) + " bytes)");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(ws_);
  // the chain context (one unsplit input-gradient GEMM: no partials, bias or W^T buffers)
  const Chain ch{st, ws, m, m.op, nullptr, 0, nullptr, nullptr, ws + P.wkn};
  const int R = (int)s.rows;
  void* gop = ws + P.gop;
  float* dP = reinterpret_cast<float*>(ws + P.dp);
  int rc;
  if ((rc = stem_grad_rows_launch(dx0, s.rows, s.D, gop, m.ka(s.Dp), s.Dp, m.x3,
                                  reinterpret_cast<float*>(ws + P.rowsum), st)))
    return rc;
  if ((rc = ch.conv_kn(w, s.P, s.D, s.Pp, s.Dp))) return rc;
  vtd_epilogue e{};
  e.act = VTD_ACT_NONE;
  e.out = dP; e.ldo = s.Pp; e.out_dtype = VTD_F32;
  if ((rc = ch.gemm(R, s.P, m.kk(s.Dp), gop, m.ka(s.Dp), ch.wkn, 1, e,
                    2.0 * R * (double)s.P * s.D)))
    return rc;
  return stem_unpatch_launch(dP, s, dimg, st);
}

}  // namespace

}  // namespace vtd

extern "C" {

int vtd_stem_backward_workspace_bytes(const vtd_stem_dims* dims, size_t* bytes) {
  VTD_CHECK_ARG(bytes, "null bytes pointer");
  vtd::StemShape s;
  if (int rc = vtd::stem_shape(dims, &s, "stem_backward_workspace_bytes")) return rc;
  *bytes = vtd::stem_plan(s, vtd::mode_of(dims->dtype)).total;
  return VTD_OK;
}

int vtd_stem_backward(const vtd_stem_dims* dims, const vtd_stem_params* params,
                      const float* images_dev, const float* dx0_dev, float* x0_dev,
                      const vtd_stem_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  return vtd::stem_backward(dims, params, images_dev, dx0_dev, x0_dev, grads, ws, ws_bytes,
                            stream);
}

int vtd_stem_image_grad_workspace_bytes(const vtd_stem_dims* dims, size_t* bytes) {
  VTD_CHECK_ARG(bytes, "null bytes pointer");
  vtd::StemShape s;
  if (int rc = vtd::stem_shape(dims, &s, "stem_image_grad_workspace_bytes")) return rc;
  *bytes = vtd::image_grad_plan(s, vtd::mode_of(dims->dtype)).total;
  return VTD_OK;
}

int vtd_stem_image_grad(const vtd_stem_dims* dims, const float* w_dev, const float* dx0_dev,
                        float* dimages_dev, void* ws, size_t ws_bytes, void* stream) {
  return vtd::stem_image_grad(dims, w_dev, dx0_dev, dimages_dev, ws, ws_bytes, stream);
}

}  // extern "C"
