// LayerNorm backward (vtd.py:353-357, 375-379 differentiated; DESIGN.md "Encoder block
// backward"): dx, dgamma, dbeta from the forward's input rows, its (mean, rstd) and dy, all
// fp32.  HBM-bound: x and dy are read once, dx written once, the residual-path gradient
// `add` folded into the same pass.  Built without FMA contraction (csrc/Makefile): every
// operation below rounds once, which is what tests/ln_grad_oracle.py counts and restates.
//
//   xhat = (x - mean) rstd, gy = dy gamma
//   dx = rstd ((gy - mean_D(gy)) - xhat mean_D(gy xhat)) [+ add]
//   dgamma = sum_rows dy xhat, dbeta = sum_rows dy
//
// Column sums without atomics and without one workgroup waiting on another: the rows are cut
// into ln_bwd_ranges(rows) contiguous ranges of ln_bwd_range_rows(rows) rows, one workgroup
// each.  Wave w of the workgroup takes rows r0 + w, r0 + w + 4, ... and keeps the per-column
// sums of its rows in registers; the four waves add up through LDS in wave order; the
// workgroup writes one [2][D] plane; ln_bwd_reduce_kernel sums the planes in range order (16
// segments of consecutive ranges, each summed in order, then the segments in order).  Every
// count is a function of rows alone, so the same inputs give the same bits on any device.
#include "vtd_launch.h"

namespace vtd {

namespace {

constexpr int LB_MAX_RANGES = 1024;   // planes of partials at the most
constexpr int LB_SEGS = 16;           // segments of the plane sum (waves of the reduce workgroup)

// rows per range: a multiple of the 4 waves, at least 8, and at most LB_MAX_RANGES ranges
inline int64_t ln_bwd_range_rows(int64_t rows) {
  const int64_t q = (rows + 4 * LB_MAX_RANGES - 1) / (4 * LB_MAX_RANGES);
  return 4 * (q < 2 ? 2 : q);
}
inline int ln_bwd_ranges(int64_t rows) {
  const int64_t rpr = ln_bwd_range_rows(rows);
  return (int)((rows + rpr - 1) / rpr);
}

__device__ __forceinline__ f32x4 ldf4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stf4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// The waves' column sums -> one plane, in wave order: LDS holds the running sum, wave w adds its
// own to it ((w0 + w1) + w2) + w3; wave 3 returns the total.  Every wave of the workgroup calls
// it (three barriers).
template <int NV>
__device__ __forceinline__ void combine_waves(f32x4 (&ag)[NV], f32x4 (&ab)[NV], f32x4* sh, int wave,
                                              int lane) {
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (w > 0) {
          ag[i] = sh[i * 64 + lane] + ag[i];
          ab[i] = sh[(NV + i) * 64 + lane] + ab[i];
        }
        if (w < 3) {
          sh[i * 64 + lane] = ag[i];
          sh[(NV + i) * 64 + lane] = ab[i];
        }
      }
    }
    if (w < 3) __syncthreads();
  }
}

// One wave per row, lane l holding columns (i * 64 + l) * 4 .. + 3 of chunk i < NV, the
// forward's 4-column layout (layernorm_kernel): the row and its dy stay in registers between
// the two row means and the store.  ADD: dx += add (dx may alias add: each element is read and
// written by the same lane).  PARAM: the column sums for dgamma / dbeta into part[range][2][D].
template <int NV, bool ADD, bool PARAM>
__global__ __launch_bounds__(256) void ln_bwd_kernel(
    const float* __restrict__ x, int ldx, const float2* __restrict__ stat,
    const float* __restrict__ gamma, const float* __restrict__ dy, int lddy, const float* add,
    int ldadd, int64_t rows, int D, int rpr, float* dx, int lddx, float* __restrict__ part) {
  __shared__ f32x4 sh[PARAM ? 2 * NV * 64 : 1];
  constexpr bool EARLY = NV <= 4;       // add loaded with x and dy (wider rows: at the store)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rpr;
  const int64_t r1 = r0 + rpr < rows ? r0 + rpr : rows;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 g[NV], ag[NV], ab[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    g[i] = c < D ? ldf4(gamma + c) : zero;
    ag[i] = ab[i] = zero;
  }
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    const float* xr = x + row * ldx;
    const float* dyr = dy + row * lddy;
    const float* ar = ADD ? add + row * ldadd : nullptr;
    float* dxr = dx + row * lddx;
    f32x4 xh[NV], gy[NV], av[EARLY && ADD ? NV : 1];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      xh[i] = c < D ? ldf4(xr + c) : zero;
      gy[i] = c < D ? ldf4(dyr + c) : zero;
      if constexpr (EARLY && ADD) av[i] = c < D ? ldf4(ar + c) : zero;
    }
    const float2 st = stat[row];
    const float mean = st.x, rstd = st.y;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float h = (xh[i][j] - mean) * rstd;
          const float d = gy[i][j];
          if constexpr (PARAM) {
            ag[i][j] += d * h;
            ab[i][j] += d;
          }
          const float gg = d * g[i][j];
          s1 += gg;
          s2 += gg * h;
          xh[i][j] = h;
          gy[i][j] = gg;
        }
      }
    }
    const float m1 = wave_sum(s1) / D;
    const float m2 = wave_sum(s2) / D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rstd * ((gy[i][j] - m1) - xh[i][j] * m2);
        if constexpr (ADD) {
          const f32x4 a = EARLY ? av[EARLY ? i : 0] : ldf4(ar + c);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] += a[j];
        }
        stf4(dxr + c, o);
      }
    }
  }
  if constexpr (PARAM) {
    combine_waves<NV>(ag, ab, sh, wave, lane);
    if (wave == 3) {
      float* p = part + (int64_t)blockIdx.x * 2 * D;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) {
          stf4(p + c, ag[i]);
          stf4(p + D + c, ab[i]);
        }
      }
    }
  }
}

// generic fallback (D % 4 != 0, D > 4096, a misaligned base or a leading dimension that is no
// multiple of 4): one wave per row, the row read twice, as layernorm_generic_kernel reads it
template <bool ADD>
__global__ __launch_bounds__(256) void ln_bwd_generic_kernel(
    const float* __restrict__ x, int ldx, const float2* __restrict__ stat,
    const float* __restrict__ gamma, const float* __restrict__ dy, int lddy, const float* add,
    int ldadd, int64_t rows, int D, float* dx, int lddx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * ldx;
  const float* dyr = dy + row * lddy;
  const float mean = stat[row].x, rstd = stat[row].y;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float h = (xr[c] - mean) * rstd;
    const float gg = dyr[c] * gamma[c];
    s1 += gg;
    s2 += gg * h;
  }
  const float m1 = wave_sum(s1) / D;
  const float m2 = wave_sum(s2) / D;
  float* dxr = dx + row * lddx;
  for (int c = lane; c < D; c += 64) {
    const float h = (xr[c] - mean) * rstd;
    const float gg = dyr[c] * gamma[c];
    float o = rstd * ((gg - m1) - h * m2);
    if constexpr (ADD) o += add[row * ldadd + c];
    dxr[c] = o;
  }
}

// the generic path's column sums: lane = column, the same ranges, wave rows and wave order as
// ln_bwd_kernel, so both paths sum dgamma / dbeta in one order.  grid (ceil(D / 64), ranges)
__global__ __launch_bounds__(256) void ln_bwd_colsum_kernel(
    const float* __restrict__ x, int ldx, const float2* __restrict__ stat,
    const float* __restrict__ dy, int lddy, int64_t rows, int D, int rpr,
    float* __restrict__ part) {
  __shared__ float sh[2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * rpr;
  const int64_t r1 = r0 + rpr < rows ? r0 + rpr : rows;
  float ag = 0.f, ab = 0.f;
  if (c < D)
    for (int64_t row = r0 + wave; row < r1; row += 4) {
      const float2 st = stat[row];
      const float h = (x[row * ldx + c] - st.x) * st.y;
      const float d = dy[row * lddy + c];
      ag += d * h;
      ab += d;
    }
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      if (w > 0) {
        ag = sh[0][lane] + ag;
        ab = sh[1][lane] + ab;
      }
      if (w < 3) {
        sh[0][lane] = ag;
        sh[1][lane] = ab;
      }
    }
    if (w < 3) __syncthreads();
  }
  if (wave == 3 && c < D) {
    float* p = part + (int64_t)blockIdx.y * 2 * D;
    p[c] = ag;
    p[D + c] = ab;
  }
}

// dgamma | dbeta = the sum of the R planes in range order: wave s of the workgroup sums the
// planes of segment s (ceil(R / 16) consecutive ranges) in order, for 64 of the 2 D elements;
// wave 0 then adds the 16 segment sums in order.
__global__ __launch_bounds__(64 * LB_SEGS) void ln_bwd_reduce_kernel(
    const float* __restrict__ part, int R, int D, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  __shared__ float sh[LB_SEGS][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int seglen = (R + LB_SEGS - 1) / LB_SEGS;
  const int a = seg * seglen, b = a + seglen < R ? a + seglen : R;
  float s = 0.f;
  if (e < 2 * D) {
    const float* p = part + e;
#pragma unroll 8
    for (int r = a; r < b; ++r) s += p[(int64_t)r * 2 * D];
  }
  sh[seg][lane] = s;
  __syncthreads();
  if (seg == 0 && e < 2 * D) {
    float t = sh[0][lane];
#pragma unroll
    for (int k = 1; k < LB_SEGS; ++k) t += sh[k][lane];
    if (e < D) dgamma[e] = t;
    else dbeta[e - D] = t;
  }
}

template <int NV>
void ln_bwd_launch_nv(bool has_add, bool param, dim3 grid, hipStream_t st, const float* x, int ldx,
                      const float2* stat, const float* gamma, const float* dy, int lddy,
                      const float* add, int ldadd, int64_t rows, int D, int rpr, float* dx,
                      int lddx, float* part) {
#define VTD_LB(A, P) hipLaunchKernelGGL((ln_bwd_kernel<NV, A, P>), grid, dim3(256), 0, st, x, ldx, \
                                        stat, gamma, dy, lddy, add, ldadd, rows, D, rpr, dx, lddx, part)
  if (has_add && param) VTD_LB(true, true);
  else if (has_add) VTD_LB(true, false);
  else if (param) VTD_LB(false, true);
  else VTD_LB(false, false);
#undef VTD_LB
}

}  // namespace

int layernorm_backward_workspace_bytes(int64_t rows, int D, size_t* bytes) {
  VTD_CHECK_ARG(bytes, "layernorm_backward_workspace_bytes: null pointer");
  VTD_CHECK_ARG(rows > 0 && D > 0, "layernorm_backward_workspace_bytes: non-positive size");
  *bytes = (size_t)ln_bwd_ranges(rows) * 2 * (size_t)D * sizeof(float);
  return VTD_OK;
}

int layernorm_backward_launch(const float* x, int ldx, const float* stat, const float* gamma,
                              const float* dy, int lddy, const float* add, int ldadd,
                              int64_t rows, int D, float* dx, int lddx, float* dgamma,
                              float* dbeta, void* ws, size_t ws_bytes, hipStream_t st) {
  VTD_CHECK_ARG(x && stat && gamma && dy && dx, "layernorm_backward: null pointer");
  VTD_CHECK_ARG(rows > 0 && D > 0, "layernorm_backward: non-positive size");
  VTD_CHECK_ARG(ldx >= D && lddy >= D && lddx >= D && (!add || ldadd >= D),
                "layernorm_backward: leading dimension below D");
  VTD_CHECK_ARG((dgamma != nullptr) == (dbeta != nullptr),
                "layernorm_backward: dgamma and dbeta come together or not at all");
  auto mis = [](const void* p, int n) { return reinterpret_cast<uintptr_t>(p) % n != 0; };
  VTD_CHECK_ARG(!mis(stat, 8), "layernorm_backward: stat must be 8-byte aligned");
  VTD_CHECK_ARG(!mis(x, 4) && !mis(gamma, 4) && !mis(dy, 4) && !mis(add, 4) && !mis(dx, 4) &&
                    !mis(dgamma, 4) && !mis(dbeta, 4),
                "layernorm_backward: a pointer is not 4-byte aligned");
  const bool param = dgamma != nullptr;
  if (param) {
    size_t need = 0;
    if (int rc = layernorm_backward_workspace_bytes(rows, D, &need)) return rc;
    VTD_CHECK_ARG(ws, "layernorm_backward: null workspace");
    VTD_CHECK_ARG(!mis(ws, 16), "layernorm_backward: workspace must be 16-byte aligned");
    if (ws_bytes < need)
      return fail(VTD_ERR_WORKSPACE, "layernorm_backward: workspace smaller than "
                                     "vtd_layernorm_backward_workspace_bytes");
  }
  ProfScope ps(st, PROF_LN, 0.0);
  const float2* stat2 = reinterpret_cast<const float2*>(stat);
  float* part = static_cast<float*>(ws);
  const int rpr = (int)ln_bwd_range_rows(rows);
  const int R = ln_bwd_ranges(rows);
  const bool vec = D % 4 == 0 && D <= 4096 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 &&
                   (!add || ldadd % 4 == 0) && !mis(x, 16) && !mis(gamma, 16) && !mis(dy, 16) &&
                   !mis(add, 16) && !mis(dx, 16);
  if (vec) {
    const dim3 grid((unsigned)R);
    const int nv = (D + 255) / 256;
#define VTD_LBN(NV) ln_bwd_launch_nv<NV>(add != nullptr, param, grid, st, x, ldx, stat2, gamma, dy, \
                                         lddy, add, ldadd, rows, D, rpr, dx, lddx, part)
    if (nv <= 1) VTD_LBN(1);
    else if (nv <= 2) VTD_LBN(2);
    else if (nv <= 3) VTD_LBN(3);
    else if (nv <= 4) VTD_LBN(4);
    else if (nv <= 8) VTD_LBN(8);
    else VTD_LBN(16);
#undef VTD_LBN
    VTD_LAUNCH_CHECK("layernorm_backward");
  } else {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (add)
      hipLaunchKernelGGL((ln_bwd_generic_kernel<true>), grid, dim3(256), 0, st, x, ldx, stat2,
                         gamma, dy, lddy, add, ldadd, rows, D, dx, lddx);
    else
      hipLaunchKernelGGL((ln_bwd_generic_kernel<false>), grid, dim3(256), 0, st, x, ldx, stat2,
                         gamma, dy, lddy, add, ldadd, rows, D, dx, lddx);
    VTD_LAUNCH_CHECK("layernorm_backward");
    if (param) {
      hipLaunchKernelGGL(ln_bwd_colsum_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)R),
                         dim3(256), 0, st, x, ldx, stat2, dy, lddy, rows, D, rpr, part);
      VTD_LAUNCH_CHECK("layernorm_backward column sums");
    }
  }
  if (param) {
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((unsigned)((2 * (int64_t)D + 63) / 64)),
                       dim3(64 * LB_SEGS), 0, st, part, R, D, dgamma, dbeta);
    VTD_LAUNCH_CHECK("layernorm_backward reduce");
  }
  return VTD_OK;
}

}  // namespace vtd

extern "C" {

int vtd_layernorm_backward_workspace_bytes(int64_t rows, int D, size_t* bytes) {
  return vtd::layernorm_backward_workspace_bytes(rows, D, bytes);
}

int vtd_layernorm_backward(const float* x_dev, int ldx, const float* stat_dev,
                           const float* gamma_dev, const float* dy_dev, int lddy,
                           const float* add_dev, int ldadd, int64_t rows, int D, float* dx_dev,
                           int lddx, float* dgamma_dev, float* dbeta_dev, void* ws_dev,
                           size_t ws_bytes, void* stream) {
  return vtd::layernorm_backward_launch(x_dev, ldx, stat_dev, gamma_dev, dy_dev, lddy, add_dev,
                                        ldadd, rows, D, dx_dev, lddx, dgamma_dev, dbeta_dev,
                                        ws_dev, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
