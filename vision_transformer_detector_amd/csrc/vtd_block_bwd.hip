// The pieces of vtd_encoder_block_backward (vtd_train_runtime.hip) that no other kernel covers: the
// gather of the Keras attention kernels into the operand forms of the fused, per-head padded
// matrices, the un-gather of the fused gradients back into the Keras shapes, and the block's
// last step y = x1 + act(z).  All of them move at most a few MB per call (the last one a
// residual-stream pass), with plain loads and stores, one writer per element, no atomics.
#include <algorithm>

#include "vtd_launch.h"

namespace vtd {

namespace {

// Element (k, n) of the padded matrix Wp [Kp][Np] a BlockGather describes, 0 in every pad.
//   k -> group k / kgp, column k % kgp (valid below kg): source row (k / kgp) kg + k % kgp
//   n -> part n / part_np, then group and column as for k: source column of tensor `part`
__device__ __forceinline__ float gather_value(const BlockGather& g, int k, int n) {
  const int gk = k / g.kgp, ck = k - gk * g.kgp;
  const int ks = gk * g.kg + ck;
  const int part = n / g.part_np, r = n - part * g.part_np;
  const int gn = r / g.ngp, cn = r - gn * g.ngp;
  const int ns = gn * g.ng + cn;
  if (ck >= g.kg || ks >= g.K || part >= g.nparts || cn >= g.ng || ns >= g.N) return 0.f;
  // (selects, not an indexed array: a kernel argument indexed at run time goes to scratch)
  const float* s = part == 0 ? g.src[0] : part == 1 ? g.src[1] : g.src[2];
  return s[(int64_t)ks * g.N + ns];
}

// 8 values at columns c0 .. c0 + 7 of a B-operand row: bf16, or the split [hi | hi | lo] with
// P-wide pieces (the conversions of split_bf16x3_kernel role 1)
__device__ __forceinline__ void store_b8(const float (&v)[8], bf16_t* yr, int c0, int P, bool x3) {
  uint4 hi, lo;
  hi.x = pack_bf16x2(v[0], v[1]); lo.x = pack_lo_bf16x2(v[0], v[1], hi.x);
  hi.y = pack_bf16x2(v[2], v[3]); lo.y = pack_lo_bf16x2(v[2], v[3], hi.y);
  hi.z = pack_bf16x2(v[4], v[5]); lo.z = pack_lo_bf16x2(v[4], v[5], hi.z);
  hi.w = pack_bf16x2(v[6], v[7]); lo.w = pack_lo_bf16x2(v[6], v[7], hi.w);
  *reinterpret_cast<uint4*>(yr + c0) = hi;
  if (x3) {
    *reinterpret_cast<uint4*>(yr + P + c0) = hi;
    *reinterpret_cast<uint4*>(yr + 2 * P + c0) = lo;
  }
}

// Wp -> dst [Kp][ld], ld = Np (bf16) or 3 Np: the rows as stored, the Bt of an input-gradient
// GEMM.  One thread per 8 columns of a row: reads along n (the sources' contiguous axis),
// 16-B stores.  Np % 8 == 0.
__global__ __launch_bounds__(256) void block_gather_kn_kernel(BlockGather g, bf16_t* __restrict__ dst,
                                                              int x3) {
  const int chunks = g.Np / 8, ld = x3 ? 3 * g.Np : g.Np;
  const int64_t total = (int64_t)g.Kp * chunks;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / chunks), c0 = (int)(i - (int64_t)k * chunks) * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = gather_value(g, k, c0 + j);
    store_b8(v, dst + (int64_t)k * ld, c0, g.Np, x3 != 0);
  }
}

// Wp -> its transpose dst [Np][ld], ld = Kp or 3 Kp: the Bt of a forward GEMM.  64 x 64 tiles
// through LDS (Kp % 64 == Np % 64 == 0): reads along n, 4 B per lane; then a thread takes 8
// consecutive k of one n and stores 16 B per piece, the 8 threads of a column one 128-B run.
// float tile[64][65]: a wave writes one row (consecutive words: no conflict).  The 4-B reads
// (8 a + j, n0 + b) are served per 32-lane half on 32 banks: word (8 a + j) 65 + b, bank
// (8 a + b + j) mod 32 with a < 8 and four b, so a and a + 4 meet: 2-way.  Left so: 8 KiB of
// LDS reads per tile, off the hot path.
__global__ __launch_bounds__(256) void block_gather_t_kernel(BlockGather g, bf16_t* __restrict__ dst,
                                                             int x3, int tiles_k) {
  __shared__ float tile[64][65];
  const int k0 = (blockIdx.x % tiles_k) * 64, n0 = (blockIdx.x / tiles_k) * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) tile[r][tx] = gather_value(g, k0 + r, n0 + tx);
  __syncthreads();
  const int ld = x3 ? 3 * g.Kp : g.Kp;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int item = threadIdx.x + 256 * i, a = item & 7, b = item >> 3;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[8 * a + j][b];
    store_b8(v, dst + (int64_t)(n0 + b) * ld, k0 + 8 * a, g.Kp, x3 != 0);
  }
}

// the biases of a BlockGather (K = kg = kgp = 1) -> the padded fp32 vector [Np]
__global__ __launch_bounds__(256) void block_gather_bias_kernel(BlockGather g,
                                                                float* __restrict__ dst) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < g.Np) dst[n] = gather_value(g, 0, n);
}

// The inverse: the padded fp32 gradient W [Kp][ldw] (and vector b, nullable) -> the Keras-shaped
// tensors dst[part] [K][N] (dstb[part] [N]), pads dropped.  One thread per Keras element,
// consecutive threads along the Keras tensor's contiguous axis.
__global__ __launch_bounds__(256) void block_ungather_kernel(
    BlockGather g, float* __restrict__ d0, float* __restrict__ d1, float* __restrict__ d2,
    float* __restrict__ b0, float* __restrict__ b1, float* __restrict__ b2,
    const float* __restrict__ W, int ldw, const float* __restrict__ b) {
  const int64_t per = (int64_t)(g.K + (b ? 1 : 0)) * g.N, total = per * g.nparts;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int part = (int)(i / per);
    const int64_t e = i - part * per;
    const int ks = (int)(e / g.N), ns = (int)(e - (int64_t)ks * g.N);
    const int n = part * g.part_np + (ns / g.ng) * g.ngp + ns % g.ng;
    if (ks == g.K) {
      float* o = part == 0 ? b0 : part == 1 ? b1 : b2;
      o[ns] = b[n];
    } else {
      const int k = (ks / g.kg) * g.kgp + ks % g.kg;
      float* o = part == 0 ? d0 : part == 1 ? d1 : d2;
      o[e] = W[(int64_t)k * ldw + n];
    }
  }
}

// y = x1 + act(z), fp32: the block's output from the last MLP layer's kept pre-activation (the
// activation is the GEMM epilogue's own device function).  VEC: D % 4 == 0, every leading
// dimension a multiple of 4 and 16-B aligned bases.
template <bool VEC>
__global__ __launch_bounds__(256) void block_resid_act_kernel(const float* __restrict__ x1, int ldx,
                                                              const float* __restrict__ z, int ldz,
                                                              int64_t rows, int D, int act,
                                                              float* __restrict__ y, int ldy) {
  constexpr int V = VEC ? 4 : 1;
  const int chunks = D / V;
  const int64_t total = rows * chunks;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / chunks;
    const int c = (int)(i - m * chunks) * V;
    if constexpr (VEC) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x1 + m * ldx + c);
      const f32x4 zz = *reinterpret_cast<const f32x4*>(z + m * ldz + c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = a[j] + apply_act(act, zz[j]);
      *reinterpret_cast<f32x4*>(y + m * ldy + c) = o;
    } else {
      y[m * ldy + c] = x1[m * ldx + c] + apply_act(act, z[m * ldz + c]);
    }
  }
}

// y = x1 + drop(act(z)): the reference drops after the last MLP layer too, before the residual
// add.  One thread per 4 columns (one Philox block, vtd_philox.h); one fp32 multiply by inv_keep.
__global__ __launch_bounds__(256) void block_resid_act_drop_kernel(
    const float* __restrict__ x1, int ldx, const float* __restrict__ z, int ldz, int64_t rows,
    int D, int act, float* __restrict__ y, int ldy, DropKey dk) {
  const int chunks = (D + 3) / 4;
  const int64_t total = rows * chunks;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / chunks;
    const int cb = (int)(i - m * chunks);
    const uint32_t keep = drop_keep4_rows(dk, m, (uint32_t)cb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cb * 4 + j;
      if (c < D)
        y[m * ldy + c] = x1[m * ldx + c] +
                         ((keep >> j) & 1u ? apply_act(act, z[m * ldz + c]) * dk.inv_keep : 0.f);
    }
  }
}

int grid_of(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 16384); }

int gather_check(const char* what, const BlockGather& g) {
  VTD_CHECK_ARG(g.nparts >= 1 && g.nparts <= 3 && g.K > 0 && g.N > 0 && g.kg > 0 &&
                    g.kgp >= g.kg && g.ng > 0 && g.ngp >= g.ng && g.part_np > 0 && g.Kp > 0 &&
                    g.Np > 0,
                std::string(what) + ": bad geometry");
  for (int i = 0; i < g.nparts; ++i)
    VTD_CHECK_ARG(g.src[i], std::string(what) + ": null source");
  return VTD_OK;
}

}  // namespace

int block_gather_launch(const BlockGather& g, void* dst_t, void* dst_kn, int dtype,
                        hipStream_t st) {
  if (int rc = gather_check("block_gather", g)) return rc;
  VTD_CHECK_ARG(dtype == VTD_BF16 || dtype == VTD_BF16X3, "block_gather: bf16 or split-bf16");
  VTD_CHECK_ARG(g.Kp % 64 == 0 && g.Np % 64 == 0, "block_gather: Kp, Np must be multiples of 64");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(dst_t) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(dst_kn) % 16 == 0,
                "block_gather: destinations must be 16-byte aligned");
  const int x3 = dtype == VTD_BF16X3 ? 1 : 0;
  ProfScope ps(st, PROF_OTHER, 0.0);
  if (dst_t) {
    const int tiles_k = g.Kp / 64, tiles_n = g.Np / 64;
    hipLaunchKernelGGL(block_gather_t_kernel, dim3((unsigned)(tiles_k * tiles_n)), dim3(256), 0, st,
                       g, static_cast<bf16_t*>(dst_t), x3, tiles_k);
    VTD_LAUNCH_CHECK("block_gather (transposed)");
  }
  if (dst_kn) {
    hipLaunchKernelGGL(block_gather_kn_kernel, dim3(grid_of((int64_t)g.Kp * (g.Np / 8))),
                       dim3(256), 0, st, g, static_cast<bf16_t*>(dst_kn), x3);
    VTD_LAUNCH_CHECK("block_gather");
  }
  return VTD_OK;
}

int block_gather_bias_launch(const BlockGather& g, float* dst, hipStream_t st) {
  if (int rc = gather_check("block_gather_bias", g)) return rc;
  VTD_CHECK_ARG(dst && g.K == 1 && g.kg == 1 && g.kgp == 1, "block_gather_bias: bad arguments");
  ProfScope ps(st, PROF_OTHER, 0.0);
  hipLaunchKernelGGL(block_gather_bias_kernel, dim3((g.Np + 255) / 256), dim3(256), 0, st, g, dst);
  VTD_LAUNCH_CHECK("block_gather_bias");
  return VTD_OK;
}

int block_ungather_launch(const BlockGather& g, float* const* dst, float* const* dstb,
                          const float* W, int ldw, const float* b, hipStream_t st) {
  VTD_CHECK_ARG(g.nparts >= 1 && g.nparts <= 3 && g.K > 0 && g.N > 0 && g.kg > 0 &&
                    g.kgp >= g.kg && g.ng > 0 && g.ngp >= g.ng && g.part_np > 0 && W && dst &&
                    (!b || dstb),
                "block_ungather: bad arguments");
  // the last padded column read
  const int64_t nmax = (int64_t)(g.nparts - 1) * g.part_np + (int64_t)((g.N - 1) / g.ng) * g.ngp +
                       (g.N - 1) % g.ng;
  VTD_CHECK_ARG(ldw > nmax, "block_ungather: ldw too small");
  float* d[3] = {nullptr, nullptr, nullptr};
  float* db[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < g.nparts; ++i) {
    d[i] = dst[i];
    if (b) db[i] = dstb[i];
    VTD_CHECK_ARG(d[i] && (!b || db[i]), "block_ungather: null destination");
  }
  ProfScope ps(st, PROF_OTHER, 0.0);
  const int64_t total = (int64_t)(g.K + (b ? 1 : 0)) * g.N * g.nparts;
  hipLaunchKernelGGL(block_ungather_kernel, dim3(grid_of(total)), dim3(256), 0, st, g, d[0], d[1],
                     d[2], db[0], db[1], db[2], W, ldw, b);
  VTD_LAUNCH_CHECK("block_ungather");
  return VTD_OK;
}

int block_resid_act_launch(const float* x1, int ldx, const float* z, int ldz, int64_t rows, int D,
                           int act, float* y, int ldy, hipStream_t st, const DropKey* dk) {
  VTD_CHECK_ARG(x1 && z && y && rows > 0 && D > 0 && ldx >= D && ldz >= D && ldy >= D,
                "block_resid_act: bad arguments");
  VTD_CHECK_ARG(act >= VTD_ACT_NONE && act <= VTD_ACT_MISH, "block_resid_act: unknown activation");
  if (dk) {
    ProfScope ps(st, PROF_OTHER, 0.0);
    hipLaunchKernelGGL(block_resid_act_drop_kernel, dim3(grid_of(rows * ((D + 3) / 4))), dim3(256),
                       0, st, x1, ldx, z, ldz, rows, D, act, y, ldy, *dk);
    VTD_LAUNCH_CHECK("block_resid_act (dropout)");
    return VTD_OK;
  }
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && al16(x1) &&
                   al16(z) && al16(y);
  ProfScope ps(st, PROF_OTHER, 0.0);
  if (vec)
    hipLaunchKernelGGL(block_resid_act_kernel<true>, dim3(grid_of(rows * (D / 4))), dim3(256), 0,
                       st, x1, ldx, z, ldz, rows, D, act, y, ldy);
  else
    hipLaunchKernelGGL(block_resid_act_kernel<false>, dim3(grid_of(rows * D)), dim3(256), 0, st, x1,
                       ldx, z, ldz, rows, D, act, y, ldy);
  VTD_LAUNCH_CHECK("block_resid_act");
  return VTD_OK;
}

}  // namespace vtd
