// Weight-gradient GEMM of the head backward: dW[k][n] = sum_m X[m][k] G[m][n] and
// db[n] = sum_m G[m][n].  Both operands are contraction-major -- the activation X exactly as
// the forward's producers store it, G = dZ as vtd_act_grad writes it -- so neither is
// transposed in memory: both are staged by LDS-DMA as bf16 images [m][128 columns] and both
// MFMA operands come from transposed LDS reads (ds_read_b64_tr_b16).
//
// One workgroup (4 waves, 2 x 2, each 64 x 64 of v_mfma_f32_32x32x16_bf16) owns a 128 (k) x
// 128 (n) output tile over one range of M; the grid is output tiles x msplit ranges.
// M-step = 32 rows: per operand piece one 8 KiB image of 256-B rows, two LDS stages.  The
// DMA's destination is lane-linear, so the image is swizzled on the SOURCE address: the
// 16-B chunk c of row r sits at chunk c ^ (((r & 3) << 2) | ((r >> 2) & 3)), which puts the
// 4 rows x 64 B that one 32-lane half of a transposed read touches on 64 distinct banks.
// VTD_BF16X3: the hi and lo pieces of X and G are four images per stage and three MFMA
// products (hi hi + lo hi + hi lo) run into the one accumulator.
// Rows beyond M: the DMA reads row M - 1 instead (in bounds) and the ragged last step's
// rows >= M are zeroed in LDS before they are read.  Columns beyond the piece width are
// redirected to the tile's first chunk and never stored.
// msplit > 1: every range writes its fp32 partial plane [K + 1][N] (row K = the db partial,
// summed from the G images by the workgroups of the first k-tile) and wgrad_reduce_kernel
// sums the planes in range order: no atomics, the same bits at every run.
#include <algorithm>

#include "vtd_launch.h"

namespace vtd {
namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(1))) const void gbl_cvoid_t;

constexpr int WG_TILE = 128;          // output tile edge (k and n)
constexpr int WG_MS = 32;             // rows of M per step
constexpr int WG_IMG = WG_MS * 256;   // one operand piece image, bytes
constexpr int WG_MAX_SPLIT = 256;

__device__ __forceinline__ int wg_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

template <bool X3>
__global__ __launch_bounds__(256) void wgrad_kernel(
    const bf16_t* __restrict__ X, int ldx, const bf16_t* __restrict__ G, int ldg, int M, int K,
    int N, int pwx, int pwg, float* __restrict__ out, int ldo, int64_t plane,
    float* __restrict__ dbout, int zero_to, int steps_total, int tiles_n) {
  constexpr int NIMG = X3 ? 4 : 2, STAGE = NIMG * WG_IMG, GIMG = X3 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x % tiles_n, kt = blockIdx.x / tiles_n;
  const int sp = blockIdx.y, nsp = gridDim.y;
  const int s0 = (int)((int64_t)sp * steps_total / nsp);
  const int s1 = (int)((int64_t)(sp + 1) * steps_total / nsp);
  const int k0 = kt * WG_TILE, n0 = nt * WG_TILE;
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(smem);

  // ---- DMA sources: wave w fills the 4-row groups 2 w and 2 w + 1 of every image
  int ld_row[2], xcol[2], gcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 4 * (wave * 2 + j) + (lane >> 4);
    const int ch = (lane & 15) ^ wg_swz(row);
    ld_row[j] = row;
    xcol[j] = k0 + 8 * ch + 8 <= pwx ? k0 + 8 * ch : k0;
    gcol[j] = n0 + 8 * ch + 8 <= pwg ? n0 + 8 * ch : n0;
  }
  auto issue = [&](int s, int stage) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = min(s * WG_MS + ld_row[j], M - 1);
      char* dst = smem + stage * STAGE + (wave * 2 + j) * 1024;
      const bf16_t* xs = X + (int64_t)m * ldx + xcol[j];
      const bf16_t* gs = G + (int64_t)m * ldg + gcol[j];
      __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)xs, (lds_void_t*)dst, 16, 0, 0);
      if constexpr (X3)
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)(xs + pwx), (lds_void_t*)(dst + WG_IMG), 16,
                                         0, 0);
      __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)gs, (lds_void_t*)(dst + GIMG * WG_IMG), 16, 0,
                                       0);
      if constexpr (X3)
        __builtin_amdgcn_global_load_lds((gbl_cvoid_t*)(gs + pwg),
                                         (lds_void_t*)(dst + 3 * WG_IMG), 16, 0, 0);
    }
  };

  // ---- transposed-read addresses: lane 4 q + p of a 16-lane group addresses
  // row q, columns 4 p .. 4 p + 3 of a 4-row x 16-column block and receives column (lane & 15).
  // 32x32x16 operand: lane l holds column l & 31 at the 8 contraction slots 8 (l >> 5) + 0..7:
  // groups 0 / 1 the columns 0..15 / 16..31 of rows 0..7, groups 2 / 3 of rows 8..15; read rd
  // takes rows 4 rd .. 4 rd + 3 of the eight.
  const int wk = wave >> 1, wn = wave & 1;
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  uint32_t offA[2][2], offB[2][2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int row = 8 * (grp >> 1) + 4 * rd + q;
    const int sw = wg_swz(row);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cha = 8 * wk + 4 * i + 2 * (grp & 1) + (p >> 1);
      const int chb = 8 * wn + 4 * i + 2 * (grp & 1) + (p >> 1);
      offA[i][rd] = 256 * row + 16 * (cha ^ sw) + 8 * (p & 1);
      offB[i][rd] = 256 * row + 16 * (chb ^ sw) + 8 * (p & 1);
    }
  }
  auto frag = [&](uint32_t img, const uint32_t (&off)[2], int ks) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_bf16x4*)(uintptr_t)(img + off[0] + ks * 4096));
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_bf16x4*)(uintptr_t)(img + off[1] + ks * 4096));
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // db: thread t sums column t & 127 over the rows 16 (t >> 7) + 0..15 of every step
  const bool want_db = dbout != nullptr && kt == 0;
  float dbs = 0.f;

  if (s0 < s1) issue(s0, 0);
  for (int s = s0; s < s1; ++s) {
    const int stage = (s - s0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMAs of the stage
    __syncthreads();                    // stage landed for every wave, the other stage is free
    if (s + 1 < s1) issue(s + 1, stage ^ 1);
    const int valid = M - s * WG_MS;    // ragged last step: rows >= valid contribute zero
    if (valid < WG_MS) {
      const int per = (WG_MS - valid) * 16;
      for (int e = tid; e < NIMG * per; e += 256) {
        const int img = e / per, r = e - img * per;
        *reinterpret_cast<uint4*>(smem + stage * STAGE + img * WG_IMG + valid * 256 + r * 16) =
            uint4{0u, 0u, 0u, 0u};
      }
      __syncthreads();
    }
    const uint32_t sx = lds_base + stage * STAGE, sg = sx + GIMG * WG_IMG;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ah[2], bh[2], al[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = frag(sx, offA[i], ks);
        bh[i] = frag(sg, offB[i], ks);
        if constexpr (X3) {
          al[i] = frag(sx + WG_IMG, offA[i], ks);
          bl[i] = frag(sg + WG_IMG, offB[i], ks);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          if constexpr (X3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          }
        }
    }
    if (want_db) {
      const int c = tid & 127, rb = 16 * (tid >> 7);
      const char* gi = smem + stage * STAGE + GIMG * WG_IMG;
#pragma unroll 4
      for (int r = rb; r < rb + 16; ++r) {
        const int o = 256 * r + 16 * ((c >> 3) ^ wg_swz(r)) + 2 * (c & 7);
        float v = bf16_to_f32(*reinterpret_cast<const bf16_t*>(gi + o));
        if constexpr (X3) v += bf16_to_f32(*reinterpret_cast<const bf16_t*>(gi + WG_IMG + o));
        dbs += v;
      }
    }
  }

  // ---- store: accumulator register r of lane l = row 8 (r >> 2) + 4 (l >> 5) + (r & 3),
  // column l & 31
  float* o = out + (int64_t)sp * plane;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + 64 * wn + 32 * j + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + 64 * wk + 32 * i + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (k < K && n < N) o[(int64_t)k * ldo + n] = acc[i][j][r];
      }
    }
  // the unsplit form writes dW itself: its pad columns [N, zero_to) as zero (last n-tile)
  if (zero_to > N && nt == tiles_n - 1) {
    const int w = zero_to - N, rows = min(WG_TILE, K - k0);
    for (int e = tid; e < rows * w; e += 256) o[(int64_t)(k0 + e / w) * ldo + N + e % w] = 0.f;
  }
  if (want_db) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    if (tid >= 128) red[tid - 128] = dbs;
    __syncthreads();
    if (tid < 128 && n0 + tid < N) dbout[(int64_t)sp * plane + n0 + tid] = dbs + red[tid];
  }
}

// dW[k][n] = sum of the planes' [k][n] in range order (n < N; columns [N, ldw) zero); the
// planes' row K -> db
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part,
                                                           int nsp, int K, int N,
                                                           float* __restrict__ dW, int ldw,
                                                           float* __restrict__ db) {
  const int64_t plane = (int64_t)(K + 1) * N, body = (int64_t)K * ldw;
  const int64_t total = body + (db ? N : 0);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const bool isdb = e >= body;
    const int64_t k = isdb ? K : e / ldw;
    const int n = isdb ? (int)(e - body) : (int)(e - k * ldw);
    float s = 0.f;
    if (n < N) {
      const float* ps = part + k * N + n;
      for (int i = 0; i < nsp; ++i) s += ps[i * plane];
    }
    if (isdb) db[n] = s;
    else dW[e] = s;
  }
}

int wgrad_steps(int M) { return (M + WG_MS - 1) / WG_MS; }

}  // namespace

// The split the head backward uses: enough ranges of M to put about two workgroups on every
// CU when the output has few tiles, each range at least 4 steps of 32 rows.
int gemm_wgrad_choice(int M, int K, int N, int dtype) {
  if ((dtype != VTD_BF16 && dtype != VTD_BF16X3) || M <= 0 || K <= 0 || N <= 0) return 1;
  const int64_t tiles = (int64_t)((K + WG_TILE - 1) / WG_TILE) * ((N + WG_TILE - 1) / WG_TILE);
  const int T = wgrad_steps(M);
  if (tiles >= 256) return 1;
  const int64_t want = (512 + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)T / 4, (int64_t)64}));
}

int gemm_wgrad_launch(int M, int K, int N, const void* X, int ldx, const void* G, int ldg,
                      int dtype, float* dW, int ldw, float* db, float* part, size_t part_bytes,
                      int msplit, hipStream_t st) {
  VTD_CHECK_ARG(X && G && dW, "gemm_wgrad: null pointer");
  VTD_CHECK_ARG(M > 0 && K > 0 && N > 0, "gemm_wgrad: M, K, N must be positive");
  if (dtype != VTD_BF16 && dtype != VTD_BF16X3)
    return fail(VTD_ERR_UNSUPPORTED, "gemm_wgrad: dtype must be VTD_BF16 or VTD_BF16X3");
  const bool x3 = dtype == VTD_BF16X3;
  VTD_CHECK_ARG(ldx % (x3 ? 16 : 8) == 0 && ldg % (x3 ? 16 : 8) == 0,
                "gemm_wgrad: ldx, ldg must be multiples of 8 (VTD_BF16X3: 16)");
  const int pwx = x3 ? ldx / 2 : ldx, pwg = x3 ? ldg / 2 : ldg;
  VTD_CHECK_ARG(pwx >= K && pwg >= N, "gemm_wgrad: ldx / ldg smaller than K / N (VTD_BF16X3: "
                                      "the piece width ld / 2)");
  VTD_CHECK_ARG(ldw >= N, "gemm_wgrad: ldw < N");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(X) % 16 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0,
                "gemm_wgrad: X, G must be 16-byte aligned");
  const int T = wgrad_steps(M);
  VTD_CHECK_ARG(msplit >= 1 && msplit <= T && msplit <= WG_MAX_SPLIT,
                "gemm_wgrad: msplit must be in [1, min(ceil(M / 32), 256)]");
  const size_t plane = (size_t)(K + 1) * N;
  if (msplit > 1) {
    VTD_CHECK_ARG(part, "gemm_wgrad: msplit > 1 needs part_dev");
    VTD_CHECK_ARG(part_bytes >= (size_t)msplit * plane * 4,
                  "gemm_wgrad: part_bytes < msplit * (K + 1) * N * 4");
  }
  const int tiles_n = (N + WG_TILE - 1) / WG_TILE, tiles_k = (K + WG_TILE - 1) / WG_TILE;
  VTD_CHECK_ARG((int64_t)tiles_n * tiles_k < (int64_t)1 << 31, "gemm_wgrad: too many tiles");
  ProfScope ps(st, PROF_GEMM, 2.0 * M * (double)K * N);
  const dim3 grid((unsigned)(tiles_n * tiles_k), (unsigned)msplit);
  const bf16_t* x = static_cast<const bf16_t*>(X);
  const bf16_t* g = static_cast<const bf16_t*>(G);
  float* out = msplit > 1 ? part : dW;
  const int ldo = msplit > 1 ? N : ldw;
  float* dbo = msplit > 1 && db ? part + (size_t)K * N : db;
  const int zero_to = msplit > 1 ? N : ldw;
  if (x3)
    hipLaunchKernelGGL(wgrad_kernel<true>, grid, dim3(256), 0, st, x, ldx, g, ldg, M, K, N, pwx,
                       pwg, out, ldo, (int64_t)plane, dbo, zero_to, T, tiles_n);
  else
    hipLaunchKernelGGL(wgrad_kernel<false>, grid, dim3(256), 0, st, x, ldx, g, ldg, M, K, N, pwx,
                       pwg, out, ldo, (int64_t)plane, dbo, zero_to, T, tiles_n);
  VTD_LAUNCH_CHECK("gemm_wgrad");
  if (msplit > 1) {
    const int64_t total = (int64_t)K * ldw + N;
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, part, msplit, K, N,
                       dW, ldw, db);
    VTD_LAUNCH_CHECK("gemm_wgrad reduce");
  }
  return VTD_OK;
}

}  // namespace vtd

extern "C" {

int vtd_gemm_wgrad(int M, int K, int N, const void* X_dev, int ldx, const void* G_dev, int ldg,
                   int dtype, float* dW_dev, int ldw, float* db_dev, float* part_dev,
                   size_t part_bytes, int msplit, void* stream) {
  return vtd::gemm_wgrad_launch(M, K, N, X_dev, ldx, G_dev, ldg, dtype, dW_dev, ldw, db_dev,
                                part_dev, part_bytes, msplit, static_cast<hipStream_t>(stream));
}

int vtd_gemm_wgrad_choice(int M, int K, int N, int dtype) {
  return vtd::gemm_wgrad_choice(M, K, N, dtype);
}

}  // extern "C"
