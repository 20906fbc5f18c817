// Backward of the MultiHeadAttention core (vtd_attention_train's forward): dQ, dK, dV from
// qkv, O, dO and the forward's LSE, in VTD_BF16 and VTD_BF16X3 (include/vtd.h
// "vtd_attention_backward"; DESIGN.md "Attention backward").
//
//   delta_i = sum_d dO_id O_id          P = exp(scale q.k - lse)       dP = dO V^T
//   dS = P o (dP - delta) scale         dV = P^T dO     dK = dS^T Q    dQ = dS K
//
// P is recomputed tile by tile from qkv and lse; no N x N array is stored.  Two passes of one
// kernel template, both without atomics, without any workgroup waiting on another, and with a
// fixed summation order (the same inputs give the same bits):
//   KV pass  key-stationary: a wave owns 32 keys, keeps their K and V as MFMA B operands and
//            dK^T, dV^T in accumulators, and sweeps the 32-query slices of its (image, head);
//   Q pass   query-stationary: a wave owns 32 queries (Q, dO as B operands, dQ^T in
//            accumulators) and sweeps the 32-key slices.  It recomputes S and dP (7 products
//            over both passes instead of 5) and so needs no sum of dQ across key blocks.
// In both the stationary index is on the MFMA lane: S and dP leave the matrix core as
// [streamed row][stationary column] accumulators, which are already the B operands of the
// X^T P / X^T dS products (the forward's P V structure); the streamed tile has ONE row-major
// LDS image, read by rows (A operand of S, dP) and by ds_read_b64_tr_b16 (A operand of the
// transposed products).  -lse and -delta are the initial accumulators (bf16 mode; the split
// mode scales its fp32 score after the chain, as its forward does).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "vtd_common.h"
#include "vtd_launch.h"

namespace vtd {
namespace {

constexpr float kLog2e = 1.4426950408889634f;

// waves per workgroup (32 stationary rows each) and workgroups per CU the registers are capped for:
// dkp 128 needs the whole register file of a SIMD per wave (4 waves, one workgroup); the split
// mode at dkp <= 64 fits 256 registers (8 waves); bf16 runs 4-wave workgroups, several per CU,
// whose barriers are independent (measured against 8 waves in DESIGN.md "Attention backward")
constexpr int bwd_waves(int dkp, bool x3) { return dkp == 128 || !x3 ? 4 : 8; }
constexpr int bwd_min_blocks(int dkp, bool x3) { return dkp == 128 || x3 ? 1 : (dkp == 64 ? 2 : 4); }

template <int DKP, bool X3>
struct BwdCfg {
  static constexpr int NW = bwd_waves(DKP, X3);
  static constexpr int VS = DKP * 2 + 64;             // tile row stride (bytes): the forward's V image
  static constexpr int TILE = 32 * VS;                // one 32-row tile of one tensor, one plane
  static constexpr int PLANE = 2 * TILE;              // X1 tile, X2 tile
  static constexpr int NPL = X3 ? 2 : 1;              // hi plane, lo plane
  static constexpr int CONST_OFF = NPL * PLANE;       // 32 x -lse log2(e), -delta, 1 / rowsum (fp32)
  static constexpr int BUF = CONST_OFF + 512;
  static constexpr int EPC = X3 ? 4 : 8;              // elements per 16-B global chunk
  static constexpr int CPR = DKP / EPC;               // chunks per row
  static constexpr int NCH = 32 * CPR * 2;            // chunks per (X1, X2) tile pair
  static constexpr int KSTEPS = DKP / 16;
  static constexpr int DB = DKP / 32;
  // split mode at dkp 128: the lo fragments of the stationary rows live in LDS, not in 64
  // registers (a wave-private image per wave: 32 rows x 2 tensors, row stride DKP * 2 + 16 B)
  static constexpr bool YLO_LDS = X3 && DKP == 128;
  static constexpr int YS = DKP * 2 + 16;
  static constexpr int YLO_OFF = 2 * BUF;
  static constexpr int LDS = 2 * BUF + (YLO_LDS ? NW * 2 * 32 * YS : 0);
};

// 8 f32 values -> split-bf16 (hi, lo) fragments
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
  const uint32_t h0 = pack_bf16x2(a[0], a[1]), h1 = pack_bf16x2(a[2], a[3]);
  const uint32_t h2 = pack_bf16x2(b[0], b[1]), h3 = pack_bf16x2(b[2], b[3]);
  hi = __builtin_bit_cast(bf16x8, i32x4{(int)h0, (int)h1, (int)h2, (int)h3});
  lo = __builtin_bit_cast(bf16x8, i32x4{(int)pack_lo_bf16x2(a[0], a[1], h0),
                                        (int)pack_lo_bf16x2(a[2], a[3], h1),
                                        (int)pack_lo_bf16x2(b[0], b[1], h2),
                                        (int)pack_lo_bf16x2(b[2], b[3], h3)});
}
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  return __builtin_bit_cast(bf16x8, i32x4{(int)pack_bf16x2(a[0], a[1]), (int)pack_bf16x2(a[2], a[3]),
                                          (int)pack_bf16x2(b[0], b[1]), (int)pack_bf16x2(b[2], b[3])});
}
// 8 bf16 values times c, rounded to bf16 again (the forward's pre-scaled query)
__device__ __forceinline__ bf16x8 scale8(const bf16x8& v, float c) {
  const i32x4 raw = __builtin_bit_cast(i32x4, v);
  i32x4 sc;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    sc[j] = (int)pack_bf16x2(__uint_as_float((uint32_t)raw[j] << 16) * c,
                             __uint_as_float((uint32_t)raw[j] & 0xffff0000u) * c);
  return __builtin_bit_cast(bf16x8, sc);
}

// delta[b][h][i] = sum_d dO[i][h dkp + d] * O[i][h dkp + d] (fp32; O = hi + lo in the split
// mode).  8 lanes per (row, head), 4 columns per lane and step, butterfly sum: a fixed order.
template <bool X3>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(
    const void* __restrict__ o_, int ldo, const void* __restrict__ do_, int lddo, int B, int N,
    int heads, int dkp, float* __restrict__ delta) {
  const int64_t items = (int64_t)B * N * heads;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int sub = (int)(gid & 7);
  const int64_t item = (gid >> 3) < items ? (gid >> 3) : items - 1;
  const int64_t row = item / heads;
  const int h = (int)(item - row * heads);
  float s = 0.f;
  if constexpr (X3) {
    const float* dp = static_cast<const float*>(do_) + row * lddo + h * dkp;
    const bf16_t* oh = static_cast<const bf16_t*>(o_) + row * ldo + h * dkp;
    const bf16_t* ol = oh + ldo / 2;
    for (int d = sub * 4; d < dkp; d += 32) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(dp + d);
      const uint2 a = *reinterpret_cast<const uint2*>(oh + d);
      const uint2 b = *reinterpret_cast<const uint2*>(ol + d);
      s += g[0] * (__uint_as_float(a.x << 16) + __uint_as_float(b.x << 16));
      s += g[1] * (__uint_as_float(a.x & 0xffff0000u) + __uint_as_float(b.x & 0xffff0000u));
      s += g[2] * (__uint_as_float(a.y << 16) + __uint_as_float(b.y << 16));
      s += g[3] * (__uint_as_float(a.y & 0xffff0000u) + __uint_as_float(b.y & 0xffff0000u));
    }
  } else {
    const bf16_t* dp = static_cast<const bf16_t*>(do_) + row * lddo + h * dkp;
    const bf16_t* op = static_cast<const bf16_t*>(o_) + row * ldo + h * dkp;
    for (int d = sub * 4; d < dkp; d += 32) {
      const uint2 g = *reinterpret_cast<const uint2*>(dp + d);
      const uint2 a = *reinterpret_cast<const uint2*>(op + d);
      s += __uint_as_float(g.x << 16) * __uint_as_float(a.x << 16);
      s += __uint_as_float(g.x & 0xffff0000u) * __uint_as_float(a.x & 0xffff0000u);
      s += __uint_as_float(g.y << 16) * __uint_as_float(a.y << 16);
      s += __uint_as_float(g.y & 0xffff0000u) * __uint_as_float(a.y & 0xffff0000u);
    }
  }
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  if (sub == 0 && (gid >> 3) < items) {
    const int64_t b = row / N;
    const int n = (int)(row - b * N);
    delta[(b * heads + h) * N + n] = s;
  }
}

// One pass.  KV: stationary = keys (Y1 = K, Y2 = V), streamed = queries (X1 = Q, X2 = dO),
// outputs dK^T, dV^T.  !KV: stationary = queries (Y1 = Q, Y2 = dO), streamed = keys (X1 = K,
// X2 = V), output dQ^T.  S tile = X1 Y1^T, dP tile = X2 Y2^T, [streamed][stationary].
// Grid: one workgroup per (block of NW x 32 stationary rows, head, image), XCD-aware as the
// forward's: the blocks of one (image, head) share an XCD and stream the same tiles through
// its L2.  Rows beyond N are clamped on read (nothing is read past row B N - 1); streamed
// rows beyond N get P = 0, stationary rows beyond N are not written.
// DROP (vtd_attention_backward_dropout): the forward's mask M of (b, h, query, key) is
// regenerated per tile (vtd_philox.h; four keys of a query per Philox block in the Q pass, four
// queries of a key from two blocks in the KV pass): dP = M inv_keep (dO V^T) -- so -delta
// joins after the masking instead of as the initial accumulator -- dS = P (dP - delta) with the
// unmasked P, and the dV product takes P o M inv_keep.  The row-sum sweep stays unmasked.
template <int DKP, bool X3, bool KV, bool DROP>
__device__ __forceinline__ void attn_bwd_body(
    const void* qkv_, int ldqkv, const void* do_, int lddo, const float* lse, const float* delta,
    int N, int heads, float scale_log2, float scale, bf16_t* dqkv, int lddqkv, int nblk,
    float* rinv, DropKey dk) {      // (the kernels' own arguments carry the __restrict__)
  using C = BwdCfg<DKP, X3>;
  using T = std::conditional_t<X3, float, bf16_t>;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int nthreads = 64 * C::NW;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  int v = blockIdx.x;
  {
    const int G = gridDim.x, xcd = v & 7, q8 = G >> 3, r8 = G & 7;
    v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (v >> 3);
  }
  const int pair = v / nblk, blk = v - pair * nblk;
  const int b = pair / heads, h = pair - b * heads;
  const int inner = heads * DKP;
  const int64_t row0 = (int64_t)b * N;
  const int s0 = (blk * C::NW + wave) * 32;
  const bool active = s0 < N;
  const int srow = min(s0 + col, N - 1);
  const T* qkv = static_cast<const T*>(qkv_) + row0 * ldqkv + h * DKP;
  const T* dob = static_cast<const T*>(do_) + row0 * lddo + h * DKP;
  const float* lse_p = lse + (int64_t)pair * N;
  const float* del_p = delta + (int64_t)pair * N;
  // RENORM (split mode): lse arrives as one fp32 number per row, so exp2(score - lse) carries
  // the row's common factor 2^(error of lse), relative error ~ |lse| 2^-24 -- nothing for
  // ordinary scores, far over this mode's 2^-15 when the scores share a large offset.  The Q
  // pass therefore first sweeps the keys once for the row sums of exp2(score - lse), keeps
  // their reciprocals (per lane, and in rinv[b][h][i] for the KV pass, which runs after it) and
  // both passes use P = exp2(score - lse) / rowsum: one more S product, rows that sum to 1.
  constexpr bool RENORM = X3;
  float* rinv_p = rinv + (int64_t)pair * N;

  // stationary fragments: lane = row srow, k = d (st * 16 + half * 8 ..)
  bf16x8 y1h[C::KSTEPS], y2h[C::KSTEPS];
  bf16x8 y1l[X3 && !C::YLO_LDS ? C::KSTEPS : 1], y2l[X3 && !C::YLO_LDS ? C::KSTEPS : 1];
  char* ylo = smem + C::YLO_OFF + wave * (2 * 32 * C::YS) + col * C::YS + half * 16;
  {
    const T* p1 = qkv + (int64_t)srow * ldqkv + (KV ? inner : 0);
    const T* p2 = KV ? qkv + (int64_t)srow * ldqkv + 2 * inner : dob + (int64_t)srow * lddo;
#pragma unroll
    for (int st = 0; st < C::KSTEPS; ++st) {
      const int d = st * 16 + half * 8;
      if constexpr (C::YLO_LDS) {
        bf16x8 l1, l2;
        split8(*reinterpret_cast<const f32x4*>(p1 + d), *reinterpret_cast<const f32x4*>(p1 + d + 4),
               y1h[st], l1);
        split8(*reinterpret_cast<const f32x4*>(p2 + d), *reinterpret_cast<const f32x4*>(p2 + d + 4),
               y2h[st], l2);
        *reinterpret_cast<bf16x8*>(ylo + st * 32) = l1;
        *reinterpret_cast<bf16x8*>(ylo + 32 * C::YS + st * 32) = l2;
      } else if constexpr (X3) {
        split8(*reinterpret_cast<const f32x4*>(p1 + d), *reinterpret_cast<const f32x4*>(p1 + d + 4),
               y1h[st], y1l[st]);
        split8(*reinterpret_cast<const f32x4*>(p2 + d), *reinterpret_cast<const f32x4*>(p2 + d + 4),
               y2h[st], y2l[st]);
      } else {
        y1h[st] = *reinterpret_cast<const bf16x8*>(p1 + d);
        // the forward's query: scaled by scale log2(e) and rounded to bf16 again
        if constexpr (!KV) y1h[st] = scale8(y1h[st], scale_log2);
        y2h[st] = *reinterpret_cast<const bf16x8*>(p2 + d);
      }
    }
  }
  // row constants of the query: per lane in the Q pass, per streamed row (LDS) in the KV pass
  float nl = 0.f, nd = 0.f;
  if constexpr (!KV) {
    nl = -lse_p[srow] * kLog2e;
    nd = -del_p[srow];
  }
  f32x16 acc1[C::DB], acc2[KV ? C::DB : 1];    // dK^T or dQ^T; dV^T
#pragma unroll
  for (int i = 0; i < C::DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[i][r] = 0.f;
#pragma unroll
  for (int i = 0; i < (KV ? C::DB : 1); ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[i][r] = 0.f;

  // streamed tiles: global -> registers during the previous tile's compute -> LDS after it
  const T* x1 = qkv + (KV ? 0 : inner);
  const T* x2 = KV ? dob : qkv + 2 * inner;
  const int ld2 = KV ? lddo : ldqkv;
  constexpr int NPASS = (C::NCH + nthreads - 1) / nthreads;
  // the next tile's loads fly under this tile's compute, except where their 32 staging
  // registers would not fit beside the split dkp-128 fragments and accumulators
  constexpr bool EARLY = !(X3 && KV && DKP == 128);
  i32x4 stg[NPASS];
  float cst = 0.f;
  auto gload = [&](int t0) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int c = tid + i * nthreads;
      if (c < C::NCH) {
        const int t = c >= 32 * C::CPR;
        const int cc = c - t * 32 * C::CPR;
        const int r = cc / C::CPR, ch = cc - r * C::CPR;
        const int64_t row = min(t0 + r, N - 1);
        const T* src = t ? x2 + row * ld2 : x1 + row * ldqkv;
        stg[i] = *reinterpret_cast<const i32x4*>(src + ch * C::EPC);
      }
    }
    if constexpr (KV) {
      if (tid < (RENORM ? 96 : 64)) {
        const int r = min(t0 + (tid & 31), N - 1);
        cst = tid < 32 ? -lse_p[r] * kLog2e : tid < 64 ? -del_p[r] : rinv_p[r];
      }
    }
  };
  auto swrite = [&](int buf) {
    char* base = smem + buf * C::BUF;
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int c = tid + i * nthreads;
      if (c < C::NCH) {
        const int t = c >= 32 * C::CPR;
        const int cc = c - t * 32 * C::CPR;
        const int r = cc / C::CPR, ch = cc - r * C::CPR;
        if constexpr (X3) {
          const f32x4 f = __builtin_bit_cast(f32x4, stg[i]);
          char* dst = base + t * C::TILE + r * C::VS + ch * 8;
          const uint32_t h0 = pack_bf16x2(f[0], f[1]), h1 = pack_bf16x2(f[2], f[3]);
          *reinterpret_cast<uint2*>(dst) = uint2{h0, h1};
          *reinterpret_cast<uint2*>(dst + C::PLANE) =
              uint2{pack_lo_bf16x2(f[0], f[1], h0), pack_lo_bf16x2(f[2], f[3], h1)};
        } else {
          *reinterpret_cast<i32x4*>(base + t * C::TILE + r * C::VS + ch * 16) = stg[i];
        }
      }
    }
    if constexpr (KV) {
      if (tid < (RENORM ? 96 : 64)) *reinterpret_cast<float*>(base + C::CONST_OFF + tid * 4) = cst;
    }
  };

  const int ntiles = (N + 31) / 32;
  const int tr_row = 4 * half + ((lane & 15) >> 2);
  const int tr_d = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  float ir = 1.f, rs = 0.f;          // Q pass: 1 / rowsum of the lane's query; its running sum
  // sweep 0 (Q pass with RENORM only): row sums; sweep 1: the gradients
  for (int sweep = (RENORM && !KV) ? 0 : 1; sweep < 2; ++sweep) {
  const bool pre = sweep == 0;
  gload(0);
  swrite(0);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int t0 = t * 32;
    const bool more = t + 1 < ntiles;
    if (more && EARLY) gload(t0 + 32);
    if (active) {
      const char* img1 = smem + (t & 1) * C::BUF;     // X1 tile (hi); X2 at + TILE; lo at + PLANE
      const char* img2 = img1 + C::TILE;
      // per-register row constants (KV): register 4 g + j is streamed row 8 g + 4 half + j
      f32x4 nl4[4], nd4[4], ir4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if constexpr (KV) {
          const float* cp = reinterpret_cast<const float*>(img1 + C::CONST_OFF) + 8 * g + 4 * half;
          nl4[g] = *reinterpret_cast<const f32x4*>(cp);
          nd4[g] = *reinterpret_cast<const f32x4*>(cp + 32);
          if constexpr (RENORM) ir4[g] = *reinterpret_cast<const f32x4*>(cp + 64);
        } else {
          nl4[g] = f32x4{nl, nl, nl, nl};
          nd4[g] = f32x4{nd, nd, nd, nd};
          ir4[g] = f32x4{ir, ir, ir, ir};
        }
      }
      // DROP: the tile's 16 keep bits per lane first, while the score registers are not yet
      // live (bit 4 g + j: streamed row t0 + 8 g + 4 half + j, stationary row s0 + col)
      uint32_t keep = 0;
      if constexpr (DROP) {
        if (!pre) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int x0 = t0 + 8 * g + 4 * half;
            keep |= (KV ? drop_keep4_queries(dk, b, h, x0, s0 + col)
                        : drop_keep4_keys(dk, b, h, s0 + col, x0)) << (4 * g);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = X3 ? 0.f : nl4[r >> 2][r & 3];
        dp[r] = DROP ? 0.f : nd4[r >> 2][r & 3];
      }
      const char* r1 = img1 + col * C::VS + half * 16;
      const char* r2 = img2 + col * C::VS + half * 16;
#pragma unroll
      for (int st = 0; st < C::KSTEPS; ++st) {
        bf16x8 a1 = *reinterpret_cast<const bf16x8*>(r1 + st * 32);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(r2 + st * 32);
        if constexpr (X3) {
          const bf16x8 a1l = *reinterpret_cast<const bf16x8*>(r1 + C::PLANE + st * 32);
          const bf16x8 a2l = *reinterpret_cast<const bf16x8*>(r2 + C::PLANE + st * 32);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, y1h[st], s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, y1h[st], s, 0, 0, 0);
          bf16x8 b1l, b2l;
          if constexpr (C::YLO_LDS) {        // the wave's own writes: ordered by its own waits
            b1l = *reinterpret_cast<const bf16x8*>(ylo + st * 32);
            b2l = *reinterpret_cast<const bf16x8*>(ylo + 32 * C::YS + st * 32);
          } else {
            b1l = y1l[st];
            b2l = y2l[st];
          }
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1l, s, 0, 0, 0);
          if (pre) continue;
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, y2h[st], dp, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2l, y2h[st], dp, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2l, dp, 0, 0, 0);
        } else {
          if constexpr (KV) a1 = scale8(a1, scale_log2);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, y1h[st], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, y2h[st], dp, 0, 0, 0);
        }
      }
      // P = exp2(score - lse) (log2 units), dS' = P (dP - delta); the scale joins in the epilogue
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (X3) s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], scale_log2, nl4[r >> 2][r & 3]));
        else s[r] = __builtin_amdgcn_exp2f(s[r]);
      }
      if (t0 + 32 > N) {      // ragged last tile: streamed rows beyond N contribute exactly zero
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t0 + (r & 3) + 8 * (r >> 2) + 4 * half >= N) s[r] = 0.f;
      }
      if (pre) {         // row sums only; summed in register order, then over the lane pair
#pragma unroll
        for (int r = 0; r < 16; ++r) rs += s[r];
      } else {
      if constexpr (RENORM) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= ir4[r >> 2][r & 3];
      }
      if constexpr (DROP) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool k = (keep >> (4 * g + j)) & 1u;
            dp[4 * g + j] = ((k ? dp[4 * g + j] * dk.inv_keep : 0.f) + nd4[g][j]) * s[4 * g + j];
            if constexpr (KV) s[4 * g + j] = k ? s[4 * g + j] * dk.inv_keep : 0.f;   // dV's operand
          }
        }
      } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] *= s[r];
      }
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const f32x4 p0 = {s[8 * st + 0], s[8 * st + 1], s[8 * st + 2], s[8 * st + 3]};
        const f32x4 p1 = {s[8 * st + 4], s[8 * st + 5], s[8 * st + 6], s[8 * st + 7]};
        const f32x4 d0 = {dp[8 * st + 0], dp[8 * st + 1], dp[8 * st + 2], dp[8 * st + 3]};
        const f32x4 d1 = {dp[8 * st + 4], dp[8 * st + 5], dp[8 * st + 6], dp[8 * st + 7]};
        bf16x8 ph, pl, dh, dl;
        if constexpr (X3) {
          if constexpr (KV) split8(p0, p1, ph, pl);
          split8(d0, d1, dh, dl);
        } else {
          if constexpr (KV) ph = pack8(p0, p1);
          dh = pack8(d0, d1);
        }
        const int rw = 16 * st + tr_row;
#pragma unroll
        for (int db = 0; db < C::DB; ++db) {
          const char* va = img1 + rw * C::VS + (db * 32 + tr_d) * 2;
          auto trA = [&](const char* p) {
            const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
            const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 8 * C::VS));
            return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          };
          const bf16x8 x1h = trA(va);
          acc1[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1h, dh, acc1[db], 0, 0, 0);
          if constexpr (X3) {
            const bf16x8 x1l = trA(va + C::PLANE);
            acc1[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1l, dh, acc1[db], 0, 0, 0);
            acc1[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1h, dl, acc1[db], 0, 0, 0);
          }
          if constexpr (KV) {
            const bf16x8 x2h = trA(va + C::TILE);
            acc2[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2h, ph, acc2[db], 0, 0, 0);
            if constexpr (X3) {
              const bf16x8 x2l = trA(va + C::TILE + C::PLANE);
              acc2[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2l, ph, acc2[db], 0, 0, 0);
              acc2[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2h, pl, acc2[db], 0, 0, 0);
            }
          }
        }
      }
      }   // !pre
    }
    if (more) {
      if constexpr (!EARLY) gload(t0 + 32);
      swrite((t + 1) & 1);
    }
    __syncthreads();
  }
  if (pre) {
    const auto pr = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
    ir = 1.f / (__uint_as_float(pr[0]) + __uint_as_float(pr[1]));
    if (active && half == 0 && s0 + col < N) rinv_p[s0 + col] = ir;
  }
  }   // sweep
  if (!active || s0 + col >= N) return;
  // accumulator register 4 g + j of block db is column d = db * 32 + 8 g + 4 half + j of the
  // lane's row; written in dtype form (bf16, or [hi | lo] with piece width lddqkv / 2)
  const int P = lddqkv / 2;
  bf16_t* op = dqkv + (row0 + s0 + col) * (int64_t)lddqkv + h * DKP + (KV ? inner : 0);
  auto store4 = [&](bf16_t* p, float a, float bb, float cc, float dd) {
    const uint32_t h0 = pack_bf16x2(a, bb), h1 = pack_bf16x2(cc, dd);
    *reinterpret_cast<uint2*>(p) = uint2{h0, h1};
    if constexpr (X3)
      *reinterpret_cast<uint2*>(p + P) =
          uint2{pack_lo_bf16x2(a, bb, h0), pack_lo_bf16x2(cc, dd, h1)};
  };
#pragma unroll
  for (int db = 0; db < C::DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = db * 32 + 8 * g + 4 * half;
      store4(op + d, acc1[db][4 * g] * scale, acc1[db][4 * g + 1] * scale,
             acc1[db][4 * g + 2] * scale, acc1[db][4 * g + 3] * scale);
      if constexpr (KV)
        store4(op + inner + d, acc2[db][4 * g], acc2[db][4 * g + 1], acc2[db][4 * g + 2],
               acc2[db][4 * g + 3]);
    }
}

template <int DKP, bool X3, bool KV>
__global__ __launch_bounds__(64 * bwd_waves(DKP, X3), bwd_min_blocks(DKP, X3)) void attn_bwd_kernel(
    const void* __restrict__ qkv_, int ldqkv, const void* __restrict__ do_, int lddo,
    const float* __restrict__ lse, const float* __restrict__ delta, int N, int heads,
    float scale_log2, float scale, bf16_t* __restrict__ dqkv, int lddqkv, int nblk,
    float* __restrict__ rinv) {
  attn_bwd_body<DKP, X3, KV, false>(qkv_, ldqkv, do_, lddo, lse, delta, N, heads, scale_log2, scale,
                                    dqkv, lddqkv, nblk, rinv, DropKey{});
}
// launch bounds of its own: one workgroup fewer per CU where the mask arithmetic needs the
// registers (DESIGN.md "Dropout", resource table)
constexpr int bwd_drop_min_blocks(int dkp, bool x3) {
  return dkp == 128 || x3 ? 1 : (dkp == 64 ? 2 : 3);
}
template <int DKP, bool X3, bool KV>
__global__ __launch_bounds__(64 * bwd_waves(DKP, X3), bwd_drop_min_blocks(DKP, X3))
void attn_bwd_drop_kernel(
    const void* __restrict__ qkv_, int ldqkv, const void* __restrict__ do_, int lddo,
    const float* __restrict__ lse, const float* __restrict__ delta, int N, int heads,
    float scale_log2, float scale, bf16_t* __restrict__ dqkv, int lddqkv, int nblk,
    float* __restrict__ rinv, uint32_t dk0, uint32_t dk1, uint32_t dthr, float inv_keep) {
  const DropKey dk{dk0, dk1, dthr, inv_keep};
  attn_bwd_body<DKP, X3, KV, true>(qkv_, ldqkv, do_, lddo, lse, delta, N, heads, scale_log2, scale,
                                   dqkv, lddqkv, nblk, rinv, dk);
}

template <int DKP, bool X3, bool KV>
int launch_pass(const void* qkv, int ldqkv, const void* dO, int lddo, const float* lse,
                float* delta, int B, int N, int heads, float scale, void* dqkv, int lddqkv,
                hipStream_t stream, const DropKey* dk) {
  using C = BwdCfg<DKP, X3>;
  static_assert(C::LDS <= 160 * 1024, "LDS budget");
  const int nblk = ((N + 31) / 32 + C::NW - 1) / C::NW;
  if (dk) {
    static std::once_flag donce[kMaxDevices];
    once_per_device(donce, [] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_drop_kernel<DKP, X3, KV>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
    });
    hipLaunchKernelGGL((attn_bwd_drop_kernel<DKP, X3, KV>), dim3(nblk * heads * B),
                       dim3(64 * C::NW), C::LDS, stream, qkv, ldqkv, dO, lddo, lse, delta, N, heads,
                       scale * kLog2e, scale, static_cast<bf16_t*>(dqkv), lddqkv, nblk,
                       delta + (size_t)B * heads * N, dk->k0, dk->k1, dk->thr, dk->inv_keep);
    VTD_LAUNCH_CHECK(KV ? "attention_backward_dropout (dK, dV)" : "attention_backward_dropout (dQ)");
    return VTD_OK;
  }
  static std::once_flag once[kMaxDevices];
  once_per_device(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_kernel<DKP, X3, KV>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
  });
  hipLaunchKernelGGL((attn_bwd_kernel<DKP, X3, KV>), dim3(nblk * heads * B), dim3(64 * C::NW),
                     C::LDS, stream, qkv, ldqkv, dO, lddo, lse, delta, N, heads, scale * kLog2e,
                     scale, static_cast<bf16_t*>(dqkv), lddqkv, nblk,
                     delta + (size_t)B * heads * N);      // rinv follows delta (split mode)
  VTD_LAUNCH_CHECK(KV ? "attention_backward (dK, dV)" : "attention_backward (dQ)");
  return VTD_OK;
}

template <int DKP, bool X3>
int launch_both(const void* qkv, int ldqkv, const void* dO, int lddo, const float* lse,
                float* delta, int B, int N, int heads, float scale, void* dqkv, int lddqkv,
                hipStream_t stream, const DropKey* dk) {
  // the Q pass first: in the split mode it leaves the row sums' reciprocals for the KV pass
  if (int rc = launch_pass<DKP, X3, false>(qkv, ldqkv, dO, lddo, lse, delta, B, N, heads, scale,
                                           dqkv, lddqkv, stream, dk))
    return rc;
  return launch_pass<DKP, X3, true>(qkv, ldqkv, dO, lddo, lse, delta, B, N, heads, scale, dqkv,
                                    lddqkv, stream, dk);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

int attention_backward_workspace_bytes(int B, int N, int heads, int dkp, int dtype,
                                       size_t* bytes) {
  VTD_CHECK_ARG(bytes, "attention_backward_workspace_bytes: null pointer");
  VTD_CHECK_ARG(B > 0 && N > 0 && heads > 0, "attention_backward_workspace_bytes: bad B/N/heads");
  VTD_CHECK_ARG(dkp == 32 || dkp == 64 || dkp == 128,
                "attention_backward_workspace_bytes: dkp must be 32/64/128");
  if (dtype != VTD_BF16 && dtype != VTD_BF16X3)
    return fail(VTD_ERR_UNSUPPORTED,
                "attention_backward_workspace_bytes: dtype must be VTD_BF16 or VTD_BF16X3");
  // delta, and in the split mode 1 / rowsum: fp32 [B][heads][N] each
  *bytes = (size_t)B * heads * N * sizeof(float) * (dtype == VTD_BF16X3 ? 2 : 1);
  return VTD_OK;
}

int attention_backward_launch(const void* qkv, const void* o, const void* dO, const float* lse,
                              int B, int N, int heads, int dkp, int ldqkv, int ldo, int lddo,
                              float scale, void* dqkv, int lddqkv, int dtype, void* ws,
                              size_t ws_bytes, hipStream_t stream, const DropKey* dk) {
  VTD_CHECK_ARG(qkv && o && dO && lse && dqkv && ws, "attention_backward: null pointer");
  VTD_CHECK_ARG(B > 0 && N > 0 && heads > 0, "attention_backward: bad B/N/heads");
  VTD_CHECK_ARG(dkp == 32 || dkp == 64 || dkp == 128, "attention_backward: dkp must be 32/64/128");
  VTD_CHECK_ARG(scale > 0 && std::isfinite(scale),
                "attention_backward: scale must be positive and finite");
  if (dtype != VTD_BF16 && dtype != VTD_BF16X3)
    return fail(VTD_ERR_UNSUPPORTED, "attention_backward: dtype must be VTD_BF16 or VTD_BF16X3");
  const bool x3 = dtype == VTD_BF16X3;
  const int inner = heads * dkp;
  VTD_CHECK_ARG((int64_t)heads * dkp * 3 < INT32_MAX, "attention_backward: heads * dkp too large");
  VTD_CHECK_ARG(ldqkv >= 3 * inner && ldqkv % 8 == 0,
                "attention_backward: ldqkv must be >= 3 heads dkp and a multiple of 8");
  VTD_CHECK_ARG(lddo >= inner && lddo % 8 == 0,
                "attention_backward: lddo must be >= heads dkp and a multiple of 8");
  VTD_CHECK_ARG(ldo > 0 && ldo % (x3 ? 16 : 8) == 0 && (x3 ? ldo / 2 : ldo) >= inner,
                "attention_backward: ldo (VTD_BF16X3: the piece width ldo / 2) must be >= heads dkp "
                "and a multiple of 8");
  VTD_CHECK_ARG(lddqkv > 0 && lddqkv % (x3 ? 16 : 8) == 0 && (x3 ? lddqkv / 2 : lddqkv) >= 3 * inner,
                "attention_backward: lddqkv (VTD_BF16X3: the piece width lddqkv / 2) must be >= "
                "3 heads dkp and a multiple of 8");
  VTD_CHECK_ARG(aligned16(qkv) && aligned16(o) && aligned16(dO) && aligned16(dqkv) &&
                    reinterpret_cast<uintptr_t>(lse) % 4 == 0 && aligned16(ws),
                "attention_backward: qkv, O, dO, dqkv, workspace must be 16-byte aligned");
  const int nblk = ((N + 31) / 32 + 3) / 4;
  VTD_CHECK_ARG((int64_t)nblk * heads * B < INT32_MAX && (int64_t)B * N * heads * 8 < ((int64_t)1 << 39),
                "attention_backward: grid too large");
  size_t need = 0;
  if (int rc = attention_backward_workspace_bytes(B, N, heads, dkp, dtype, &need)) return rc;
  if (ws_bytes < need)
    return fail(VTD_ERR_WORKSPACE, "attention_backward: workspace smaller than "
                                   "vtd_attention_backward_workspace_bytes");
  // S, dP in both passes; dV, dK; dQ: 7 products of 2 N^2 dkp each, 8 with the row-sum sweep
  ProfScope ps(stream, PROF_ATTN, (x3 ? 16.0 : 14.0) * B * heads * (double)N * N * dkp);
  float* delta = static_cast<float*>(ws);
  const int64_t lanes = (int64_t)B * N * heads * 8;
  const dim3 dgrid((unsigned)((lanes + 255) / 256));
  if (x3)
    hipLaunchKernelGGL(attn_bwd_delta_kernel<true>, dgrid, dim3(256), 0, stream, o, ldo, dO, lddo,
                       B, N, heads, dkp, delta);
  else
    hipLaunchKernelGGL(attn_bwd_delta_kernel<false>, dgrid, dim3(256), 0, stream, o, ldo, dO, lddo,
                       B, N, heads, dkp, delta);
  VTD_LAUNCH_CHECK("attention_backward delta");
#define VTD_BWD(D, X) \
  launch_both<D, X>(qkv, ldqkv, dO, lddo, lse, delta, B, N, heads, scale, dqkv, lddqkv, stream, dk)
  if (x3) return dkp == 32 ? VTD_BWD(32, true) : dkp == 64 ? VTD_BWD(64, true) : VTD_BWD(128, true);
  return dkp == 32 ? VTD_BWD(32, false) : dkp == 64 ? VTD_BWD(64, false) : VTD_BWD(128, false);
#undef VTD_BWD
}

}  // namespace vtd

extern "C" {

int vtd_attention_backward_workspace_bytes(int B, int N, int heads, int dkp, int dtype,
                                           size_t* bytes) {
  return vtd::attention_backward_workspace_bytes(B, N, heads, dkp, dtype, bytes);
}

int vtd_attention_backward(const void* qkv_dev, const void* o_dev, const void* do_dev,
                           const float* lse_dev, int B, int N, int heads, int dkp, int ldqkv,
                           int ldo, int lddo, float scale, void* dqkv_dev, int lddqkv, int dtype,
                           void* ws_dev, size_t ws_bytes, void* stream) {
  return vtd::attention_backward_launch(qkv_dev, o_dev, do_dev, lse_dev, B, N, heads, dkp, ldqkv,
                                        ldo, lddo, scale, dqkv_dev, lddqkv, dtype, ws_dev, ws_bytes,
                                        static_cast<hipStream_t>(stream));
}

int vtd_attention_backward_dropout(const void* qkv_dev, const void* o_dev, const void* do_dev,
                                   const float* lse_dev, int B, int N, int heads, int dkp,
                                   int ldqkv, int ldo, int lddo, float scale, void* dqkv_dev,
                                   int lddqkv, int dtype, void* ws_dev, size_t ws_bytes,
                                   void* stream, const vtd_dropout* drop) {
  vtd::DropKey dk;
  bool on;
  if (int rc = vtd::drop_prepare("vtd_attention_backward_dropout", drop, &dk, &on)) return rc;
  return vtd::attention_backward_launch(qkv_dev, o_dev, do_dev, lse_dev, B, N, heads, dkp, ldqkv,
                                        ldo, lddo, scale, dqkv_dev, lddqkv, dtype, ws_dev, ws_bytes,
                                        static_cast<hipStream_t>(stream), on ? &dk : nullptr);
}

}  // extern "C"
