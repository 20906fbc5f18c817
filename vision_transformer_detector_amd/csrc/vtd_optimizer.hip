// Adam step of keras.optimizers.Adam fused with the ClipWeight constraint (vtd.py:209-236) and
// with the re-pack of the forward's operands: ONE kernel, one launch per training step over a
// table of tensors (vtd_train_plan_upload, vtd_train_step; include/vtd.h).  A table entry
// (vtd_train_tensor) carries vtd_pack_dense's grouping, a destination format, a constraint flag
// and an update rule.  vtd_adam_tensor is the ungrouped, always-constrained, dense-rule form of
// vtd_train_tensor: the vtd_adam_* entries convert their table (as_train_tensor) and run the
// same plan code and the same kernel.
//
// This file is compiled with -ffp-contract=off (Makefile) and with hipcc's correctly rounded
// fp32 sqrt and division: every operation of adam_element is one IEEE fp32 operation, in the
// order written, so the result is bit-identical to a numpy float32 restatement
// (tests/adam_oracle.py step32, tests/train_oracle.py sparse32).  The clips are comparisons:
// fminf / fmaxf drop a NaN and tf.clip_by_value does not.
//
// Work unit: a tile of 64 PACKED columns k' (k0' a multiple of 64) by 64 Keras columns n of one
// matrix, 256 threads, or 256 elements of a vector.  The plan holds the tensor descriptors and a
// tile -> (tensor, tile in tensor) map; workgroup b takes map[b].  Every element belongs to
// exactly one thread: no atomics, the same bits on every run.
//
//   phase 1 (coalesced along N, the Keras layout's contiguous axis): each thread takes V
//     consecutive columns of one row, V = 4 / 2 / 1 the widest vector that every row start of
//     the tensor is aligned for (N % V == 0; the bases are 16-B aligned) -- 64 / V threads per
//     tile row, 4 V rows per pass, 16 / V passes.  Tile row kk holds k' = k0' + kk; it is the
//     image of k = (k' / k_group_p) k_group + k' % k_group_p when k' % k_group_p < k_group and
//     k' / k_group_p < K / k_group, else a pad row.  A real row reads w, m, v, g, updates, writes
//     w, m, v back and leaves the new w in LDS; pad rows and columns n >= N leave 0 there, so a
//     phase-2 run of 8 k' that straddles a group's end (k_group 10, k_group_p 32: k' = 8 .. 15
//     is two real columns and six pads) reads its zeros from LDS like any other value.  Along N
//     the tile stays in the Keras layout, so a vector of V columns never meets a group boundary.
//     Ungrouped (k_group = K, one group): the row map is the identity on [0, K) and every
//     k' >= K is a pad; without a destination the plan sets k_group = k_group_p = K.
//   phase 2 (coalesced along K, the packed layout's contiguous axis): each thread takes 8
//     consecutive k' of one column n, converts them with the conversions vtd_pack_dense /
//     vtd_split_bf16x3 use (pack_bf16x2, pack_lo_bf16x2) and stores 16 B per piece to packed
//     row row_offset + (n / n_group) n_group_p + n % n_group: the 8 threads of a column write one
//     whole 128-B run, a wave 8 columns.  An fp32 destination stores the 8 values as two 16-B
//     stores.
//
// LDS layout: float tile[64][65], element (kk, nn) at word 65 kk + nn.  gfx950's LDS has 64 banks
// of 4 B, bank = word mod 64 = (kk + nn) mod 64 since 65 = 1 (mod 64).
//   phase-1 writes (4-B, one per column of the thread): a wave holds V tile rows; for a fixed j
//     lane l writes column V c + j (c = l mod (64 / V)) of row r0 + q (q = l / (64 / V) < V):
//     banks (r0 + j + q + V c) mod 64, and q + V c is a bijection onto [0, 64): no two lanes
//     share a bank.
//   phase-2 reads (4-B): lane l reads (8 (l & 7) + j, n0 + (l >> 3)) for j = 0 .. 7: banks
//     (8 (l & 7) + (l >> 3) + j + n0) mod 64, and 8 a + b with a, b < 8 is a bijection onto
//     [0, 64): conflict-free.
// A pitch of 64 would put the whole phase-2 read of a wave on 8 banks (8-way conflict).
//
// Padding rule: for every real n the kernel writes the whole piece(s) [0, K_p) of its packed
// row (K_p = ld, or ld / 3 in split-bf16), zeros at every k' that is no image of a real k.
// Packed rows that are the image of no n (the pad rows inside a group, rows >= N, the rows of
// other tensors sharing the buffer) and everything outside the buffers stay untouched.  A vector
// writes the images of its elements [0, N) in its fp32 destination.
#include "vtd_common.h"

#include <cmath>
#include <vector>

namespace vtd {
namespace {

constexpr int kTile = 64;           // tile edge (K and N)
constexpr int kPitch = kTile + 1;   // LDS row pitch in words (see above)
constexpr int kThreads = 256;
constexpr int kVecTile = 256;       // elements of a vector per workgroup

// device form of vtd_train_tensor plus what the plan derives from it
struct StepDesc {
  float* w; float* m; float* v; const float* g;
  void* packed;
  int kind, K, N, ld;
  int kp;        // piece width of a packed row (matrix); K without a destination
  int ntn;       // tiles along N (matrix)
  int vec;       // 4 / 2 / 1: columns per thread in phase 1
  int pk;        // destination: 0 none, 1 bf16, 2 split-bf16 [hi | hi | lo], 3 fp32
  int kg, kgp, ng, ngp, off;
  int constrain, rule;
  int pad_;
};
struct AdamScalars {
  float alpha, beta1, beta2, epsilon, clipvalue, max_weight;
  int constrain;
};

// The table's pointers are loaded from memory, so the compiler cannot tell their address space
// and would use flat_* accesses; they are device-memory pointers: global_* loads and stores.
template <class T> using gptr = __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ gptr<T> as_global(T* p) {
  return (gptr<T>)p;
}

__device__ __forceinline__ float clip(float x, float lo, float hi) {
  return x < lo ? lo : (x > hi ? hi : x);          // NaN passes through
}

// one element under the tensor's rule; `constrain`: the step's flag and the tensor's.  Returns
// the new w.
__device__ __forceinline__ float adam_element(float w, float& m, float& v, float g,
                                              const AdamScalars& s, int rule, int constrain) {
  if (s.clipvalue > 0.f) g = clip(g, -s.clipvalue, s.clipvalue);
  const float omb1 = 1.f - s.beta1, omb2 = 1.f - s.beta2;
  if (rule == VTD_TRAIN_RULE_DENSE) {              // TF's ApplyAdam functor
    m = m + (g - m) * omb1;
    v = v + (g * g - v) * omb2;
    w = w - (m * s.alpha) / (sqrtf(v) + s.epsilon);
  } else {                                         // Keras's sparse path
    m = m * s.beta1 + g * omb1;
    v = v * s.beta2 + (g * g) * omb2;
    w = w - (s.alpha * m) / (sqrtf(v) + s.epsilon);
  }
  if (constrain) w = clip(w != w ? 1.f : w, -s.max_weight, s.max_weight);
  return w;
}

template <int V>
__device__ __forceinline__ void phase1(const StepDesc& d, const AdamScalars& s, int k0, int n0,
                                       float (*tile)[kPitch]) {
  typedef float vecf __attribute__((ext_vector_type(V)));
  const gptr<float> pw = as_global(d.w), pm = as_global(d.m), pv = as_global(d.v);
  const gptr<const float> pg = as_global(d.g);
  constexpr int kTpr = kTile / V;                  // threads per tile row
  constexpr int kRpp = kThreads / kTpr;            // rows per pass
  const int c = (threadIdx.x % kTpr) * V, r = threadIdx.x / kTpr;
  const int groups = d.K / d.kg, constrain = s.constrain && d.constrain;
#pragma unroll 2
  for (int p = 0; p < kTile / kRpp; ++p) {
    const int kk = p * kRpp + r, kq = k0 + kk, n = n0 + c;
    const int grp = kq / d.kgp, in = kq - grp * d.kgp;
    const int k = grp * d.kg + in;                 // used only when the row is real
    float out[V];
    if (in < d.kg && grp < groups && n < d.N) {    // N % V == 0: all V columns or none
      const int64_t at = (int64_t)k * d.N + n;
      float wv[V], mv[V], vv[V], gv[V];
      if constexpr (V == 1) {
        wv[0] = pw[at]; mv[0] = pm[at]; vv[0] = pv[at]; gv[0] = pg[at];
      } else {
        const vecf a = *(gptr<const vecf>)(pw + at);
        const vecf b = *(gptr<const vecf>)(pm + at);
        const vecf e = *(gptr<const vecf>)(pv + at);
        const vecf f = *(gptr<const vecf>)(pg + at);
#pragma unroll
        for (int j = 0; j < V; ++j) { wv[j] = a[j]; mv[j] = b[j]; vv[j] = e[j]; gv[j] = f[j]; }
      }
#pragma unroll
      for (int j = 0; j < V; ++j)
        out[j] = adam_element(wv[j], mv[j], vv[j], gv[j], s, d.rule, constrain);
      if constexpr (V == 1) {
        pw[at] = out[0]; pm[at] = mv[0]; pv[at] = vv[0];
      } else {
        vecf a, b, e;
#pragma unroll
        for (int j = 0; j < V; ++j) { a[j] = out[j]; b[j] = mv[j]; e[j] = vv[j]; }
        *(gptr<vecf>)(pw + at) = a;
        *(gptr<vecf>)(pm + at) = b;
        *(gptr<vecf>)(pv + at) = e;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) out[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) tile[kk][c + j] = out[j];
  }
}

__global__ __launch_bounds__(kThreads) void step_kernel(const StepDesc* __restrict__ descs,
                                                        const int2* __restrict__ map,
                                                        AdamScalars s) {
  __shared__ float tile[kTile][kPitch];
  const int2 where = map[blockIdx.x];
  const StepDesc d = descs[where.x];
  if (d.kind == VTD_ADAM_VECTOR) {
    const int n = where.y * kVecTile + threadIdx.x;
    if (n < d.N) {
      const gptr<float> pw = as_global(d.w), pm = as_global(d.m), pv = as_global(d.v);
      float m = pm[n], v = pv[n];
      const float w = adam_element(pw[n], m, v, as_global(d.g)[n], s, d.rule,
                                   s.constrain && d.constrain);
      pw[n] = w; pm[n] = m; pv[n] = v;
      if (d.packed)
        as_global(static_cast<float*>(d.packed))[d.off + (n / d.ng) * d.ngp + n % d.ng] = w;
    }
    return;
  }
  const int k0 = (where.y / d.ntn) * kTile, n0 = (where.y % d.ntn) * kTile;
  if (d.vec == 4) phase1<4>(d, s, k0, n0, tile);
  else if (d.vec == 2) phase1<2>(d, s, k0, n0, tile);
  else phase1<1>(d, s, k0, n0, tile);
  if (!d.packed) return;                            // uniform per workgroup
  __syncthreads();
  const int kc = k0 + 8 * (threadIdx.x & 7);
#pragma unroll
  for (int p = 0; p < kTile / (kThreads / 8); ++p) {
    const int nn = p * (kThreads / 8) + (threadIdx.x >> 3), n = n0 + nn;
    if (n >= d.N || kc >= d.kp) continue;           // kp % 8 == 0: all 8 or none
    const int64_t prow = (int64_t)d.off + (n / d.ng) * d.ngp + n % d.ng;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[kc - k0 + j][nn];
    if (d.pk == 3) {                                // fp32 staging [N_p][K_p]
      const gptr<float> row = as_global(static_cast<float*>(d.packed)) + prow * d.ld + kc;
      *(gptr<f32x4>)row = f32x4{v[0], v[1], v[2], v[3]};
      *(gptr<f32x4>)(row + 4) = f32x4{v[4], v[5], v[6], v[7]};
      continue;
    }
    const uint32_t h0 = pack_bf16x2(v[0], v[1]), h1 = pack_bf16x2(v[2], v[3]),
                   h2 = pack_bf16x2(v[4], v[5]), h3 = pack_bf16x2(v[6], v[7]);
    const i32x4 hi = {(int)h0, (int)h1, (int)h2, (int)h3};
    const gptr<bf16_t> row = as_global(static_cast<bf16_t*>(d.packed)) + prow * d.ld + kc;
    *(gptr<i32x4>)row = hi;
    if (d.pk == 2) {                                // B operand [hi | hi | lo]
      const i32x4 lo = {(int)pack_lo_bf16x2(v[0], v[1], h0), (int)pack_lo_bf16x2(v[2], v[3], h1),
                        (int)pack_lo_bf16x2(v[4], v[5], h2), (int)pack_lo_bf16x2(v[6], v[7], h3)};
      *(gptr<i32x4>)(row + d.kp) = hi;
      *(gptr<i32x4>)(row + 2 * d.kp) = lo;
    }
  }
}

// ------------------------------------------------------------------ plan (host)
int check_tensors(const vtd_train_tensor* t, int n, int dtype, const char* what) {
  const std::string w(what);
  VTD_CHECK_ARG(n > 0, w + ": n_tensors must be positive");
  VTD_CHECK_ARG(t, w + ": null tensor table");
  for (int i = 0; i < n; ++i) {
    const vtd_train_tensor& a = t[i];
    const std::string at = w + ": tensor " + std::to_string(i);
    VTD_CHECK_ARG(a.w && a.m && a.v && a.g, at + ": null pointer (w, m, v, g)");
    VTD_CHECK_ARG(a.kind == VTD_ADAM_MATRIX || a.kind == VTD_ADAM_VECTOR, at + ": bad kind");
    VTD_CHECK_ARG(a.N > 0 && (a.kind == VTD_ADAM_VECTOR || a.K > 0),
                  at + ": non-positive size");
    for (const void* p : {(const void*)a.w, (const void*)a.m, (const void*)a.v,
                          (const void*)a.g})
      VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(p) % 16 == 0, at + ": w, m, v, g need 16-B "
                    "aligned bases");
    VTD_CHECK_ARG(a.rule == VTD_TRAIN_RULE_DENSE || a.rule == VTD_TRAIN_RULE_SPARSE,
                  at + ": bad rule");
    VTD_CHECK_ARG(a.packed_dtype == VTD_TRAIN_PACK_NONE || a.packed_dtype == VTD_TRAIN_PACK_MODE ||
                  a.packed_dtype == VTD_TRAIN_PACK_F32, at + ": bad packed_dtype");
    VTD_CHECK_ARG((a.packed_dtype == VTD_TRAIN_PACK_NONE) == (a.packed == nullptr),
                  at + ": packed_dtype NONE goes with a null destination and only with one");
    if (!a.packed) continue;
    VTD_CHECK_ARG(a.packed_dtype != VTD_TRAIN_PACK_MODE || dtype == VTD_BF16 ||
                  dtype == VTD_BF16X3,
                  at + ": a destination in the mode's format needs dtype VTD_BF16 or VTD_BF16X3");
    VTD_CHECK_ARG(a.n_group > 0 && a.n_group_p >= a.n_group && a.N % a.n_group == 0,
                  at + ": bad n group (n_group > 0, n_group_p >= n_group, N % n_group == 0)");
    VTD_CHECK_ARG(a.row_offset >= 0, at + ": negative row_offset");
    if (a.kind == VTD_ADAM_VECTOR) {                  // fp32, ld and the k groups unused
      VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(a.packed) % 4 == 0,
                    at + ": a vector's destination needs a 4-B aligned base");
      continue;
    }
    // the row width first: an ungrouped entry (k_group = K, k_group_p = K_p) whose ld is too
    // small is told so, not that its groups overlap
    VTD_CHECK_ARG(a.k_group > 0 && a.K % a.k_group == 0,
                  at + ": bad k group (k_group > 0, K % k_group == 0)");
    const bool x3 = a.packed_dtype == VTD_TRAIN_PACK_MODE && dtype == VTD_BF16X3;
    VTD_CHECK_ARG(!x3 || a.ld % 3 == 0,
                  at + ": ld must be a multiple of 3 in split-bf16 (ld = 3 K_p)");
    const int64_t kp = x3 ? a.ld / 3 : a.ld;
    const int64_t last = (int64_t)(a.K / a.k_group - 1) * a.k_group_p + a.k_group;
    VTD_CHECK_ARG(kp >= last, at + ": ld too small (K_p < the last packed column + 1)");
    VTD_CHECK_ARG(a.k_group_p >= a.k_group, at + ": bad k group (k_group_p >= k_group)");
    VTD_CHECK_ARG(kp % 8 == 0 && reinterpret_cast<uintptr_t>(a.packed) % 16 == 0,
                  at + ": packed rows are written 16 B at a time: K_p % 8 == 0 and a 16-B "
                  "aligned base");
  }
  return VTD_OK;
}

int tensor_tiles(const vtd_train_tensor& a, int dtype, int* ntn, int* kp_out) {
  if (a.kind == VTD_ADAM_VECTOR) { *ntn = 1; *kp_out = 0; return (a.N + kVecTile - 1) / kVecTile; }
  // with a destination the K tiles run over the packed columns to K_p, so that every pad is zeroed
  const bool x3 = a.packed_dtype == VTD_TRAIN_PACK_MODE && dtype == VTD_BF16X3;
  const int kp = a.packed ? (x3 ? a.ld / 3 : a.ld) : a.K;
  *ntn = (a.N + kTile - 1) / kTile;
  *kp_out = kp;
  return ((kp + kTile - 1) / kTile) * *ntn;
}

size_t plan_bytes(int n, int64_t tiles) {
  return (size_t)round_up((int64_t)n * sizeof(StepDesc), 16) + (size_t)tiles * sizeof(int2);
}

// vtd_adam_tensor is the ungrouped, always-constrained, dense-rule form of vtd_train_tensor
vtd_train_tensor as_train_tensor(const vtd_adam_tensor& a, int dtype) {
  vtd_train_tensor t = {};
  t.w = a.w; t.m = a.m; t.v = a.v; t.g = a.g; t.packed = a.packed;
  t.kind = a.kind; t.K = a.K; t.N = a.N; t.ld = a.ld;
  t.k_group = a.K; t.k_group_p = dtype == VTD_BF16X3 ? a.ld / 3 : a.ld;      // K_p
  t.n_group = t.n_group_p = a.N;
  t.packed_dtype = a.packed ? VTD_TRAIN_PACK_MODE : VTD_TRAIN_PACK_NONE;
  t.constrain = 1; t.rule = VTD_TRAIN_RULE_DENSE;
  return t;
}

std::vector<vtd_train_tensor> as_train_table(const vtd_adam_tensor* t, int n, int dtype) {
  std::vector<vtd_train_tensor> out;
  for (int i = 0; t && i < n; ++i) out.push_back(as_train_tensor(t[i], dtype));
  return out;
}

// The three entries behind both tables; `who` ("adam" / "train") prefixes the error texts.
int plan_size(const vtd_train_tensor* tensors, int n_tensors, int dtype, size_t* bytes, int* tiles,
              const std::string& who) {
  const std::string what = who + "_plan_bytes";
  VTD_CHECK_ARG(bytes && tiles, what + ": null output");
  if (int rc = check_tensors(tensors, n_tensors, dtype, what.c_str())) return rc;
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    int ntn, kp;
    total += tensor_tiles(tensors[i], dtype, &ntn, &kp);
  }
  VTD_CHECK_ARG(total <= 0x7fffffff, what + ": too many tiles");
  *tiles = (int)total;
  *bytes = plan_bytes(n_tensors, total);
  return VTD_OK;
}

int plan_upload(const vtd_train_tensor* tensors, int n_tensors, int dtype, void* plan_dev,
                size_t plan_bytes, void* stream, const std::string& who) {
  size_t need = 0;
  int tiles = 0;
  if (int rc = plan_size(tensors, n_tensors, dtype, &need, &tiles, who)) return rc;
  const std::string what = who + "_plan_upload";
  VTD_CHECK_ARG(plan_dev, what + ": null plan_dev");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(plan_dev) % 16 == 0,
                what + ": plan_dev needs a 16-B aligned base");
  VTD_CHECK_ARG(plan_bytes >= need, what + ": plan_bytes too small");
  std::vector<char> host(need, 0);
  StepDesc* d = reinterpret_cast<StepDesc*>(host.data());
  int2* map = reinterpret_cast<int2*>(host.data() +
                                      round_up((int64_t)n_tensors * sizeof(StepDesc), 16));
  int at = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const vtd_train_tensor& a = tensors[i];
    const bool matrix = a.kind == VTD_ADAM_MATRIX;
    int ntn, kp;
    const int nt = tensor_tiles(a, dtype, &ntn, &kp);
    d[i].w = a.w; d[i].m = a.m; d[i].v = a.v; d[i].g = a.g; d[i].packed = a.packed;
    d[i].kind = a.kind; d[i].K = matrix ? a.K : 1; d[i].N = a.N;
    d[i].ld = a.ld; d[i].kp = kp; d[i].ntn = ntn;
    d[i].vec = a.N % 4 == 0 ? 4 : (a.N % 2 == 0 ? 2 : 1);
    d[i].pk = !a.packed ? 0 : a.packed_dtype == VTD_TRAIN_PACK_F32 ? 3
                              : dtype == VTD_BF16X3 ? 2 : 1;
    // without a destination the packed column is the Keras one
    d[i].kg = a.packed && matrix ? a.k_group : d[i].K;
    d[i].kgp = a.packed && matrix ? a.k_group_p : d[i].K;
    d[i].ng = a.packed ? a.n_group : a.N;
    d[i].ngp = a.packed ? a.n_group_p : a.N;
    d[i].off = a.packed ? a.row_offset : 0;
    d[i].constrain = a.constrain ? 1 : 0; d[i].rule = a.rule;
    for (int t = 0; t < nt; ++t) map[at++] = int2{i, t};
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  VTD_HIP(hipMemcpyAsync(plan_dev, host.data(), need, hipMemcpyHostToDevice, st));
  VTD_HIP(hipStreamSynchronize(st));                 // `host` goes out of scope
  return VTD_OK;
}

int launch_step(const void* plan_dev, int n_tensors, int tiles, int64_t t, double learning_rate,
                float beta1, float beta2, float epsilon, float clipvalue, int constrain,
                float max_weight, void* stream, const std::string& who) {
  const std::string what = who + "_step";
  VTD_CHECK_ARG(plan_dev, what + ": null plan_dev");
  VTD_CHECK_ARG(n_tensors > 0 && tiles > 0, what + ": non-positive n_tensors / tiles");
  VTD_CHECK_ARG(t >= 1, what + ": t (the step number) starts at 1");
  VTD_CHECK_ARG(!constrain || max_weight > 0.f, what + ": max_weight must be positive");
  // alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) in double from the fp32 betas, rounded once
  const double b1 = beta1, b2 = beta2;
  AdamScalars s;
  s.alpha = (float)(learning_rate * std::sqrt(1.0 - std::pow(b2, (double)t)) /
                    (1.0 - std::pow(b1, (double)t)));
  s.beta1 = beta1; s.beta2 = beta2; s.epsilon = epsilon;
  s.clipvalue = clipvalue > 0.f ? clipvalue : 0.f;   // <= 0 or NaN: no gradient clip
  s.max_weight = max_weight; s.constrain = constrain ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope ps(st, PROF_OTHER, 0.0);
  const char* base = static_cast<const char*>(plan_dev);
  const int2* map = reinterpret_cast<const int2*>(
      base + round_up((int64_t)n_tensors * sizeof(StepDesc), 16));
  hipLaunchKernelGGL(step_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st,
                     reinterpret_cast<const StepDesc*>(base), map, s);
  VTD_LAUNCH_CHECK(what);
  return VTD_OK;
}

}  // namespace
}  // namespace vtd

extern "C" {

int vtd_train_plan_bytes(const vtd_train_tensor* tensors, int n_tensors, int dtype, size_t* bytes,
                         int* tiles) {
  return vtd::plan_size(tensors, n_tensors, dtype, bytes, tiles, "train");
}

int vtd_train_plan_upload(const vtd_train_tensor* tensors, int n_tensors, int dtype,
                          void* plan_dev, size_t plan_bytes, void* stream) {
  return vtd::plan_upload(tensors, n_tensors, dtype, plan_dev, plan_bytes, stream, "train");
}

int vtd_train_step(const void* plan_dev, int n_tensors, int tiles, int64_t t,
                   double learning_rate, float beta1, float beta2, float epsilon, float clipvalue,
                   int constrain, float max_weight, void* stream) {
  return vtd::launch_step(plan_dev, n_tensors, tiles, t, learning_rate, beta1, beta2, epsilon,
                          clipvalue, constrain, max_weight, stream, "train");
}

// the head-only table: the same plan and the same kernel through as_train_tensor
int vtd_adam_plan_bytes(const vtd_adam_tensor* tensors, int n_tensors, int dtype, size_t* bytes,
                        int* tiles) {
  const auto table = vtd::as_train_table(tensors, n_tensors, dtype);
  return vtd::plan_size(tensors ? table.data() : nullptr, n_tensors, dtype, bytes, tiles, "adam");
}

int vtd_adam_plan_upload(const vtd_adam_tensor* tensors, int n_tensors, int dtype,
                         void* plan_dev, size_t plan_bytes, void* stream) {
  const auto table = vtd::as_train_table(tensors, n_tensors, dtype);
  return vtd::plan_upload(tensors ? table.data() : nullptr, n_tensors, dtype, plan_dev,
                          plan_bytes, stream, "adam");
}

int vtd_adam_step(const void* plan_dev, int n_tensors, int tiles, int64_t t,
                  double learning_rate, float beta1, float beta2, float epsilon, float clipvalue,
                  int constrain, float max_weight, void* stream) {
  return vtd::launch_step(plan_dev, n_tensors, tiles, t, learning_rate, beta1, beta2, epsilon,
                          clipvalue, constrain, max_weight, stream, "adam");
}

}  // extern "C"
