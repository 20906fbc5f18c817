// Numerical health: per-tensor statistics of a table of fp32 device tensors in one pass
// (vtd_stats_plan_bytes, vtd_stats_plan_upload, vtd_tensor_stats; include/vtd.h "Numerical
// health" states a record's semantics).  What the reference's check_inf_nan / check_weights /
// CheckModelWeight read off a tensor on the host -- NaN and Inf counts, the largest and smallest
// value -- and the fp64 sum of squares a gradient norm needs, without moving the tensor.
//
// Work unit: one chunk of kChunk = 16 Ki elements (64 KiB) of one tensor per workgroup of 256
// threads, counted from the tensor's element 0; the plan holds the tensor descriptors and a
// chunk -> (tensor, chunk in tensor) map, as vtd_optimizer.hip's does for its tiles.  Why 16 Ki:
// each thread issues 16 independent 16-B loads, enough to keep the memory queue full from a
// workgroup's first instruction to its last; the workgroup's reduction (42 cross-lane moves
// per wave, one barrier, one 32-B store) is paid once per 64 KiB read; the partials are 1 / 2048
// of the bytes read; and the 180 M parameters of C2 still make 11 k workgroups, 43 per CU, so the
// tail of the last round is small.  A tensor shorter than a chunk (every bias) costs one mostly
// idle workgroup, which at 2 k elements is still one 16-B load per thread.
//
// Vector width V = 4 / 2 / 1 floats per load, per tensor: the widest for which x, out and 4 n are
// all multiples of 4 V bytes (a torch view can start at any multiple of 4 B).  A chunk starts at a
// multiple of 64 KiB from the base, so every vector of a tensor is aligned when its base is, and
// n % V == 0 leaves no partial vector.  Thread t of the workgroup takes vectors t, t + 256, ...
// of the chunk in that order and its V elements in index order: per thread a sequential sum, so
// the order is a function of (n, V) alone.
//
// Reduction tree (fixed; no atomics): per wave the xor butterfly over lanes 32, 16, 8, 4, 2, 1
// (every lane ends with the wave's total), lane 0 of each wave stores it to LDS, and after the
// barrier thread 0 merges waves 0, 1, 2, 3 in that order and writes the chunk's partial.  The
// fold kernel runs one wave per tensor: lane l merges partials l, l + 64, ... in that order, then
// the same butterfly, and lane 0 writes the record.  max / min merge by comparison and counts by
// integer addition, both exact in any order; sumsq adds fp64 values in the order above.
//
// LDS: 4 partials of 32 B, written by 4 lanes and read by one thread: nothing to conflict.
#include "vtd_common.h"

#include <vector>

namespace vtd {
namespace {

constexpr int kChunk = VTD_STATS_CHUNK;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kInfBits = 0x7f800000u;

struct StatsDesc {
  const float* x; float* out;
  int64_t n;
  int chunk0, nchunks;     // this tensor's partials are workspace[chunk0, chunk0 + nchunks)
  int vec;                 // 4 / 2 / 1 floats per load
  int pad_;
};
struct Partial {           // 32 B; one per chunk
  float max, min;
  int nan, pos_inf, neg_inf, pad_;
  double sumsq;
};
static_assert(sizeof(Partial) == 32 && sizeof(vtd_tensor_stat) == 48, "record layout");

// the counts of a chunk fit an int; a tensor's need 64 bits
template <class Count>
struct Acc {
  float mx, mn;
  Count nan, pinf, ninf;
  double ss;
};
template <class Count>
__device__ __forceinline__ Acc<Count> empty() {
  return Acc<Count>{__uint_as_float(0xff800000u), __uint_as_float(kInfBits), 0, 0, 0, 0.0};
}

// The table's pointers are loaded from memory: tell the compiler they are device memory
// (global_* instead of flat_* accesses), as vtd_optimizer.hip does.
template <class T> using gptr = __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ gptr<T> as_global(T* p) {
  return (gptr<T>)p;
}

__device__ __forceinline__ void take(Acc<int>& a, float x) {
  const uint32_t bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
  if (x > a.mx) a.mx = x;                          // false for a NaN: it never moves max / min
  if (x < a.mn) a.mn = x;
  a.nan += mag > kInfBits ? 1 : 0;
  a.pinf += bits == kInfBits ? 1 : 0;
  a.ninf += bits == (kInfBits | 0x80000000u) ? 1 : 0;
  const double d = (double)x;                      // converted first: d * d is exact
  a.ss = mag < kInfBits ? a.ss + d * d : a.ss;
}

template <class A, class B>
__device__ __forceinline__ void merge(Acc<A>& a, const Acc<B>& b) {
  if (b.mx > a.mx) a.mx = b.mx;
  if (b.mn < a.mn) a.mn = b.mn;
  a.nan += b.nan; a.pinf += b.pinf; a.ninf += b.ninf;
  a.ss += b.ss;
}

// xor butterfly over the 64 lanes; every lane ends with the same total
template <class Count>
__device__ __forceinline__ void wave_merge(Acc<Count>& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc<Count> b;
    b.mx = __shfl_xor(a.mx, o, 64); b.mn = __shfl_xor(a.mn, o, 64);
    b.nan = __shfl_xor(a.nan, o, 64); b.pinf = __shfl_xor(a.pinf, o, 64);
    b.ninf = __shfl_xor(a.ninf, o, 64);
    b.ss = __shfl_xor(a.ss, o, 64);
    merge(a, b);
  }
}

// One chunk: `nloc` elements from element `base` of the tensor.  FULL: nloc == kChunk, no bound
// checks, so the loads of an unrolled group issue back to back.  OUT: write the NaN-replaced copy.
template <int V, bool FULL, bool OUT>
__device__ __forceinline__ void scan(const StatsDesc& d, int64_t base, int nloc, float replace_nan,
                                     Acc<int>& a) {
  typedef float vecf __attribute__((ext_vector_type(V)));
  constexpr int kIters = kChunk / (kThreads * V);
  const gptr<const float> px = as_global(d.x) + base;
  const gptr<float> po = as_global(d.out) + base;
#pragma unroll 8
  for (int i = 0; i < kIters; ++i) {
    const int e = (i * kThreads + (int)threadIdx.x) * V;
    if (!FULL && e >= nloc) break;                 // nloc % V == 0: a whole vector or none
    float v[V];
    if constexpr (V == 1) {
      v[0] = px[e];
    } else {
      const vecf w = *(gptr<const vecf>)(px + e);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = w[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) take(a, v[j]);
    if constexpr (OUT) {
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = v[j] != v[j] ? replace_nan : v[j];
      if constexpr (V == 1) {
        po[e] = v[0];
      } else {
        vecf w;
#pragma unroll
        for (int j = 0; j < V; ++j) w[j] = v[j];
        *(gptr<vecf>)(po + e) = w;
      }
    }
  }
}

template <int V>
__device__ __forceinline__ void scan_v(const StatsDesc& d, int64_t base, int nloc,
                                       float replace_nan, Acc<int>& a) {
  const bool full = nloc == kChunk;                // uniform per workgroup, as is d.out
  if (d.out) {
    if (full) scan<V, true, true>(d, base, nloc, replace_nan, a);
    else scan<V, false, true>(d, base, nloc, replace_nan, a);
  } else {
    if (full) scan<V, true, false>(d, base, nloc, replace_nan, a);
    else scan<V, false, false>(d, base, nloc, replace_nan, a);
  }
}

__global__ __launch_bounds__(kThreads) void stats_chunk_kernel(const StatsDesc* __restrict__ descs,
                                                               const int2* __restrict__ map,
                                                               Partial* __restrict__ partials,
                                                               float replace_nan) {
  __shared__ Acc<int> waves[kWaves];
  const int2 where = map[blockIdx.x];
  const StatsDesc d = descs[where.x];
  const int64_t base = (int64_t)where.y * kChunk;
  const int64_t left = d.n - base;
  const int nloc = left < kChunk ? (int)left : kChunk;
  Acc<int> a = empty<int>();
  if (d.vec == 4) scan_v<4>(d, base, nloc, replace_nan, a);
  else if (d.vec == 2) scan_v<2>(d, base, nloc, replace_nan, a);
  else scan_v<1>(d, base, nloc, replace_nan, a);
  wave_merge(a);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = waves[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) merge(a, waves[w]);
  // (kernel-argument pointers are known to be global memory: no as_global needed)
  partials[d.chunk0 + where.y] = Partial{a.mx, a.mn, a.nan, a.pinf, a.ninf, 0, a.ss};
}

// one wave per tensor
__global__ __launch_bounds__(64) void stats_fold_kernel(const StatsDesc* __restrict__ descs,
                                                        const Partial* __restrict__ partials,
                                                        vtd_tensor_stat* __restrict__ stats) {
  const StatsDesc d = descs[blockIdx.x];
  const Partial* p = partials + d.chunk0;
  Acc<int64_t> a = empty<int64_t>();
  for (int c = threadIdx.x; c < d.nchunks; c += 64) {
    const Partial q = p[c];
    merge(a, Acc<int>{q.max, q.min, q.nan, q.pos_inf, q.neg_inf, q.sumsq});
  }
  wave_merge(a);
  if (threadIdx.x != 0) return;
  vtd_tensor_stat r;
  r.max = a.mx; r.min = a.mn; r.n = d.n;
  r.nan = a.nan; r.pos_inf = a.pinf; r.neg_inf = a.ninf; r.sumsq = a.ss;
  stats[blockIdx.x] = r;
}

// ------------------------------------------------------------------ plan (host)
int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

size_t desc_bytes(int n_tensors) {
  return (size_t)round_up((int64_t)n_tensors * sizeof(StatsDesc), 16);
}

int plan_size(const vtd_stats_tensor* t, int n_tensors, size_t* plan_bytes,
              size_t* workspace_bytes, int* chunks, const char* what) {
  const std::string w(what);
  VTD_CHECK_ARG(plan_bytes && workspace_bytes && chunks, w + ": null output");
  VTD_CHECK_ARG(n_tensors > 0, w + ": n_tensors must be positive");
  VTD_CHECK_ARG(t, w + ": null tensor table");
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const std::string at = w + ": tensor " + std::to_string(i);
    VTD_CHECK_ARG(t[i].x, at + ": null x");
    VTD_CHECK_ARG(t[i].n > 0, at + ": n must be positive");
    VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(t[i].x) % 4 == 0, at + ": x needs a 4-B aligned base");
    VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(t[i].out) % 4 == 0,
                  at + ": out needs a 4-B aligned base");
    total += chunks_of(t[i].n);
    VTD_CHECK_ARG(total <= 0x7fffffff, w + ": too many chunks (more than an int holds)");
  }
  *chunks = (int)total;
  *plan_bytes = desc_bytes(n_tensors) + (size_t)total * sizeof(int2);
  *workspace_bytes = (size_t)total * sizeof(Partial);
  return VTD_OK;
}

}  // namespace
}  // namespace vtd

extern "C" {

int vtd_stats_plan_bytes(const vtd_stats_tensor* tensors, int n_tensors, size_t* plan_bytes,
                         size_t* workspace_bytes, int* chunks) {
  return vtd::plan_size(tensors, n_tensors, plan_bytes, workspace_bytes, chunks,
                        "stats_plan_bytes");
}

int vtd_stats_plan_upload(const vtd_stats_tensor* tensors, int n_tensors, void* plan_dev,
                          size_t plan_bytes, void* stream) {
  using namespace vtd;
  size_t need = 0, ws = 0;
  int chunks = 0;
  if (int rc = plan_size(tensors, n_tensors, &need, &ws, &chunks, "stats_plan_upload")) return rc;
  VTD_CHECK_ARG(plan_dev, "stats_plan_upload: null plan_dev");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(plan_dev) % 16 == 0,
                "stats_plan_upload: plan_dev needs a 16-B aligned base");
  VTD_CHECK_ARG(plan_bytes >= need, "stats_plan_upload: plan_bytes too small");
  std::vector<char> host(need, 0);
  StatsDesc* d = reinterpret_cast<StatsDesc*>(host.data());
  int2* map = reinterpret_cast<int2*>(host.data() + desc_bytes(n_tensors));
  int at = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const vtd_stats_tensor& a = tensors[i];
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out) |
                           (uintptr_t)(a.n % 4) * 4;
    d[i].x = a.x; d[i].out = a.out; d[i].n = a.n;
    d[i].chunk0 = at; d[i].nchunks = (int)chunks_of(a.n);
    d[i].vec = bits % 16 == 0 ? 4 : (bits % 8 == 0 ? 2 : 1);
    for (int c = 0; c < d[i].nchunks; ++c) map[at++] = int2{i, c};
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  VTD_HIP(hipMemcpyAsync(plan_dev, host.data(), need, hipMemcpyHostToDevice, st));
  VTD_HIP(hipStreamSynchronize(st));                 // `host` goes out of scope
  return VTD_OK;
}

int vtd_tensor_stats(const void* plan_dev, int n_tensors, int chunks, void* workspace,
                     size_t workspace_bytes, vtd_tensor_stat* stats_dev, float replace_nan,
                     void* stream) {
  using namespace vtd;
  VTD_CHECK_ARG(plan_dev, "tensor_stats: null plan_dev");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(plan_dev) % 16 == 0,
                "tensor_stats: plan_dev needs a 16-B aligned base");
  VTD_CHECK_ARG(n_tensors > 0 && chunks > 0, "tensor_stats: non-positive n_tensors / chunks");
  VTD_CHECK_ARG(workspace, "tensor_stats: null workspace");
  VTD_CHECK_ARG(stats_dev, "tensor_stats: null stats_dev");
  VTD_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(stats_dev) % 8 == 0,
                "tensor_stats: workspace and stats_dev need 8-B aligned bases");
  VTD_CHECK_ARG(workspace_bytes >= (size_t)chunks * sizeof(Partial),
                "tensor_stats: workspace_bytes too small (32 per chunk)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfScope ps(st, PROF_OTHER, 0.0);
  const char* base = static_cast<const char*>(plan_dev);
  const StatsDesc* descs = reinterpret_cast<const StatsDesc*>(base);
  const int2* map = reinterpret_cast<const int2*>(base + desc_bytes(n_tensors));
  Partial* partials = static_cast<Partial*>(workspace);
  hipLaunchKernelGGL(stats_chunk_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, st, descs, map,
                     partials, replace_nan);
  VTD_LAUNCH_CHECK("tensor_stats (chunks)");
  hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)n_tensors), dim3(64), 0, st, descs,
                     partials, stats_dev);
  VTD_LAUNCH_CHECK("tensor_stats (fold)");
  return VTD_OK;
}

}  // extern "C"
