// Dropout masks: Philox4x32-10 and the one definition of a mask bit that every kernel, the
// mask entries (vtd_dropout_mask*) and the numpy restatement in tests/dropout_oracle.py share
// (DESIGN.md "Dropout").  Host and device inline code.
//
// A mask bit is a pure function of (seed, step, site, logical index):
//   subkey  (k0, k1) = words 0, 1 of Philox(counter = (step lo, step hi, site, kDropTag),
//           key = (seed lo, seed hi)) -- computed once on the host per call;
//   patch   one Philox block under the subkey covers 2 rows x 4 columns of the index plane:
//           counter = (column >> 2, row >> 1 low, row >> 1 high, 0)   elementwise [rows][N]
//           counter = (j >> 2, i >> 1, h, b)                          attention (b, h, i, j)
//           output word w holds row (w >> 1) of the patch, columns 2 (w & 1) (low 16 bits) and
//           2 (w & 1) + 1 (high 16 bits);
//   keep    the element's 16-bit lane u >= thr, thr = round(rate * 65536) clamped to 65535:
//           realised rate thr / 65536, inv_keep = fp32(1 / (1 - thr / 65536)).
// Nothing else enters: no leading dimension, padding, batch size, kernel variant or pass.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define VTD_HD __host__ __device__ __forceinline__
#else
#define VTD_HD inline
#endif

namespace vtd {

constexpr uint32_t kDropTag = 0x44524F50u;   // "DROP": the subkey derivation's counter word 3

struct Philox4 { uint32_t w[4]; };

VTD_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// what a kernel receives: the subkey, the threshold and the kept scale
struct DropKey {
  uint32_t k0, k1, thr;
  float inv_keep;
};

inline DropKey drop_key(uint64_t seed, uint64_t step, uint32_t site, float rate) {
  const Philox4 s = philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), site, kDropTag,
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
  double t = (double)rate * 65536.0 + 0.5;
  uint32_t thr = t >= 65535.0 ? 65535u : (uint32_t)t;
  return DropKey{s.w[0], s.w[1], thr, (float)(1.0 / (1.0 - (double)thr / 65536.0))};
}

// keep bits (bit c = column 4 cb + c) of the 4 columns of patch column cb on one row
VTD_HD uint32_t keep4_words(uint32_t lo, uint32_t hi, uint32_t thr) {
  return ((lo & 0xffffu) >= thr ? 1u : 0u) | ((lo >> 16) >= thr ? 2u : 0u) |
         ((hi & 0xffffu) >= thr ? 4u : 0u) | ((hi >> 16) >= thr ? 8u : 0u);
}
// elementwise site: row m, columns 4 cb .. 4 cb + 3
VTD_HD uint32_t drop_keep4_rows(DropKey k, int64_t m, uint32_t cb) {
  const uint64_t pr = (uint64_t)m >> 1;
  const Philox4 p = philox4x32_10(cb, (uint32_t)pr, (uint32_t)(pr >> 32), 0u, k.k0, k.k1);
  const bool odd = m & 1;      // selects, not indexing: the block stays in registers
  return keep4_words(odd ? p.w[2] : p.w[0], odd ? p.w[3] : p.w[1], k.thr);
}
// attention site: query i, keys j0 .. j0 + 3 (j0 % 4 == 0)
VTD_HD uint32_t drop_keep4_keys(DropKey k, int b, int h, int i, int j0) {
  const Philox4 p = philox4x32_10((uint32_t)j0 >> 2, (uint32_t)i >> 1, (uint32_t)h, (uint32_t)b,
                                  k.k0, k.k1);
  const bool odd = i & 1;
  return keep4_words(odd ? p.w[2] : p.w[0], odd ? p.w[3] : p.w[1], k.thr);
}
// attention site: key j, queries i0 .. i0 + 3 (i0 % 4 == 0): two patches, one 16-bit lane of
// each row
VTD_HD uint32_t drop_keep4_queries(DropKey k, int b, int h, int i0, int j) {
  const bool w = (j >> 1) & 1;
  const int sh = (j & 1) * 16;
  uint32_t bits = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const Philox4 p = philox4x32_10((uint32_t)j >> 2, ((uint32_t)i0 >> 1) + t, (uint32_t)h,
                                    (uint32_t)b, k.k0, k.k1);
    bits |= ((((w ? p.w[1] : p.w[0]) >> sh) & 0xffffu) >= k.thr ? 1u : 0u) << (2 * t);
    bits |= ((((w ? p.w[3] : p.w[2]) >> sh) & 0xffffu) >= k.thr ? 1u : 0u) << (2 * t + 1);
  }
  return bits;
}

}  // namespace vtd
