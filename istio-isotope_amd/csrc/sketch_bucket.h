// The bucket rule of the mergeable latency sketch (include/isim.h isim_sketch*,
// DESIGN.md §16), one header for sketch.cpp (host compiler) and sketch.hip
// (host and device): the bin of a u64 and the bounds of a bin, in exact
// integer arithmetic.
#pragma once

#include <cstdint>

#include "../../include/isim.h"
#include "host_device.h"

namespace isim {
namespace sk {

constexpr uint32_t kMaxSubBits = ISIM_SK_MAX_SUB_BITS;

__host__ __device__ inline uint32_t bins(uint32_t s) { return (65u - s) << s; }

// bits needed to write v (0 for 0)
__host__ __device__ inline uint32_t bitlen(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }

// The bin of v: v itself below 2^(s+1); above, the top s + 1 bits of v (the
// leading 1 and s more) select the bin inside the octave `shift`.  At
// v = 2^(s+1), shift is 1 and v >> 1 is 2^s: bin 2^(s+1), so the rule is
// continuous; 2^64 - 1 gives ((63 - s) << s) + 2^(s+1) - 1 = bins(s) - 1.
__host__ __device__ inline uint32_t bucket(uint32_t s, uint64_t v) {
  if (v < (2ull << s)) return (uint32_t)v;
  const uint32_t shift = bitlen(v) - (s + 1u);
  return (shift << s) + (uint32_t)(v >> shift);
}

// [lo, hi] of a bin below bins(s): hi - lo = 2^shift - 1 < 2^shift <= lo >> s
__host__ __device__ inline void bounds(uint32_t s, uint32_t bin, uint64_t &lo, uint64_t &hi) {
  if (bin < (2u << s)) {
    lo = hi = bin;
    return;
  }
  const uint32_t shift = (bin >> s) - 1u;
  lo = (uint64_t)((1u << s) + (bin & ((1u << s) - 1u))) << shift;
  hi = lo + ((1ull << shift) - 1ull);
}

}  // namespace sk
}  // namespace isim
