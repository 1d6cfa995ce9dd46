// An isim_trace_rec (include/isim.h) as the kernels that read records see it:
// one 16-byte load and the fields taken from its words.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace isim {
namespace dev {

typedef uint32_t rec4 __attribute__((ext_vector_type(4)));  // latency lo, hi, hops, status_err

// record i, or zeros for a lane past the end
__device__ __forceinline__ rec4 load_rec(const rec4 *__restrict__ rec, uint64_t i, bool live = true) {
  rec4 r = live ? rec[i] : rec4{0, 0, 0, 0};
  asm volatile("" : "+v"(r));  // all four words stay live: the record is one 16-byte load (hops is unused)
  return r;
}

__device__ __forceinline__ uint64_t latency(rec4 r) { return (uint64_t)r.x | ((uint64_t)r.y << 32); }

// 0: a 200, 1: a 500
__device__ __forceinline__ uint32_t code(rec4 r) { return r.w >> 31; }

// arrival + latency, saturating
__device__ __forceinline__ uint64_t completion(uint64_t arrival, uint64_t lat) {
  const uint64_t c = arrival + lat;
  return c < arrival ? ~0ull : c;
}

}  // namespace dev
}  // namespace isim
