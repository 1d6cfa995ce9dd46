// The row arithmetic of the timeline tables (include/isim.h isim_timeline_params,
// DESIGN.md §14), shared by timeline.hip and timeline_quantiles.hip: the
// parameter rules, the exact u64 division by the window and the row of a time.
// service_timeline.h reads it on the host as well.
#pragma once

#include <cstdint>

#include "../../include/isim.h"
#include "host_device.h"

#if defined(__HIPCC__)
#define ISIM_TL_FN __host__ __device__ __forceinline__
#else
#define ISIM_TL_FN inline
#endif

namespace isim {
namespace tl {

static_assert(ISIM_TL_MAX_WINDOWS == 65536u, "the message below names the limit");

// the rule an isim_timeline_params breaks, or nullptr
inline const char *params_error(const isim_timeline_params *p) {
  if (!p) return "null isim_timeline_params";
  if (p->window_ns == 0) return "window_ns must be at least 1";
  if (p->n_windows == 0 || p->n_windows > ISIM_TL_MAX_WINDOWS) return "n_windows must be 1..65536";
  if (p->reserved != 0) return "isim_timeline_params.reserved must be 0";
  return nullptr;
}

// floor(x / d) for every u64 x with m = floor((2^64 - 1) / d): the estimate
// q' = mulhi(x, m) satisfies x/d - 1 < x m / 2^64 <= x/d (m >= (2^64 - d) / d
// and x < 2^64), so q' is q or q - 1 and the remainder x - q' d lies in
// [0, 2 d): one correction (the second never fires; it costs two VALU).
__host__ __device__ inline uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
__host__ __device__ inline uint64_t div_recip(uint64_t x, uint64_t d, uint64_t m) {
  uint64_t q = mulhi64(x, m);
  uint64_t r = x - q * d;
  if (r >= d) {
    ++q;
    r -= d;
  }
  if (r >= d) ++q;
  return q;
}

// The row fields of a kernel's argument struct A (t0, window, recip = floor((2^64 - 1) / window),
// n_windows, and for a power-of-two window pow2 = 1 and shift = its log2) from valid parameters.
template <typename A>
inline void set_row_args(A &a, const isim_timeline_params &p) {
  a.t0 = p.t0_ns;
  a.window = p.window_ns;
  a.recip = ~0ull / p.window_ns;
  a.n_windows = p.n_windows;
  a.pow2 = (p.window_ns & (p.window_ns - 1)) == 0 ? 1u : 0u;
  a.shift = a.pow2 ? (uint32_t)__builtin_ctzll(p.window_ns) : 0u;
}

// the table row of time x: 0 before t0, 1 + w for window w, n_windows + 1 after the last
template <typename A>
ISIM_TL_FN uint32_t row_of(const A &a, uint64_t x) {
  if (x < a.t0) return 0u;
  const uint64_t d = x - a.t0;
  const uint64_t w = a.pow2 ? d >> a.shift : div_recip(d, a.window, a.recip);
  return 1u + (uint32_t)(w < a.n_windows ? w : a.n_windows);
}

}  // namespace tl
}  // namespace isim
