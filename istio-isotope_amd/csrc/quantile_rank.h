// The nearest-rank rule and the quantile-list rules of the exact percentiles
// (include/isim.h isim_quantile_rank), shared by quantile.hip,
// timeline_quantiles.hip and, built by the host compiler, sketch.cpp.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "host_device.h"

namespace isim {
namespace q {

// 1-based nearest rank: max(1, ceil(q_ppm * n / 1e6))
__host__ __device__ inline uint64_t nearest_rank(uint64_t n, uint32_t q_ppm) {
  // n <= 2^40, q_ppm <= 10^6 < 2^20: the product stays below 2^60
  const uint64_t k = (n * (uint64_t)q_ppm + 999999ull) / 1000000ull;
  return k ? k : 1;
}

// the rule a quantile list breaks (empty: none)
inline std::string list_error(const uint32_t *q_ppm, uint32_t n_q) {
  if (n_q == 0 || n_q > ISIM_MAX_QUANTILES) return "n_q must be 1.." + std::to_string(ISIM_MAX_QUANTILES);
  if (!q_ppm) return "null q_ppm";
  for (uint32_t i = 0; i < n_q; ++i)
    if (q_ppm[i] > 1000000u) return "q_ppm[" + std::to_string(i) + "] is above 1000000";
  return std::string();
}

}  // namespace q
}  // namespace isim
