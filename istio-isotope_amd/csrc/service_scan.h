// The offset scan over the counts per (service, code) of a tapped batch's spans,
// device only: what service_quantiles.hip and service_sketch.hip
// (§30) launch between span_segments.h's k_svq_count and k_svq_scatter.  The
// segments of more than LONG_ABOVE spans are the long ones: §28's are those the
// LDS select cannot stage, §30's those that pay for a table in LDS.
#pragma once

#include "span_segments.h"

namespace isim {
namespace svq {

constexpr uint32_t kScanThreads = 1024;

// One workgroup, a service per thread and tile: the exclusive scan of the counts into the segment offsets and
// the scatter cursors; the long segments get a slot each, in service order, and the first of their chunks.
// The counts are of at most cap spans, so no more than n_slots segments are long.
template <uint32_t LONG_ABOVE>
static __global__ __launch_bounds__(kScanThreads) void k_svq_scan(const uint32_t *__restrict__ cnt,
                                                                 uint32_t *__restrict__ off, uint32_t *__restrict__ cur,
                                                                 uint32_t n_services, Slot *slots, uint32_t n_slots,
                                                                 Head *head) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t c_elem = 0, c_long = 0, c_chunk = 0;
  for (uint32_t tile = 0; tile < n_services; tile += kScanThreads) {
    const uint32_t s = tile + t;
    const bool live = s < n_services;
    const uint32_t n200 = live ? cnt[2 * s] : 0u, n500 = live ? cnt[2 * s + 1] : 0u;
    const uint32_t n = n200 + n500;
    const bool is_long = n > LONG_ABOVE;
    uint32_t t_elem, t_long, t_chunk;
    const uint32_t e = c_elem + rs::block_scan<kScanThreads>(n, s_wave, lane, wave, t_elem);
    const uint32_t l = c_long + rs::block_scan<kScanThreads>(is_long ? 1u : 0u, s_wave, lane, wave, t_long);
    const uint32_t c =
        c_chunk + rs::block_scan<kScanThreads>(is_long ? (n - 1) / kChunk + 1 : 0u, s_wave, lane, wave, t_chunk);
    if (live) {
      off[2 * s] = cur[2 * s] = e;
      off[2 * s + 1] = cur[2 * s + 1] = e + n200;
      if (is_long && l < n_slots) {
        Slot &x = slots[l];
        x.svc = s;
        x.chunk0 = c;
        x.n200 = n200;
        x.n500 = n500;
        x.off = e;
        for (uint32_t m = 0; m < kMeasures; ++m) x.any[m] = 0;
      }
    }
    c_elem += t_elem;
    c_long += t_long;
    c_chunk += t_chunk;
  }
  if (t == 0) {
    const bool fits = c_long <= n_slots;  // always, for counts of at most cap spans
    head->n_long = fits ? c_long : 0u;
    head->n_chunks = fits ? c_chunk : 0u;
  }
}

}  // namespace svq
}  // namespace isim
