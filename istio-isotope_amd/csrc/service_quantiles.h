// Per-service exact percentiles of queue wait, service time and duration
// (include/isim.h isim_service_quantiles*), one header for
// service_quantiles.cpp (host) and service_quantiles.hip (host and device): the
// span rule (service_timeline.h's own), the three measures of a span, the
// layout of the table and of the device call's workspace, and the host's fold.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/isim.h"
#include "quantile_rank.h"
#include "service_timeline.h"

namespace isim {
namespace svq {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMeasures = ISIM_SVQ_MEASURES;
constexpr uint32_t kClasses = ISIM_SVQ_CLASSES;
constexpr uint32_t kStage = ISIM_SVQ_STAGE;  // a segment of at most this many spans is selected in LDS
// elements of a long segment one workgroup histograms per digit.  ISIM_SVQ_VARIANT_CHUNK is for a measuring build
// only (tools/build_variant.sh): 1 << 30 makes every long segment one chunk, one workgroup per segment and measure.
#ifdef ISIM_SVQ_VARIANT_CHUNK
constexpr uint32_t kChunk = ISIM_SVQ_VARIANT_CHUNK;
#else
constexpr uint32_t kChunk = ISIM_SVQ_CHUNK;
#endif
constexpr uint64_t kMaxSpans = ISIM_SVQ_MAX_SPANS;
constexpr uint32_t kMaxServices = 1u << 30;  // the key 2 * service + code stays below kNone
constexpr uint64_t kHeadBytes = 256;         // the ticket and the long segments' totals
constexpr uint64_t kSlotBytes = ISIM_SVQ_SLOT_BYTES;  // a long segment's record and select states (service_quantiles.hip)

// the span rule is §23's
using svt::span_refused;

// measure m of a span that is not refused
ISIM_TL_FN uint64_t measure(uint32_t m, uint64_t arrival, uint64_t start, uint64_t finish) {
  return m == ISIM_SVQ_WAIT ? start - arrival : m == ISIM_SVQ_SERVICE ? finish - start : finish - arrival;
}

// the table: u64 [n_services][kMeasures][kClasses][1 + n_q], then the header
inline uint64_t cell_words(uint32_t n_q) { return 1ull + n_q; }
inline uint64_t table_words(uint64_t n_services, uint32_t n_q) {
  return n_services * kMeasures * kClasses * cell_words(n_q) + ISIM_SVQ_HEADER_WORDS;
}

// The device call's workspace (byte offsets).  Per service: three u32 arrays of one word per (service, code)
// (counts, segment offsets, scatter cursors), each padded to 256 B.  Per span: the three measures, u64 each,
// scattered by service.  Per long segment, of which cap / (kStage + 1) can exist and no more than there are
// services: kSlotBytes of state and the u32 bins [kMeasures][kClasses][n_q][256].
struct Layout {
  uint64_t counters;  // 2 * n_services
  uint64_t cnt, off, cur, seg, slots, bins, total;
  uint64_t n_slots, slot_bins;  // slot_bins: u32 words of one slot's bins
};
inline Layout layout(uint64_t n_services, uint64_t cap, uint32_t n_q) {
  Layout l{};
  l.counters = 2 * n_services;
  const uint64_t cbytes = (l.counters * 4 + 255) & ~255ull;
  l.cnt = kHeadBytes;
  l.off = l.cnt + cbytes;
  l.cur = l.off + cbytes;
  l.seg = l.cur + cbytes;
  l.slots = l.seg + (uint64_t)kMeasures * cap * 8;
  l.n_slots = std::min<uint64_t>(n_services, cap / (kStage + 1ull));
  l.slot_bins = (uint64_t)kMeasures * kClasses * n_q * 256;
  l.bins = l.slots + l.n_slots * kSlotBytes;
  l.total = l.bins + l.n_slots * l.slot_bins * 4;
  return l;
}

// ---- the host's fold of spans into segments of a table [n_segments][kMeasures][kClasses][1 + n_q] and its
// header: segment_of(span) is the span's segment, kNone for a refused one; a sort per segment, measure and
// class.  WRITES every word of out [n_segments * kMeasures * kClasses * (1 + n_q) + ISIM_SVQ_HEADER_WORDS].
template <typename SegmentOf>
inline void fold_segments(uint64_t n_segments, const uint32_t *q_ppm, uint32_t n_q, const isim_des_span *spans,
                          uint64_t n, uint64_t *out, SegmentOf segment_of) {
  const uint64_t ow = cell_words(n_q), words = table_words(n_segments, n_q);
  for (uint64_t i = 0; i < words; ++i) out[i] = 0;
  uint64_t *hdr = out + words - ISIM_SVQ_HEADER_WORDS;
  // spans per (segment, code), then their indices by (segment, code)
  std::vector<uint64_t> off(2 * n_segments + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const isim_des_span &s = spans[i];
    const uint32_t g = segment_of(s);
    if (g == kNone) {
      hdr[ISIM_SVQ_H_REFUSED] += 1;
      continue;
    }
    hdr[ISIM_SVQ_H_FOLDED] += 1;
    off[2 * (uint64_t)g + (s.status & 1u) + 1] += 1;
  }
  for (uint64_t k = 0; k < 2 * n_segments; ++k) off[k + 1] += off[k];
  std::vector<uint64_t> cur(off.begin(), off.end() - 1), idx(hdr[ISIM_SVQ_H_FOLDED]);
  for (uint64_t i = 0; i < n; ++i) {
    const isim_des_span &s = spans[i];
    const uint32_t g = segment_of(s);
    if (g != kNone) idx[cur[2 * (uint64_t)g + (s.status & 1u)]++] = i;
  }
  std::vector<uint64_t> v;
  for (uint64_t s = 0; s < n_segments; ++s) {
    // the class's elements of the segment: all, its 200s, its 500s
    const uint64_t lo[kClasses] = {off[2 * s], off[2 * s], off[2 * s + 1]};
    const uint64_t hi[kClasses] = {off[2 * s + 2], off[2 * s + 1], off[2 * s + 2]};
    for (uint32_t m = 0; m < kMeasures; ++m)
      for (uint32_t c = 0; c < kClasses; ++c) {
        const uint64_t n_c = hi[c] - lo[c];
        if (!n_c) continue;
        v.resize(n_c);
        for (uint64_t i = 0; i < n_c; ++i) {
          const isim_des_span &x = spans[idx[lo[c] + i]];
          v[i] = measure(m, x.arrival_ns, x.start_ns, x.finish_ns);
        }
        std::sort(v.begin(), v.end());
        uint64_t *cell = out + ((s * kMeasures + m) * kClasses + c) * ow;
        cell[0] = n_c;
        for (uint32_t i = 0; i < n_q; ++i) cell[1 + i] = v[q::nearest_rank(n_c, q_ppm[i]) - 1];
      }
  }
}

// isim_service_quantiles_host, and tests/cpp/service_quantiles_check.cpp under the sanitizers: a segment per
// service.  WRITES every word of out [table_words(n_services, n_q)].
inline void fold_host(uint32_t n_services, const uint32_t *q_ppm, uint32_t n_q, const isim_des_span *spans, uint64_t n,
                      uint64_t *out) {
  fold_segments(n_services, q_ppm, n_q, spans, n, out, [n_services](const isim_des_span &s) {
    return span_refused(n_services, s.arrival_ns, s.start_ns, s.finish_ns, s.service) ? kNone : s.service;
  });
}

// ---- host side (service_quantiles.cpp): the handler, the number of quantiles and the span bound, and with
// them the quantile list; n_services on success
int check_sizes(const isim_handler *h, uint32_t n_q, uint64_t n_spans, uint64_t &n_services);
int check(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q, uint64_t n_spans, uint64_t &n_services);

// ---- device side (service_quantiles.hip): the launches of one checked call
int launch(uint32_t n_services, const uint32_t *q_ppm, uint32_t n_q, const uint64_t *d_off,
           const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_out,
           void *d_workspace, void *stream);

}  // namespace svq
}  // namespace isim
