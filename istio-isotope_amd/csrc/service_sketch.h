// Per-service latency sketch (include/isim.h isim_service_sketch*, DESIGN.md
// §30), one header for service_sketch.cpp (host) and service_sketch.hip (host
// and device): the layout of the table and of the device call's workspace, the
// word of a span's measure, the host's fold and the checks.  The span rule and
// the three measures are service_quantiles.h's (§28), the bucket rule is
// sketch_bucket.h's (§16).
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/isim.h"
#include "service_quantiles.h"
#include "sketch_bucket.h"

namespace isim {
namespace svs {

using svq::kMeasures;
constexpr uint32_t kShort = ISIM_SVS_SHORT;  // a segment of at most this many spans is added by one wave
constexpr uint64_t kMaxWords = ISIM_SVS_MAX_WORDS;
static_assert(kShort >= 1 && kShort <= svq::kChunk, "a short segment is below one chunk");

// the table: u64 [n_services][kMeasures][2][bins(s)], then the header
ISIM_TL_FN uint64_t block_words(uint32_t s) { return 2ull * sk::bins(s); }
ISIM_TL_FN uint64_t table_words(uint64_t n_services, uint32_t s) {
  return n_services * kMeasures * block_words(s) + ISIM_SVQ_HEADER_WORDS;
}
// the word of value v of measure m of a span of `service` with `code`
ISIM_TL_FN uint64_t word_of(uint32_t s, uint32_t service, uint32_t m, uint32_t code, uint64_t v) {
  return (((uint64_t)service * kMeasures + m) * 2u + code) * sk::bins(s) + sk::bucket(s, v);
}

// The device call's workspace (byte offsets): §28's head, counts, offsets, cursors and scattered measures; per
// long segment (more than kShort spans), of which cap / (kShort + 1) can exist and no more than there are
// services, one svq slot.  No bins: the long tier's are in LDS.
struct Layout {
  uint64_t counters;  // 2 * n_services
  uint64_t cnt, off, cur, seg, slots, total;
  uint64_t n_slots;
};
inline Layout layout(uint64_t n_services, uint64_t cap) {
  Layout l{};
  l.counters = 2 * n_services;
  const uint64_t cbytes = (l.counters * 4 + 255) & ~255ull;
  l.cnt = svq::kHeadBytes;
  l.off = l.cnt + cbytes;
  l.cur = l.off + cbytes;
  l.seg = l.cur + cbytes;
  l.slots = l.seg + (uint64_t)kMeasures * cap * 8;
  l.n_slots = std::min<uint64_t>(n_services, cap / (kShort + 1ull));
  l.total = l.slots + l.n_slots * svq::kSlotBytes;
  return l;
}

// isim_service_sketch_host, and tests/cpp/service_sketch_check.cpp under the sanitizers.  ADDS into
// table [table_words(n_services, s)], the header included; only the words it hits are touched.
inline void fold_host(uint32_t n_services, uint32_t s, const isim_des_span *spans, uint64_t n, uint64_t *table) {
  uint64_t *hdr = table + table_words(n_services, s) - ISIM_SVQ_HEADER_WORDS;
  for (uint64_t i = 0; i < n; ++i) {
    const isim_des_span &x = spans[i];
    if (svq::span_refused(n_services, x.arrival_ns, x.start_ns, x.finish_ns, x.service)) {
      hdr[ISIM_SVQ_H_REFUSED] += 1;
      continue;
    }
    hdr[ISIM_SVQ_H_FOLDED] += 1;
    for (uint32_t m = 0; m < kMeasures; ++m)
      table[word_of(s, x.service, m, x.status & 1u, svq::measure(m, x.arrival_ns, x.start_ns, x.finish_ns))] += 1;
  }
}

// ---- host side (service_sketch.cpp): the handler, sub_bits, the span bound and the table's bound;
// n_services on success
int check_sizes(const isim_handler *h, uint32_t sub_bits, uint64_t n_spans, uint64_t &n_services);

// ---- device side (service_sketch.hip): the launches of one checked call
int launch(uint32_t n_services, uint32_t sub_bits, const uint64_t *d_off, const isim_des_span *d_spans,
           uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_table, void *d_workspace, void *stream);

}  // namespace svs
}  // namespace isim
