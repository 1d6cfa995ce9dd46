// Per-service exact percentiles over time (include/isim.h
// isim_service_window_quantiles*), one header for
// service_window_quantiles.cpp (host) and service_window_quantiles.hip (host
// and device): the cell of a span, the layout of the table and of the device
// call's workspace, and the host's fold.  The span rule is service_timeline.h's,
// the rows are timeline_row.h's, the measures, the classes and the fold per
// segment are service_quantiles.h's: a cell (service, row) is a segment.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/isim.h"
#include "service_quantiles.h"
#include "service_timeline.h"
#include "timeline_row.h"

namespace isim {
namespace swq {

using svq::kClasses;
using svq::kMeasures;
using svq::kNone;
using svq::kStage;
// a segment of at most kWave spans is ranked by one wave in registers.  ISIM_SWQ_VARIANT_WAVE is for a
// measuring build only (tools/build_variant.sh): 64, 128 or 256.
#ifdef ISIM_SWQ_VARIANT_WAVE
constexpr uint32_t kWave = ISIM_SWQ_VARIANT_WAVE;
#else
constexpr uint32_t kWave = ISIM_SWQ_WAVE;
#endif
static_assert(kWave == 64 || kWave == 128 || kWave == 256, "1, 2 or 4 keys per lane");
constexpr uint64_t kMaxCells = ISIM_SWQ_MAX_CELLS;  // the key 2 * cell + code stays below 2^21

using RowArgs = svt::RowArgs;

// the cell of a span that is not refused: its service's row of the finish time
template <typename A>
ISIM_TL_FN uint32_t cell_at(const A &a, uint32_t service, uint64_t finish) {
  return service * (a.n_windows + 2u) + tl::row_of(a, finish);
}
// ... and of any span; kNone: refused
template <typename A>
ISIM_TL_FN uint32_t cell_of(const A &a, uint32_t n_services, uint64_t arrival, uint64_t start, uint64_t finish,
                            uint32_t service) {
  if (svt::span_refused(n_services, arrival, start, finish, service)) return kNone;
  return cell_at(a, service, finish);
}

inline uint64_t cells_of(uint64_t n_services, uint32_t n_windows) { return svt::cells_of(n_services, n_windows); }
// the table: u64 [n_services][n_windows + 2][kMeasures][kClasses][1 + n_q], then the header
inline uint64_t table_words(uint64_t cells, uint32_t n_q) { return svq::table_words(cells, n_q); }

// The device call's workspace (byte offsets): service_quantiles.h's with a cell for a service, and between the
// cursors and the measures the list of the cells the LDS tier selects (more than kWave spans, at most kStage),
// of which cap / (kWave + 1) can exist and no more than there are cells.
struct Layout {
  uint64_t counters;  // 2 * cells
  uint64_t cnt, off, cur, mid, seg, slots, bins, total;
  uint64_t n_mid, n_slots, slot_bins;
};
inline Layout layout(uint64_t cells, uint64_t cap, uint32_t n_q) {
  Layout l{};
  l.counters = 2 * cells;
  const uint64_t cbytes = (l.counters * 4 + 255) & ~255ull;
  l.cnt = svq::kHeadBytes;
  l.off = l.cnt + cbytes;
  l.cur = l.off + cbytes;
  l.mid = l.cur + cbytes;
  l.n_mid = std::min<uint64_t>(cells, cap / (kWave + 1ull));
  l.seg = l.mid + ((l.n_mid * 4 + 255) & ~255ull);
  l.slots = l.seg + (uint64_t)kMeasures * cap * 8;
  l.n_slots = std::min<uint64_t>(cells, cap / (kStage + 1ull));
  l.slot_bins = (uint64_t)kMeasures * kClasses * n_q * 256;
  l.bins = l.slots + l.n_slots * svq::kSlotBytes;
  l.total = l.bins + l.n_slots * l.slot_bins * 4;
  return l;
}

// ---- the host's fold (isim_service_window_quantiles_host).  WRITES every word of out [table_words(cells, n_q)].
inline void fold_host(const RowArgs &a, uint32_t n_services, const uint32_t *q_ppm, uint32_t n_q,
                      const isim_des_span *spans, uint64_t n, uint64_t *out) {
  svq::fold_segments(cells_of(n_services, a.n_windows), q_ppm, n_q, spans, n, out, [&](const isim_des_span &s) {
    return cell_of(a, n_services, s.arrival_ns, s.start_ns, s.finish_ns, s.service);
  });
}

// ---- host side (service_window_quantiles.cpp): svq::check_sizes or svq::check (q_ppm checked: with_list),
// the parameters and the cells' bound; n_services and the cells on success
int check(const isim_handler *h, const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q, bool with_list,
          uint64_t n_spans, uint64_t &n_services, uint64_t &cells);

// ---- device side (service_window_quantiles.hip): the launches of one checked call
int launch(uint32_t n_services, const isim_timeline_params &p, const uint32_t *q_ppm, uint32_t n_q,
           const uint64_t *d_off, const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
           uint64_t *d_out, void *d_workspace, void *stream);

}  // namespace swq
}  // namespace isim
