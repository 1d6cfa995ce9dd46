// Service timeline (include/isim.h isim_service_timeline*), one
// header for service_timeline.cpp (host) and service_timeline.hip (host and
// device): what one isim_des_span adds to the (service x window) table.  The
// rows are timeline_row.h's.  span_updates turns a span into cells and values,
// the same on both sides; the host adds them one by one, the device adds them
// up across a wave first.  The interior rows of an interval are never walked:
// they are all whole windows, so a span adds +1 and -1 to a cover-difference
// array and one prefix sum per service (finish) turns the covers into time.
#pragma once

#include <cstdint>

#include "../../include/isim.h"
#include "timeline_row.h"

namespace isim {
namespace svt {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kW = ISIM_SVT_ROW_WORDS;
constexpr uint64_t kMaxSpans = 1ull << 40;
static_assert((uint64_t)ISIM_SVT_MAX_CELLS * kW < (1ull << 31), "word indices fit 32 bits");

// the row fields timeline_row.h's set_row_args fills and row_of reads
struct RowArgs {
  uint64_t t0, window, recip;
  uint32_t n_windows, shift, pow2;
};

// [x, y) cut at the rows: `head` goes to row r0 and, when the interval leaves r0, `tail` to row r1 > r0;
// the rows strictly between are covered whole
struct Parts {
  uint32_t r0, r1;
  uint64_t head, tail;
};
// x < y.  The last instant of the interval, y - 1, names r1, so an interval that ends on a window's edge
// stays out of the next row.  r0 < r1: the instants t0 + r0 W (the end of r0; t0 for "before") and
// t0 + (r1 - 1) W (the begin of r1) both lie in [x, y - 1], so r0 W and (r1 - 1) W are at most y - 1 - t0:
// nothing wraps, and t0 + n_windows W is not formed.
template <typename A>
ISIM_TL_FN Parts parts_of(const A &a, uint64_t x, uint64_t y) {
  Parts p;
  p.r0 = tl::row_of(a, x);
  p.r1 = tl::row_of(a, y - 1);
  p.head = y - x;
  p.tail = 0;
  if (p.r0 != p.r1) {
    p.head = p.r0 == 0 ? a.t0 - x : (uint64_t)p.r0 * a.window - (x - a.t0);
    p.tail = (y - a.t0) - (uint64_t)(p.r1 - 1) * a.window;
  }
  return p;
}

// an interval of service s as cells (s * rows + row): the head's and the tail's cell, and the two cells of
// the cover difference (+1 at c0, -1 at c1); kNone where there is none
struct Interval {
  uint32_t k0 = kNone, k1 = kNone, c0 = kNone, c1 = kNone;
  uint64_t head = 0, tail = 0;
};
template <typename A>
ISIM_TL_FN Interval interval_of(const A &a, uint32_t base, uint64_t x, uint64_t y) {
  Interval v;
  if (x >= y) return v;
  const Parts p = parts_of(a, x, y);
  v.k0 = base + p.r0;
  v.head = p.head;
  if (p.r1 != p.r0) {
    v.k1 = base + p.r1;
    v.tail = p.tail;
    if (p.r1 - p.r0 > 1) {
      v.c0 = base + p.r0 + 1;
      v.c1 = base + p.r1;
    }
  }
  return v;
}

// everything one span adds
struct Upd {
  uint32_t ka = kNone, ks = kNone, kf = kNone;  // the cells of a, S and F; all kNone: refused
  uint32_t code = 0;
  uint64_t wait = 0;
  Interval q, b;  // [a, S) and [S, S + P_s)
};
// the span rule (also service_quantiles.h's): refused if the service is out of range or a <= S <= F does not hold
ISIM_TL_FN bool span_refused(uint32_t n_services, uint64_t arrival, uint64_t start, uint64_t finish, uint32_t service) {
  return service >= n_services || arrival > start || start > finish;
}

// hold: P_s per service.  A refused span (span_refused) yields the empty Upd.
template <typename A>
ISIM_TL_FN Upd span_updates(const A &a, uint32_t n_services, const uint64_t *hold, uint64_t arrival, uint64_t start,
                            uint64_t finish, uint32_t service, uint32_t status) {
  Upd u;
  if (span_refused(n_services, arrival, start, finish, service)) return u;
  const uint32_t base = service * (a.n_windows + 2u);
  u.ka = base + tl::row_of(a, arrival);
  u.ks = base + tl::row_of(a, start);
  u.kf = base + tl::row_of(a, finish);
  u.code = status & 1u;
  u.wait = start - arrival;
  u.q = interval_of(a, base, arrival, start);
  const uint64_t p = hold[service];
  u.b = interval_of(a, base, start, start + p < start ? ~0ull : start + p);
  return u;
}

// cells of a table, workspace of the device call: the two cover-difference planes (queued, busy), u64 each
inline uint64_t cells_of(uint64_t n_services, uint32_t n_windows) { return n_services * ((uint64_t)n_windows + 2); }
inline uint64_t table_words(uint64_t cells) { return (cells + 1) * kW; }
inline uint64_t ws_bytes(uint64_t cells) { return cells * 16 < 64 ? 64 : cells * 16; }

// ---- the host's fold (isim_service_timeline_host, and tests/cpp/service_timeline_check.cpp under the
// sanitizers).  ADDS into table [table_words(cells)]; cover: 2 * cells words, zeroed here.
inline void fold_host(const RowArgs &a, uint32_t n_services, const uint64_t *hold, const isim_des_span *spans,
                      uint64_t n, uint64_t *table, uint64_t *cover) {
  const uint64_t cells = cells_of(n_services, a.n_windows);
  for (uint64_t i = 0; i < 2 * cells; ++i) cover[i] = 0;
  uint64_t *hdr = table + cells * kW;
  auto word = [&](uint32_t cell, uint32_t w) -> uint64_t & { return table[(uint64_t)cell * kW + w]; };
  for (uint64_t i = 0; i < n; ++i) {
    const isim_des_span &s = spans[i];
    const Upd u = span_updates(a, n_services, hold, s.arrival_ns, s.start_ns, s.finish_ns, s.service, s.status);
    if (u.ka == kNone) {
      hdr[ISIM_SVT_H_REFUSED] += 1;
      continue;
    }
    hdr[ISIM_SVT_H_FOLDED] += 1;
    word(u.ka, ISIM_SVT_ARRIVED) += 1;
    word(u.ks, ISIM_SVT_STARTED) += 1;
    word(u.ks, ISIM_SVT_SUM_WAIT) += u.wait;
    if (u.wait > word(u.ks, ISIM_SVT_MAX_WAIT)) word(u.ks, ISIM_SVT_MAX_WAIT) = u.wait;
    word(u.kf, ISIM_SVT_FINISHED + u.code) += 1;
    const Interval *iv[2] = {&u.q, &u.b};
    for (uint32_t k = 0; k < 2; ++k) {
      const Interval &v = *iv[k];
      const uint32_t w = k ? ISIM_SVT_BUSY_NS : ISIM_SVT_QUEUED_NS;
      if (v.k0 != kNone) word(v.k0, w) += v.head;
      if (v.k1 != kNone) word(v.k1, w) += v.tail;
      if (v.c0 != kNone) {
        cover[k * cells + v.c0] += 1;
        cover[k * cells + v.c1] -= 1;
      }
    }
  }
  // finish: per service and plane the running sum of the differences is the number of spans that cover the row whole
  const uint32_t rows = a.n_windows + 2u;
  for (uint32_t k = 0; k < 2; ++k)
    for (uint32_t s = 0; s < n_services; ++s) {
      uint64_t run = 0;
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t cell = s * rows + r;
        run += cover[k * cells + cell];
        word(cell, k ? ISIM_SVT_BUSY_NS : ISIM_SVT_QUEUED_NS) += run * a.window;
      }
    }
}

// ---- host side: every check of a handler that needs no GPU (handler.h has the handler; des_host.hip: what
// isim_serve_des_spans_device refuses with a tap); ISIM_OK or ISIM_EINVAL
int check_handler(const isim_handler *h);
// ... and of the parameters and the table's size (service_timeline.cpp); the cells of the table on success
int check(const isim_handler *h, const isim_timeline_params *p, uint64_t &cells);

// ---- device side (service_timeline.hip): the launches of one checked call
int launch(const isim_handler *h, const isim_timeline_params &p, const uint64_t *d_off, const isim_des_span *d_spans,
           uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_table, void *d_workspace, void *stream);

}  // namespace svt
}  // namespace isim
