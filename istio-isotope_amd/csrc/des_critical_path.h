// Critical path of DES trace spans (include/isim.h isim_des_critical_path*,
// DESIGN.md §22), one header for des_critical_path.cpp (host) and
// des_critical_path.hip (host and device): the fold of one trace's
// isim_des_span records in phases of independent spans.  The script walk is
// critical_path.h's replay_script; the DES spans supply a child's value
// (hop_ns + finish - arrival), check its arrival against the caller's clock and
// write nothing.  The host runs every phase as a loop over the spans; the device
// runs one trace per wave, lanes striding over the spans, a barrier between
// phases.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/isim.h"
#include "critical_path.h"

namespace isim {
namespace dcp {

constexpr uint32_t kNone = cp::kNone;
constexpr uint32_t kWinner = 1u;  // Link::flags: a local winner of its caller

// the workspace of one span: its next sibling, its flags, the sum of H + dur over its local-winner children
struct Link {
  uint32_t next, flags;
  uint64_t won;
};
static_assert(sizeof(Link) == 16, "16 bytes per span of the buffer");

// workspace of isim_des_critical_path_device: the entry counter, then a Link per span of the buffer
constexpr uint64_t kWsHead = 64;
inline uint64_t ws_bytes(uint64_t cap_spans) { return kWsHead + cap_spans * sizeof(Link); }

constexpr uint32_t kHdrWords = 5;

// the table on the host: plain adds
struct HostAcc {
  uint64_t *table;
  uint32_t n_services;
  void add(uint32_t row, uint32_t word, uint64_t v) { table[(uint64_t)row * ISIM_DCP_ROW_WORDS + word] += v; }
  void hdr(uint32_t word, uint64_t v) { add(n_services, word, v); }
};

// One trace: m spans at s, m links at w.  Every phase handles one span and touches only what the phase's
// comment names, so the spans of a phase run in any order or side by side; a phase reads what earlier phases
// wrote.  Every index read from a span or a link is bounded where it is used: memory safety does not depend
// on the spans being a tap's.
template <class KOf>
struct Fold {
  cp::ScriptView v;
  KOf kof;
  isim_des_span *s = nullptr;
  Link *w = nullptr;  // set by the caller after begin(): the links of this trace
  uint64_t base = 0;  // the trace's first span in the buffer
  uint32_t m = 0;

  // spans [off[i], off[i + 1]) of a buffer of `cap` spans; false: the offsets refuse the trace
  ISIM_TW bool begin(const uint64_t *off, uint64_t i, uint64_t cap, isim_des_span *spans) {
    const uint64_t a = off[i], b = off[i + 1];
    if (b <= a || b > cap || b - a > cp::kMaxTraceSpans) return false;
    s = spans + a;
    base = a;
    m = (uint32_t)(b - a);
    return true;
  }

  // Phase 0, read-only: span j is one of a tap's.  Preorder: the caller of j is j - 1 or one of its ancestors.
  ISIM_TW bool check(uint32_t j) const {
    const isim_des_span &q = s[j];
    if (q.hop != j || q.position >= v.n_positions || q.service >= v.n_services) return false;
    if (q.arrival_ns > q.start_ns || q.start_ns > q.finish_ns) return false;
    if (j == 0) return q.caller_hop == kNone && q.hop_ns == 0;  // (a hop cost of the entry would break the identity)
    const uint32_t c = q.caller_hop;
    if (c >= j) return false;
    uint32_t a = j - 1;
    while (a > c) {  // up the callers of j - 1: strictly descending whatever the spans hold
      const uint32_t n = s[a].caller_hop;
      if (n >= a) return false;
      a = n;
    }
    return a == c;
  }

  // Phase 1, writes w[j].next and w[j].flags: the next sibling of j is the first later span whose caller is
  // no deeper than j's, if it has j's caller (preorder).  The first child of j is j + 1 iff its caller is j.
  ISIM_TW void link(uint32_t j) {
    const uint32_t c = s[j].caller_hop;
    uint32_t n = kNone;
    if (j)
      for (uint32_t x = j + 1; x < m; ++x) {
        const uint32_t cx = s[x].caller_hop;
        if (cx <= c) {
          if (cx == c) n = x;
          break;
        }
      }
    w[j].next = n;
    w[j].flags = 0;
  }

  // a chain of siblings ascends in hop, so it ends after at most m links whatever the links hold
  ISIM_TW uint32_t next(uint32_t c) const {
    const uint32_t n = w[c].next;
    return n > c && n < m ? n : kNone;
  }

  // the children of one caller as replay_script takes them: nothing is written to a span, the arrival of a
  // matched child is checked against the clock of its call, a local winner is flagged in its link
  struct Kids {
    Fold &f;
    uint32_t child;
    bool bad;
    ISIM_TW bool more() const { return child != kNone; }
    ISIM_TW uint32_t take(uint32_t k, uint64_t at, uint64_t &val) {
      val = 0;
      if (child == kNone) return kNone;
      const isim_des_span &q = f.s[child];
      if (q.position >= f.v.n_positions || f.kof(q.position) != k) return kNone;
      const uint32_t c = child;
      child = f.next(c);
      bad |= q.arrival_ns != at + q.hop_ns;  // §10.1: the whole hop cost is on the request path
      val = q.hop_ns + (q.finish_ns - q.arrival_ns);
      return c;
    }
    ISIM_TW void win(uint32_t c) { f.w[c].flags = kWinner; }
  };

  // Phase 2, writes w[j].won and the flags of j's children: the script of j replayed from its start S.
  // false: an arrival equation fails, a child matches no call command, or self would be below 0.
  ISIM_TW bool callers(uint32_t j) {
    const isim_des_span &q = s[j];
    uint64_t won = 0;
    bool bad = false;
    if (j + 1 < m && s[j + 1].caller_hop == j) {
      Kids kids{*this, j + 1, false};
      won = cp::replay_script(v, q.service < v.n_services ? q.service : 0u, q.start_ns, kids);
      bad = kids.bad || kids.more();
    }
    w[j].won = won;
    return !bad && won <= q.finish_ns - q.start_ns;
  }

  // Phase 3, read-only: j is critical iff every span from j up to the entry's child is a local winner
  ISIM_TW bool critical(uint32_t j) const {
    uint32_t a = j;
    while (a) {
      if (!(w[a].flags & kWinner)) return false;
      const uint32_t n = s[a].caller_hop;
      if (n >= a) return false;
      a = n;
    }
    return true;
  }

  // Phases 3 and 4 of span j, once the trace is known to be accepted: the status bit and the adds.  Returns
  // the wait of j if it is critical (the trace's critical wait is their sum), else 0.
  template <class Acc>
  ISIM_TW uint64_t finish(uint32_t j, Acc &acc) {
    isim_des_span &q = s[j];
    const uint32_t svc = q.service < v.n_services ? q.service : 0u;
    const uint64_t dur = q.finish_ns - q.arrival_ns, wait = q.start_ns - q.arrival_ns;
    if (j == 0) {
      acc.hdr(ISIM_DCP_H_TRACES, 1);
      acc.hdr(ISIM_DCP_H_SPANS, m);
      acc.hdr(ISIM_DCP_H_SUM_LATENCY, dur);
    }
    acc.add(svc, ISIM_DCP_INVOCATIONS, 1);
    acc.add(svc, ISIM_DCP_SUM_DURATION, dur);
    if (!critical(j)) return 0;
    const uint32_t status = q.status;
    q.status = status | ISIM_SPAN_CRITICAL;
    acc.hdr(ISIM_DCP_H_CRITICAL, 1);
    acc.add(svc, ISIM_DCP_CRITICAL, 1);
    acc.add(svc, ISIM_DCP_WAIT_NS, wait);
    acc.add(svc, ISIM_DCP_SELF_NS, q.finish_ns - q.start_ns - w[j].won);
    acc.add(svc, ISIM_DCP_HOP_NS, q.hop_ns);
    acc.add(svc, ISIM_DCP_CRITICAL_500, status & 1u);
    acc.add(svc, ISIM_DCP_CRITICAL_WAITED, wait ? 1u : 0u);
    return wait;
  }
};

// ---- the host's fold of a list of traces (isim_des_critical_path_host, and tests/cpp/des_critical_path_check.cpp
// under the sanitizers): the phases as plain loops, the links of one trace at a time.  ADDS into table;
// trace_wait nullptr or [n]
template <class KOf>
inline void fold_list(const cp::ScriptView &v, KOf kof, const uint64_t *off, uint64_t n, isim_des_span *spans,
                      uint64_t *table, uint64_t *trace_wait) {
  HostAcc acc{table, v.n_services};
  std::vector<Link> links;
  Fold<KOf> f;
  f.v = v;
  f.kof = kof;
  const uint64_t cap = off[n];  // the end of the written spans: no trace of the list reaches past it
  for (uint64_t i = 0; i < n; ++i) {
    bool ok = f.begin(off, i, cap, spans);
    if (ok) {
      links.assign(f.m, Link{});
      f.w = links.data();
      for (uint32_t j = 0; j < f.m; ++j) ok &= f.check(j);
    }
    if (ok) {
      for (uint32_t j = 0; j < f.m; ++j) f.link(j);
      for (uint32_t j = 0; j < f.m; ++j) ok &= f.callers(j);
    }
    uint64_t wait = UINT64_MAX;
    if (ok) {
      wait = 0;
      for (uint32_t j = 0; j < f.m; ++j) wait += f.finish(j, acc);
    } else {
      acc.hdr(ISIM_DCP_H_REFUSED, 1);
    }
    if (trace_wait) trace_wait[i] = wait;
  }
}

// ---- host side: every check of a handler that needs no GPU (handler.h has the handler; des_host.hip: what
// isim_serve_des_spans_device refuses with a tap); ISIM_OK or ISIM_EINVAL
int check_handler(const isim_handler *h);

// ---- device side (des_critical_path.hip): the launches of one checked call
int launch(const isim_handler *h, const uint64_t *d_off, isim_des_span *d_spans, uint64_t cap_spans,
           const uint64_t *d_info, uint64_t n_ids, uint64_t *d_table, uint64_t *d_trace_wait, void *d_workspace,
           void *stream);

}  // namespace dcp
}  // namespace isim
