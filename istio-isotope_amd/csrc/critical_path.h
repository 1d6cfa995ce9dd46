// Critical path of chosen traces (include/isim.h isim_critical_path*, DESIGN.md
// §20), one header for critical_path.cpp (host) and critical_path.hip (host and
// device): the flat script table, the replay of one caller's script (start
// times and local winners, spans.cpp place_trace's clock), and the fold of one
// trace in steps of one span: check, children links (two passes), one forward
// pass in hop order.  The host runs the steps of a trace in a loop; the device runs one
// trace per lane, a step per turn, and refills the lanes that have finished.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/isim.h"
#include "spans.h"

namespace isim {
namespace cp {

constexpr uint32_t kNone = spans::kNone;
constexpr uint32_t kSleepWon = 0xFFFFFFFEu;  // the winner of a concurrent step is one of its sleeps
constexpr uint64_t kMaxTraceSpans = 0xFFFFFFFFull;

// ---- the flat script table: cmd_off[n_services + 1] into one packed u64 per command
//   bit 63 clear          a sleep of max(d, 0) ns (a member of a concurrent step that is neither a call
//                         nor a sleep counts as a sleep of 0, as place_trace counts it)
//   bits 63..62 = 10      a call command
//   bits 63..62 = 11      a concurrent step begins: the low 32 bits count its members, which follow
constexpr uint64_t kCmdCall = 2ull << 62;
constexpr uint64_t kCmdConc = 3ull << 62;
ISIM_TW bool cmd_is_sleep(uint64_t c) { return (c >> 63) == 0; }
ISIM_TW bool cmd_is_conc(uint64_t c) { return (c >> 62) == 3; }

struct FlatScripts {
  std::vector<uint32_t> cmd_off;
  std::vector<uint64_t> cmds;
};
FlatScripts flat_scripts(const ServiceGraph &g);  // critical_path.cpp

struct ScriptView {
  const uint32_t *cmd_off;
  const uint64_t *cmds;
  uint32_t n_services, n_positions;
};

// ---- the call index of a position, from the tree's nodes in either format (kernel_abi.h)
struct K8 {
  const uint64_t *p;  // TreeNode: size | k << 16 | ...
  ISIM_TW uint32_t operator()(uint32_t pos) const { return ((uint32_t)p[pos] >> 16) & 0xFFFFu; }
};
struct K16 {
  const uint32_t *p;  // TreeNodeW: size, k, ...
  ISIM_TW uint32_t operator()(uint32_t pos) const { return p[4 * (uint64_t)pos + 1] & 0xFFFFu; }
};

// workspace of isim_critical_path_device: the batch counter, then {head, next} per span of the buffer
constexpr uint64_t kWsHead = 64;
inline uint64_t ws_bytes(uint64_t cap_spans) { return kWsHead + cap_spans * 8; }

// ---- the table on the host: plain adds
struct HostAcc {
  uint64_t *table;
  uint32_t n_services;
  void add(uint32_t row, uint32_t word, uint64_t v) { table[(uint64_t)row * ISIM_CP_ROW_WORDS + word] += v; }
  void hdr(uint32_t word, uint64_t v) { add(n_services, word, v); }
};

// The script of one caller from `clock` on, over its executed children in hop order, each matched to the call
// command whose index its position carries.  The span type supplies the children (Fold::Kids here, the DES
// spans' in des_critical_path.h):
//   more()             an executed child is left
//   take(k, at, val)   call command k, sent at clock `at`: the next child if it sits at call index k (taken: its
//                      start written or its arrival checked, `val` its H + T), else kNone with val 0
//   win(c)             child c is a local winner
// Returns the sum of H + T over the local winners.
template <class Kids>
ISIM_TW uint64_t replay_script(const ScriptView &v, uint32_t svc, uint64_t clock, Kids &kids) {
  uint32_t k = 0;
  uint64_t won = 0;
  const uint32_t end = v.cmd_off[svc + 1];
  for (uint32_t x = v.cmd_off[svc]; x < end && kids.more();) {  // (mode B: nothing follows a failed step)
    const uint64_t c = v.cmds[x++];
    if (cmd_is_sleep(c)) {
      clock += c;
    } else if (!cmd_is_conc(c)) {
      uint64_t val;
      const uint32_t w = kids.take(k++, clock, val);
      if (w != kNone) {
        kids.win(w);
        won += val;
      }
      clock += val;
    } else {
      uint32_t n = (uint32_t)c, winner = kNone;
      n = n < end - x ? n : end - x;
      uint64_t longest = 0;
      for (; n; --n) {
        const uint64_t mc = v.cmds[x++];
        uint64_t val = mc;
        uint32_t w = kSleepWon;
        if (!cmd_is_sleep(mc)) w = kids.take(k++, clock, val);
        if (val > longest) {  // strictly: ties go to the first listed member, a zero never wins
          longest = val;
          winner = w;
        }
      }
      if (winner < kSleepWon) {
        kids.win(winner);
        won += longest;
      }
      clock += longest;
    }
  }
  return won;
}

// One trace.  begin() checks the offsets; step() handles one span of the current phase and returns
// false once the trace is finished (folded or refused).  Every index read from a span or a link is
// bounded before it is used, in every phase: memory safety does not depend on the spans being a walk's.
template <class KOf>
struct Fold {
  ScriptView v;
  KOf kof;
  isim_span *s = nullptr;
  uint32_t *link = nullptr;  // {head, next} of span j at link[2 j], link[2 j + 1]: set by the caller after begin()
  uint64_t base = 0;         // the trace's first span in the buffer
  uint32_t m = 0, j = 0, phase = 0;
  bool negative = false;     // some self time would be below 0 (never for the spans of a walk)

  ISIM_TW uint32_t head(uint32_t i) const {
    const uint32_t c = link[2 * (uint64_t)i];
    return c > i && c < m ? c : kNone;
  }
  // children ascend in hop, so a chain of links ends after at most m of them whatever the links hold
  ISIM_TW uint32_t next(uint32_t c) const {
    const uint32_t n = link[2 * (uint64_t)c + 1];
    return n > c && n < m ? n : kNone;
  }

  // spans [off[i], off[i + 1]) of a buffer of `cap` spans
  template <class Acc>
  ISIM_TW bool begin(const uint64_t *off, uint64_t i, uint64_t cap, isim_span *spans, Acc &acc) {
    const uint64_t a = off[i], b = off[i + 1];
    if (b <= a || b > cap || b - a > kMaxTraceSpans) {
      acc.hdr(ISIM_CP_H_REFUSED, 1);
      return false;
    }
    s = spans + a;
    base = a;
    m = (uint32_t)(b - a);
    j = 0;
    phase = 0;
    return true;
  }

  // The children of one caller as replay_script takes them: a matched child gets its start time, a
  // local winner of a critical caller the bit
  struct Kids {
    Fold &f;
    uint32_t child;
    bool critical;
    ISIM_TW bool more() const { return child != kNone; }
    ISIM_TW uint32_t take(uint32_t k, uint64_t at, uint64_t &val) {
      val = 0;
      if (child == kNone) return kNone;
      const uint32_t pos = f.s[child].position;
      if (pos >= f.v.n_positions || f.kof(pos) != k) return kNone;
      const uint32_t c = child;
      child = f.next(c);
      f.s[c].start_ns = at;
      val = f.s[c].hop_ns + f.s[c].duration_ns;
      return c;
    }
    ISIM_TW void win(uint32_t c) {
      if (critical) f.s[c].status |= ISIM_SPAN_CRITICAL;
    }
  };
  // The script of caller i from `clock` on: its executed children get their start times; with `critical` the
  // local winners get the bit.  Returns the sum of H + T over the local winners.
  ISIM_TW uint64_t replay(uint32_t i, uint32_t svc, uint64_t clock, bool critical) {
    Kids kids{*this, head(i), critical};
    return replay_script(v, svc, clock, kids);
  }

  template <class Acc>
  ISIM_TW bool step(Acc &acc) {
    if (phase == 0) {  // the spans of a walk, as isim_trace_spans_place checks them; anything else is refused
      const isim_span &q = s[j];
      if (q.hop != j || q.position >= v.n_positions || q.service >= v.n_services ||
          (j ? q.caller_hop >= j : q.caller_hop != kNone)) {
        acc.hdr(ISIM_CP_H_REFUSED, 1);
        return false;  // nothing written so far, the workspace included
      }
      if (++j == m) {
        j = 0;
        phase = 1;
      }
      return true;
    }
    if (phase == 1) {  // no children yet (the workspace may hold anything)
      link[2 * (uint64_t)j] = kNone;
      if (++j == m) {
        j = m - 1;
        phase = j ? 2 : 3;
      }
      return true;
    }
    if (phase == 2) {  // children lists in hop order: from the last span down
      const uint32_t c = s[j].caller_hop;
      if (c < j) {
        link[2 * (uint64_t)j + 1] = link[2 * (uint64_t)c];
        link[2 * (uint64_t)c] = j;
      }
      if (--j == 0) phase = 3;
      return true;
    }
    // the forward pass: a caller's hop is below its callees', so its start time and its bit are final here
    isim_span &q = s[j];
    if (j == 0) {
      q.start_ns = 0;
      q.status |= ISIM_SPAN_CRITICAL;
      acc.hdr(ISIM_CP_H_TRACES, 1);
      acc.hdr(ISIM_CP_H_SPANS, m);
      acc.hdr(ISIM_CP_H_SUM_LATENCY, q.duration_ns);
    }
    const uint32_t svc = q.service < v.n_services ? q.service : 0u, status = q.status;
    const uint64_t dur = q.duration_ns;
    const bool critical = (status & ISIM_SPAN_CRITICAL) != 0;
    const uint64_t won = head(j) != kNone ? replay(j, svc, q.start_ns, critical) : 0;
    negative |= won > dur;
    acc.add(svc, ISIM_CP_INVOCATIONS, 1);
    acc.add(svc, ISIM_CP_SUM_DURATION, dur);
    if (critical) {
      acc.hdr(ISIM_CP_H_CRITICAL, 1);
      acc.add(svc, ISIM_CP_CRITICAL, 1);
      acc.add(svc, ISIM_CP_SELF_NS, dur - won);
      acc.add(svc, ISIM_CP_HOP_NS, q.hop_ns);
      acc.add(svc, ISIM_CP_CRITICAL_500, status & 1u);
    }
    return ++j < m;
  }
};

// ---- host side (critical_path.cpp): the checks of a call that need no GPU; ISIM_OK or ISIM_EINVAL
int check_handler(const isim_handler *h);

// ---- device side (critical_path.hip): the launches of one checked call
int launch(const isim_handler *h, const uint64_t *d_off, isim_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
           uint64_t n_ids, uint64_t *d_table, void *d_workspace, void *stream);

}  // namespace cp
}  // namespace isim
