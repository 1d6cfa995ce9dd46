// Trace spans (include/isim.h isim_trace_spans*, isim_select_traces*, DESIGN.md
// §19), one header for spans.cpp (host) and spans.hip (host and device): the
// sink that turns the lane tree walk's closes (tree_walk.h close_rec) into
// isim_span records, the walk variant of a tree, the workspace layouts and the
// selection predicate.  A trace is a pure function of (seed, trace id): its
// spans come from walking it again, with the error draws the statuses need.
#pragma once

#include <cstdint>
#include <memory>
#include <mutex>

#include "../../include/isim.h"
#include "graph.h"
#include "kernel_abi.h"
#include "program.h"
#include "tree_walk.h"

namespace isim {
namespace spans {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kMaxIds = 1ull << 32;
constexpr uint64_t kMaxRecords = 1ull << 40;

// ---- what the span code reads of a handler (handler.h has the struct): its program, graph and
// parameters, and a slot for the per-device tables of spans.hip (freed with the handler)
struct HandlerView {
  const Program *prog;
  const ServiceGraph *graph;
  const isim_params *params;
  std::mutex *mu;                  // guards *state
  std::shared_ptr<void> *state;
};
HandlerView handler_view(const isim_handler *h);  // api.hip

// ---- the walk variant of a tree: the pre-walk's set (des_items.hip prewalk_kernel)
enum Frames : uint32_t { kFramesSpill = 0, kFrames16 = 1, kFrames8 = 2 };  // 8 + spill, 16, 8 register frames
constexpr uint32_t kSpillRegFrames = 8;
inline Frames frames_of(uint32_t tree_frames) {
  return tree_frames > kTreeRegFrames ? kFramesSpill : tree_frames > 8 ? kFrames16 : kFrames8;
}
// spilled levels of one lane and the u32 words of one level
inline uint32_t spill_levels(uint32_t tree_frames) {
  return tree_frames > kTreeRegFrames ? tree_frames - kSpillRegFrames + 1 : 0;
}
inline uint32_t spill_level_words(bool t64, bool wide) {
  return (t64 ? kTreeSpillWords64 : kTreeSpillWords) + (wide ? kTreeSpillWide : 0u);
}

// ---- the device call's geometry (spans.hip; host side, shared with the workspace size)
constexpr uint32_t kT = 256;            // threads of every kernel here
constexpr uint32_t kWalkBlocks = 2048;  // walk grid cap (waves refill from a counter of 64-entry batches)
constexpr uint32_t kTile = 1024;        // entries of one scan tile (kT x 4)
inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
inline uint32_t walk_blocks(uint64_t n_ids) {
  const uint64_t waves = (n_ids + 63) / 64, b = (waves + kT / 64 - 1) / (kT / 64);
  return (uint32_t)(b < 1 ? 1 : b > kWalkBlocks ? kWalkBlocks : b);
}
inline uint64_t tiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }

// workspace of isim_trace_spans_device: two batch counters, the hop counts, the tile sums, the spill columns
struct SpanWs {
  uint64_t off_work, off_cnt, off_tile, off_spill, bytes;
};
inline SpanWs span_ws(const Program &p, uint64_t n_ids) {
  SpanWs w{};
  w.off_work = 0;
  w.off_cnt = 64;
  w.off_tile = w.off_cnt + round_up(n_ids * 4, 64);
  w.off_spill = w.off_tile + round_up((tiles_of(n_ids) + 1) * 8, 64);
  w.bytes = w.off_spill + (uint64_t)spill_levels(p.tree_frames) * spill_level_words(p.tree_t64, p.tree_wide) *
                              walk_blocks(n_ids) * kT * 4;
  return w;
}
// workspace of isim_select_traces_device: the tile sums
inline uint64_t select_ws_bytes(uint64_t n) { return round_up((tiles_of(n) + 1) * 8, 64); }

// ---- the selection predicate
ISIM_TW bool selected(uint64_t latency, uint32_t status_err, uint64_t min_latency, uint32_t cls) {
  const uint32_t code = status_err >> 31;
  return latency >= min_latency && (cls == ISIM_Q_ALL || (cls == ISIM_Q_500) == (code != 0u));
}

// ---- an invocation's own error draw, as the walk draws it (tree_walk.h Lane::own_error)
ISIM_TW bool own_of(uint32_t t_lo, uint32_t t_hi, uint32_t hop, uint32_t flags, uint32_t thr, uint32_t k0,
                    uint32_t k1) {
  if (flags & TF_ERR_ALWAYS) return true;
  if (!(flags & TF_ERR_DRAW)) return false;
  uint32_t a = t_lo, b = t_hi, c = hop >> 2, d = 0;
  tw::philox10(a, b, c, d, k0, k1);
  return tw::word4(hop & 3u, a, b, c, d) < thr;
}

// status word of a span: bit 0 the response, bit 1 the own draw.  Mode A: a 500 is the own draw.  Mode B:
// a 500 of a calling invocation is its own draw or a failed step; the draw is taken again (500s are rare)
template <bool MB>
ISIM_TW uint32_t span_status(bool st, bool leaf, uint32_t t_lo, uint32_t t_hi, uint32_t hop, uint32_t flags,
                             uint32_t thr, uint32_t k0, uint32_t k1) {
  if (!st) return 0u;
  if (!MB || leaf) return 3u;
  return own_of(t_lo, t_hi, hop, flags, thr, k0, k1) ? 3u : 1u;
}

struct NoStats {
  ISIM_TW void call(uint32_t) {}
  ISIM_TW void resp_leaf(uint32_t, bool) {}
  template <typename TT>
  ISIM_TW void resp(uint32_t, uint32_t, TT, bool) {}
};

// One span per executed invocation at out[hop], written once, whole, when the invocation closes; the
// entry's (the walk reports it with duration 0) is written by entry_span once the trace has responded.
// out == nullptr: the trace does not fit the caller's buffer and writes nothing.
template <bool MB, class Nodes>
struct SpanSink : NoStats {
  static constexpr bool kCloseRec = true;
  isim_span *out = nullptr;
  Nodes nodes;
  const TreeExt *ext = nullptr;
  const uint32_t *slot_callee = nullptr;
  uint32_t entry = 0;
  uint32_t t_lo = 0, t_hi = 0, k0 = 0, k1 = 0;
  template <typename TT>
  ISIM_TW void rec_close(uint32_t p, uint32_t hop, uint32_t caller, TT T, bool st) {
    if (caller == tw::kNoCaller || !out) return;
    const auto n = nodes.load(p);
    const TreeExt x = tw::load_ext(ext, p);
    isim_span s;
    s.start_ns = 0;
    s.duration_ns = (uint64_t)T;
    s.hop_ns = x.H;
    s.hop = hop;
    s.caller_hop = caller;
    s.position = p;
    s.slot = n.slot();
    s.service = slot_callee[n.slot()];
    s.status = span_status<MB>(st, (n.flags() & TF_LEAF) != 0, t_lo, t_hi, hop, n.flags(), x.thr, k0, k1);
    out[hop] = s;
  }
  ISIM_TW void entry_span(uint64_t lat, bool root500) {
    if (!out) return;
    const auto n = nodes.load(0);
    isim_span s;
    s.start_ns = 0;
    s.duration_ns = lat;
    s.hop_ns = 0;
    s.hop = 0;
    s.caller_hop = kNone;
    s.position = 0;
    s.slot = kNone;
    s.service = entry;
    s.status = span_status<MB>(root500, (n.flags() & TF_LEAF) != 0, t_lo, t_hi, 0u, n.flags(),
                               tw::load_ext(ext, 0).thr, k0, k1);
    out[0] = s;
  }
  ISIM_TW void begin(uint64_t trace, isim_span *o) {
    t_lo = (uint32_t)trace;
    t_hi = (uint32_t)(trace >> 32);
    out = o;
  }
};

// ---- host side (spans.cpp).  "" or why the handler has no spans
const char *handler_error(const Program &p);

// ---- device side (spans.hip).  The handler's tables on a device: the tree's nodes, per-position facts, the
// slot-to-callee table, the flat scripts (critical_path.h) and the services' worker holds (des.h); uploaded once per (handler, device) at the first
// call that needs them, under a relaxed capture mode, so that call may itself be a captured one
struct DevTables {
  void *nodes = nullptr;
  TreeExt *ext = nullptr;
  TreeStep *step = nullptr;
  uint32_t *slot_callee = nullptr;
  uint32_t *cmd_off = nullptr;
  uint64_t *cmds = nullptr;
  uint64_t *svc_hold = nullptr;  // [n_services]: des_service_holds
};
int device_tables(const HandlerView &v, DevTables &out);  // of the current device; ISIM_OK or ISIM_EHIP

// the launches of one checked call; ISIM_OK or ISIM_EHIP (message set)
int spans_launch(const isim_handler *h, const uint64_t *d_ids, uint64_t n_ids, uint64_t *d_off, isim_span *d_spans,
                 uint64_t cap_spans, uint64_t *d_info, void *d_workspace, void *stream);
// the scan step of spans_launch alone (the DES tap, des_items.hip, shares it): d_cnt[n] -> d_off[n + 1], its
// exclusive scan, and d_info's four words under cap_spans; d_tile: tiles_of(n) + 1 words; n 0 writes d_off[0] = 0
int scan_launch(const uint32_t *d_cnt, uint64_t n, uint64_t *d_tile, uint64_t *d_off, uint64_t cap_spans,
                uint64_t *d_info, void *stream);
int select_launch(const isim_trace_rec *d_records, uint64_t n, uint64_t trace_begin, uint64_t min_latency,
                  uint32_t cls, uint64_t max_ids, uint64_t *d_ids, uint64_t *d_info, void *d_workspace, void *stream);

}  // namespace spans
}  // namespace isim
