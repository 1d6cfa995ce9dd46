// Trace spans on the host (spans.h): the checks of a call, the
// walk of a list of trace ids through tw::Lane compiled for the CPU (the code
// the device runs, as tests/cpp/tree_walk_check.cpp runs it), the start times
// and the selection as a plain loop.  No HIP: these work without a GPU.
#include "spans.h"
#include "error.h"

#include <string>
#include <vector>

namespace isim {
namespace spans {

const char *handler_error(const Program &p) {
  if (p.static_walk || !p.has_tree())
    return p.static_walk ? "the handler runs a static walk, which has no unrolled tree: create it with ISIM_FLAG_DYNAMIC"
                         : "the handler has no unrolled tree of potential invocations";
  if (p.tree_dag) return "the handler walks the site graph (tree_dag), which has no positions to name spans by";
  return "";
}

}  // namespace spans
}  // namespace isim

namespace {
namespace sp = isim::spans;
namespace tw = isim::tw;
using isim::Command;
using isim::Program;
using isim::Service;

int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "trace spans: " + msg); }

// one trace on one lane: its hops, and with a sink that has a buffer its spans
template <class LaneT, class Nodes, class Sink>
uint32_t walk_one(LaneT &L, const Nodes &nodes, const Program &p, Sink &s, uint64_t trace) {
  L.start(trace);
  while (!L.done) L.step(nodes, p.tree_ext.data(), p.tree_step.data(), s, s.k0, s.k1);
  s.entry_span((uint64_t)L.lat, L.root500);
  return L.hops();
}

// The list's walks in the variant the device takes for this tree (spans.h frames_of).  Pass 1 counts
// (no buffer), pass 2 emits the traces that fit.
template <int FR, bool SPILL, bool MB, typename TT, bool W>
void walk_list(const Program &p, const isim_params &prm, const uint64_t *ids, uint64_t n, uint64_t *off,
               isim_span *spans, uint64_t cap, uint64_t *info) {
  tw::Lane<FR, MB, true, SPILL, true, TT, W> L;
  std::vector<uint32_t> spill((size_t)sp::spill_levels(p.tree_frames) * sp::spill_level_words(p.tree_t64, W) + 1);
  L.sp = spill.data();
  L.sp_stride = 1;
  using Nodes = std::conditional_t<W, tw::CpuNodesW, tw::CpuNodes>;
  Nodes nodes;
  if constexpr (W) nodes = Nodes{p.tree_nodes_w.data()};
  else nodes = Nodes{p.tree_nodes.data()};
  std::vector<uint32_t> callee(p.slot_callee.begin(), p.slot_callee.end());
  sp::SpanSink<MB, Nodes> s;
  s.nodes = nodes;
  s.ext = p.tree_ext.data();
  s.slot_callee = callee.data();
  s.entry = (uint32_t)p.entry;
  s.k0 = (uint32_t)prm.seed;
  s.k1 = (uint32_t)(prm.seed >> 32);
  uint64_t total = 0;
  off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    s.begin(ids[i], nullptr);
    total += walk_one(L, nodes, p, s, ids[i]);
    off[i + 1] = total;
  }
  uint64_t written = 0;
  while (written < n && off[written + 1] <= cap) ++written;
  for (uint64_t i = 0; i < written; ++i) {
    s.begin(ids[i], spans + off[i]);
    walk_one(L, nodes, p, s, ids[i]);
  }
  info[ISIM_SPAN_TOTAL] = total;
  info[ISIM_SPAN_WRITTEN] = written;
  info[ISIM_SPAN_N_IDS] = n;
  info[ISIM_SPAN_FIRST_UNFIT] = written;
}

template <int FR, bool SPILL, typename... A>
void walk_pick(const Program &p, const isim_params &prm, A... a) {
  const bool mb = prm.error_mode == ISIM_MODE_B;
  if (p.tree_wide) {
    if (p.tree_t64) mb ? walk_list<FR, SPILL, true, uint64_t, true>(p, prm, a...)
                       : walk_list<FR, SPILL, false, uint64_t, true>(p, prm, a...);
    else mb ? walk_list<FR, SPILL, true, uint32_t, true>(p, prm, a...)
            : walk_list<FR, SPILL, false, uint32_t, true>(p, prm, a...);
  } else {
    if (p.tree_t64) mb ? walk_list<FR, SPILL, true, uint64_t, false>(p, prm, a...)
                       : walk_list<FR, SPILL, false, uint64_t, false>(p, prm, a...);
    else mb ? walk_list<FR, SPILL, true, uint32_t, false>(p, prm, a...)
            : walk_list<FR, SPILL, false, uint32_t, false>(p, prm, a...);
  }
}

uint64_t sleep_of(const Command &c) { return c.kind == Command::Sleep && c.sleep_ns > 0 ? (uint64_t)c.sleep_ns : 0; }

// The start times of one trace's spans s[0 .. m) (hop order).  Callers come before their callees, so a
// caller's start is known when its script is replayed; a caller's executed calls are its children in hop
// order, each at the call index its position's node carries.
void place_trace(const Program &p, const isim::ServiceGraph &g, isim_span *s, uint64_t m, std::vector<uint32_t> &head,
                 std::vector<uint32_t> &next) {
  head.assign(m, sp::kNone);
  next.assign(m, sp::kNone);
  for (uint64_t i = m; i-- > 1;) {  // children lists in hop order
    const uint32_t c = s[i].caller_hop;
    next[i] = head[c];
    head[c] = (uint32_t)i;
  }
  s[0].start_ns = 0;
  for (uint64_t i = 0; i < m; ++i) {
    uint32_t child = head[i];
    if (child == sp::kNone) continue;
    uint64_t clock = s[i].start_ns;
    uint32_t k = 0;
    // the call command k: its executed child, if the next child sits at call index k
    auto take = [&](uint64_t at) -> uint64_t {
      const uint32_t kk = k++;
      if (child == sp::kNone || (p.tree_nodes_w[s[child].position].k & 0xFFFFu) != kk) return 0;
      isim_span &c = s[child];
      child = next[child];
      c.start_ns = at;
      return c.hop_ns + c.duration_ns;
    };
    for (const Command &c : g.services[s[i].service].script) {
      if (child == sp::kNone) break;  // (mode B: after a failed step no step runs, and no child remains)
      if (c.kind == Command::Sleep) {
        clock += sleep_of(c);
      } else if (c.kind == Command::Request) {
        clock += take(clock);
      } else {
        uint64_t longest = 0;
        for (const Command &x : c.commands) {
          const uint64_t d = x.kind == Command::Request ? take(clock) : sleep_of(x);
          longest = d > longest ? d : longest;
        }
        clock += longest;
      }
    }
  }
}

int check_list(const isim_handler *h, uint64_t n_ids, const void *ids, const void *off, const void *spans,
               uint64_t cap, const void *info) {
  if (!h) return sfail("null handler");
  if (const char *m = sp::handler_error(*sp::handler_view(h).prog); *m) return sfail(m);
  if (n_ids > sp::kMaxIds) return sfail("n_ids is above 2^32");
  if (!off || !info) return sfail("null offsets or info");
  if (n_ids && !ids) return sfail("null trace ids");
  if (cap && !spans) return sfail("null spans with cap_spans > 0");
  if (((uintptr_t)ids | (uintptr_t)off | (uintptr_t)spans | (uintptr_t)info) & 7u)
    return sfail("the buffers must be 8-byte aligned");
  return ISIM_OK;
}

}  // namespace

extern "C" {

int isim_trace_spans_workspace_bytes(const isim_handler *h, uint64_t n_ids, uint64_t *bytes) {
  if (!h || !bytes) return sfail("null argument");
  const Program &p = *sp::handler_view(h).prog;
  if (const char *m = sp::handler_error(p); *m) return sfail(m);
  if (n_ids > sp::kMaxIds) return sfail("n_ids is above 2^32");
  *bytes = sp::span_ws(p, n_ids).bytes;
  return ISIM_OK;
}

int isim_trace_spans_place(const isim_handler *h, const uint64_t *h_off, uint64_t n_written, isim_span *h_spans) {
  if (!h || !h_off) return sfail("null argument");
  const sp::HandlerView v = sp::handler_view(h);
  if (const char *m = sp::handler_error(*v.prog); *m) return sfail(m);
  if (n_written > sp::kMaxIds) return sfail("n_ids is above 2^32");
  if (n_written && !h_spans) return sfail("null spans");
  const uint32_t P = v.prog->tree_positions(), S = (uint32_t)v.graph->services.size();
  std::vector<uint32_t> head, next;
  for (uint64_t i = 0; i < n_written; ++i) {
    if (h_off[i + 1] <= h_off[i] || h_off[i + 1] - h_off[i] > 0xFFFFFFFFull) return sfail("offsets do not ascend");
    isim_span *s = h_spans + h_off[i];
    const uint64_t m = h_off[i + 1] - h_off[i];
    for (uint64_t j = 0; j < m; ++j)  // the spans of a walk; anything else is refused, not followed
      if (s[j].hop != j || s[j].position >= P || s[j].service >= S ||
          (j ? s[j].caller_hop >= j : s[j].caller_hop != sp::kNone))
        return sfail("the spans are not those of a walk of this handler");
    place_trace(*v.prog, *v.graph, s, m, head, next);
  }
  return ISIM_OK;
}

int isim_trace_spans_host(const isim_handler *h, const uint64_t *h_ids, uint64_t n_ids, uint64_t *h_off,
                          isim_span *h_spans, uint64_t cap_spans, uint64_t *h_info) {
  if (const int rc = check_list(h, n_ids, h_ids, h_off, h_spans, cap_spans, h_info)) return rc;
  const sp::HandlerView v = sp::handler_view(h);
  const Program &p = *v.prog;
  switch (sp::frames_of(p.tree_frames)) {
    case sp::kFramesSpill:
      walk_pick<8, true>(p, *v.params, h_ids, n_ids, h_off, h_spans, cap_spans, h_info);
      break;
    case sp::kFrames16:
      walk_pick<16, false>(p, *v.params, h_ids, n_ids, h_off, h_spans, cap_spans, h_info);
      break;
    default:
      walk_pick<8, false>(p, *v.params, h_ids, n_ids, h_off, h_spans, cap_spans, h_info);
  }
  return isim_trace_spans_place(h, h_off, h_info[ISIM_SPAN_WRITTEN], h_spans);
}

int isim_select_traces_workspace_bytes(uint64_t n, uint64_t *bytes) {
  if (!bytes) return sfail("null argument");
  if (n > sp::kMaxRecords) return sfail("n is above 2^40");
  *bytes = sp::select_ws_bytes(n);
  return ISIM_OK;
}

int isim_select_traces_host(const isim_trace_rec *h_records, uint64_t n, uint64_t trace_begin,
                            uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *h_ids,
                            uint64_t *h_info) {
  if (!h_info || (n && !h_records) || (max_ids && !h_ids)) return sfail("select: null argument");
  if (cls > ISIM_Q_500) return sfail("select: the class must be ISIM_Q_ALL, ISIM_Q_200 or ISIM_Q_500");
  if (n > sp::kMaxRecords) return sfail("select: n is above 2^40");
  uint64_t matches = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (!sp::selected(h_records[i].latency_ns, h_records[i].status_err, min_latency_ns, cls)) continue;
    if (matches < max_ids) h_ids[matches] = trace_begin + i;
    ++matches;
  }
  h_info[0] = matches;
  h_info[1] = matches < max_ids ? matches : max_ids;
  return ISIM_OK;
}

}  // extern "C"
