// Critical path on the host (critical_path.h): the flat script
// table of a graph, the checks of a call, the fold of a list of traces as a
// plain loop over the steps the device runs, and the merge.  No HIP: these work
// without a GPU.
#include "critical_path.h"
#include "error.h"

#include <string>

namespace isim {
namespace cp {

namespace {
uint64_t sleep_of(const Command &c) { return c.kind == Command::Sleep && c.sleep_ns > 0 ? (uint64_t)c.sleep_ns : 0; }
}  // namespace

FlatScripts flat_scripts(const ServiceGraph &g) {
  FlatScripts f;
  f.cmd_off.reserve(g.services.size() + 1);
  for (const Service &svc : g.services) {
    f.cmd_off.push_back((uint32_t)f.cmds.size());
    for (const Command &c : svc.script) {
      if (c.kind == Command::Sleep) {
        f.cmds.push_back(sleep_of(c));
      } else if (c.kind == Command::Request) {
        f.cmds.push_back(kCmdCall);
      } else {
        f.cmds.push_back(kCmdConc | (uint32_t)c.commands.size());
        for (const Command &x : c.commands) f.cmds.push_back(x.kind == Command::Request ? kCmdCall : sleep_of(x));
      }
    }
  }
  f.cmd_off.push_back((uint32_t)f.cmds.size());
  return f;
}

int check_handler(const isim_handler *h) {
  if (!h) return set_error(ISIM_EINVAL, "critical path: null handler");
  if (const char *m = spans::handler_error(*spans::handler_view(h).prog); *m)
    return set_error(ISIM_EINVAL, std::string("critical path: ") + m);
  return ISIM_OK;
}

}  // namespace cp
}  // namespace isim

namespace {
namespace cp = isim::cp;
namespace sp = isim::spans;
int cfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "critical path: " + msg); }

template <class KOf>
bool fold_list(const cp::ScriptView &v, KOf kof, const uint64_t *off, uint64_t n, isim_span *spans, uint64_t *table) {
  cp::HostAcc acc{table, v.n_services};
  std::vector<uint32_t> links;
  cp::Fold<KOf> f;
  f.v = v;
  f.kof = kof;
  const uint64_t cap = off[n];  // the end of the written spans: no trace of the list reaches past it
  for (uint64_t i = 0; i < n; ++i) {
    if (!f.begin(off, i, cap, spans, acc)) continue;
    links.assign(2 * (size_t)f.m, 0);  // the links of one trace at a time
    f.link = links.data();
    while (f.step(acc)) {
    }
  }
  return !f.negative;
}
}  // namespace

extern "C" {

int isim_critical_path_table_words(const isim_handler *h, uint64_t *words) {
  if (!words) return cfail("null argument");
  if (const int rc = cp::check_handler(h)) return rc;
  *words = (uint64_t)(sp::handler_view(h).graph->services.size() + 1) * ISIM_CP_ROW_WORDS;
  return ISIM_OK;
}

int isim_critical_path_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes) {
  if (!bytes) return cfail("null argument");
  if (const int rc = cp::check_handler(h)) return rc;
  if (cap_spans > sp::kMaxRecords) return cfail("cap_spans is above 2^40");
  *bytes = cp::ws_bytes(cap_spans);
  return ISIM_OK;
}

int isim_critical_path_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src) {
  if (!dst || !src) return cfail("null argument");
  if (const int rc = cp::check_handler(h)) return rc;
  const uint64_t words = (uint64_t)(sp::handler_view(h).graph->services.size() + 1) * ISIM_CP_ROW_WORDS;
  for (uint64_t i = 0; i < words; ++i) dst[i] += src[i];
  return ISIM_OK;
}

int isim_critical_path_host(const isim_handler *h, const uint64_t *h_off, uint64_t n_written, isim_span *h_spans,
                            uint64_t *h_table) {
  if (const int rc = cp::check_handler(h)) return rc;
  if (!h_off || !h_table) return cfail("null offsets or table");
  if (n_written > sp::kMaxIds) return cfail("n_written is above 2^32");
  if (((uintptr_t)h_off | (uintptr_t)h_spans | (uintptr_t)h_table) & 7u)
    return cfail("the buffers must be 8-byte aligned");
  if (h_off[n_written] && !h_spans) return cfail("null spans");
  const sp::HandlerView v = sp::handler_view(h);
  const isim::Program &p = *v.prog;
  const cp::FlatScripts fs = cp::flat_scripts(*v.graph);
  const cp::ScriptView view{fs.cmd_off.data(), fs.cmds.data(), (uint32_t)v.graph->services.size(), p.tree_positions()};
  // the call index from the nodes the device reads: the 8-byte or the 16-byte format
  const bool ok = p.tree_wide ? fold_list(view, cp::K16{(const uint32_t *)p.tree_nodes_w.data()}, h_off, n_written,
                                          h_spans, h_table)
                              : fold_list(view, cp::K8{(const uint64_t *)p.tree_nodes.data()}, h_off, n_written,
                                          h_spans, h_table);
  if (!ok) return cfail("a self time below 0: the spans are not those of a walk of this handler");
  return ISIM_OK;
}

}  // extern "C"
