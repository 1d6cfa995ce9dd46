// Critical path of DES trace spans on the host (des_critical_path.h, DESIGN.md
// §22): the sizes, the merge and the fold of a list of traces (dcp::fold_list:
// plain loops over the phases the device runs).  No HIP: these work without a GPU.
#include "des_critical_path.h"
#include "error.h"

#include <string>
#include <vector>

namespace {
namespace cp = isim::cp;
namespace dcp = isim::dcp;
namespace sp = isim::spans;
int dfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "DES critical path: " + msg); }

uint64_t table_words(const isim_handler *h) {
  return (uint64_t)(sp::handler_view(h).graph->services.size() + 1) * ISIM_DCP_ROW_WORDS;
}

}  // namespace

extern "C" {

int isim_des_critical_path_table_words(const isim_handler *h, uint64_t *words) {
  if (!words) return dfail("null argument");
  if (const int rc = dcp::check_handler(h)) return rc;
  *words = table_words(h);
  return ISIM_OK;
}

int isim_des_critical_path_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes) {
  if (!bytes) return dfail("null argument");
  if (const int rc = dcp::check_handler(h)) return rc;
  if (cap_spans > sp::kMaxRecords) return dfail("cap_spans is above 2^40");
  *bytes = dcp::ws_bytes(cap_spans);
  return ISIM_OK;
}

int isim_des_critical_path_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src) {
  if (!dst || !src) return dfail("null argument");
  if (const int rc = dcp::check_handler(h)) return rc;
  const uint64_t words = table_words(h);
  for (uint64_t i = 0; i < words; ++i) dst[i] += src[i];
  return ISIM_OK;
}

int isim_des_critical_path_host(const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                isim_des_span *h_spans, uint64_t *h_table, uint64_t *h_trace_wait) {
  if (const int rc = dcp::check_handler(h)) return rc;
  if (!h_off || !h_table) return dfail("null offsets or table");
  if (n_written > sp::kMaxIds) return dfail("n_written is above 2^32");
  if ((((uintptr_t)h_off | (uintptr_t)h_table | (uintptr_t)h_trace_wait) & 7u) || ((uintptr_t)h_spans & 15u))
    return dfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (h_off[n_written] && !h_spans) return dfail("null spans");
  const sp::HandlerView v = sp::handler_view(h);
  const isim::Program &p = *v.prog;
  const cp::FlatScripts fs = cp::flat_scripts(*v.graph);
  const cp::ScriptView view{fs.cmd_off.data(), fs.cmds.data(), (uint32_t)v.graph->services.size(), p.tree_positions()};
  // the call index from the nodes the device reads: the 8-byte or the 16-byte format
  if (p.tree_wide)
    dcp::fold_list(view, cp::K16{(const uint32_t *)p.tree_nodes_w.data()}, h_off, n_written, h_spans, h_table, h_trace_wait);
  else
    dcp::fold_list(view, cp::K8{(const uint64_t *)p.tree_nodes.data()}, h_off, n_written, h_spans, h_table, h_trace_wait);
  return ISIM_OK;
}

}  // extern "C"
