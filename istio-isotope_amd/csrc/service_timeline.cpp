// Service timeline on the host (service_timeline.h): the
// services' holds, the sizes, the merge, the parameter checks and the fold of a
// list of spans (svt::fold_host).  No HIP: these work without a GPU.
#include "service_timeline.h"

#include <algorithm>
#include <string>
#include <vector>

#include "des.h"
#include "error.h"
#include "spans.h"

namespace {
namespace svt = isim::svt;
namespace sp = isim::spans;
int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service timeline: " + msg); }

}  // namespace

// the handler, the parameters and the table's size; the cells on success
int isim::svt::check(const isim_handler *h, const isim_timeline_params *p, uint64_t &cells) {
  if (const int rc = check_handler(h)) return rc;
  if (const char *m = tl::params_error(p)) return sfail(m);
  cells = cells_of(sp::handler_view(h).graph->services.size(), p->n_windows);
  if (cells > ISIM_SVT_MAX_CELLS) return sfail("n_services x (n_windows + 2) is above 2^24");
  return ISIM_OK;
}

extern "C" {

int isim_des_service_holds(const isim_handler *h, uint64_t *hold_ns, uint32_t *replicas) {
  if (const int rc = svt::check_handler(h)) return rc;
  if (!hold_ns || !replicas) return sfail("null argument");
  const isim::ServiceGraph &g = *sp::handler_view(h).graph;
  const std::vector<uint64_t> hold = isim::des_service_holds(g);
  for (size_t s = 0; s < g.services.size(); ++s) {
    hold_ns[s] = hold[s];
    replicas[s] = (uint32_t)std::max<int32_t>(1, g.services[s].num_replicas);
  }
  return ISIM_OK;
}

int isim_service_timeline_table_words(const isim_handler *h, const isim_timeline_params *p, uint64_t *words) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (!words) return sfail("null argument");
  *words = svt::table_words(cells);
  return ISIM_OK;
}

int isim_service_timeline_workspace_bytes(const isim_handler *h, const isim_timeline_params *p, uint64_t *bytes) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (!bytes) return sfail("null argument");
  *bytes = svt::ws_bytes(cells);
  return ISIM_OK;
}

int isim_service_timeline_merge(const isim_handler *h, const isim_timeline_params *p, uint64_t *dst,
                                const uint64_t *src) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (!dst || !src) return sfail("null argument");
  for (uint64_t c = 0; c < cells; ++c)
    for (uint32_t w = 0; w < svt::kW; ++w) {
      const uint64_t i = c * svt::kW + w;
      if (w == ISIM_SVT_MAX_WAIT) dst[i] = std::max(dst[i], src[i]);
      else dst[i] += src[i];
    }
  for (uint32_t w = 0; w < svt::kW; ++w) dst[cells * svt::kW + w] += src[cells * svt::kW + w];
  return ISIM_OK;
}

int isim_service_timeline_host(const isim_handler *h, const isim_timeline_params *p, const isim_des_span *h_spans,
                               uint64_t n_spans, uint64_t *h_table) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (n_spans > svt::kMaxSpans) return sfail("n_spans is above 2^40");
  if (!h_table) return sfail("null table");
  if (n_spans && !h_spans) return sfail("null spans");
  if (((uintptr_t)h_table & 7u) || ((uintptr_t)h_spans & 7u)) return sfail("the buffers must be 8-byte aligned");
  const isim::ServiceGraph &g = *sp::handler_view(h).graph;
  const std::vector<uint64_t> hold = isim::des_service_holds(g);
  svt::RowArgs a{};
  isim::tl::set_row_args(a, *p);
  std::vector<uint64_t> cover(2 * cells);
  svt::fold_host(a, (uint32_t)g.services.size(), hold.data(), h_spans, n_spans, h_table, cover.data());
  return ISIM_OK;
}

}  // extern "C"
