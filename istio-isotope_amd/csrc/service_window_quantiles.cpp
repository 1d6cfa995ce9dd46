// Per-service percentiles over time on the host (service_window_quantiles.h,
// DESIGN.md §29): the checks every entry point shares, the sizes and the table
// of a list of spans (swq::fold_host).  No HIP: these work without a GPU.
#include "service_window_quantiles.h"

#include <string>

#include "error.h"

namespace {
namespace swq = isim::swq;
int wfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service window quantiles: " + msg); }

}  // namespace

int isim::swq::check(const isim_handler *h, const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q,
                     bool with_list, uint64_t n_spans, uint64_t &n_services, uint64_t &cells) {
  if (const int rc = with_list ? svq::check(h, q_ppm, n_q, n_spans, n_services)
                               : svq::check_sizes(h, n_q, n_spans, n_services))
    return rc;
  if (const char *m = tl::params_error(p)) return wfail(m);
  cells = cells_of(n_services, p->n_windows);
  if (cells > kMaxCells) return wfail("n_services x (n_windows + 2) is above 2^20");
  return ISIM_OK;
}

extern "C" {

int isim_service_window_quantiles_table_words(const isim_handler *h, const isim_timeline_params *p, uint32_t n_q,
                                              uint64_t *words) {
  uint64_t ns = 0, cells = 0;
  if (const int rc = swq::check(h, p, nullptr, n_q, false, 0, ns, cells)) return rc;
  if (!words) return wfail("null argument");
  *words = swq::table_words(cells, n_q);
  return ISIM_OK;
}

int isim_service_window_quantiles_workspace_bytes(const isim_handler *h, const isim_timeline_params *p,
                                                  uint64_t cap_spans, uint32_t n_q, uint64_t *bytes) {
  uint64_t ns = 0, cells = 0;
  if (const int rc = swq::check(h, p, nullptr, n_q, false, cap_spans, ns, cells)) return rc;
  if (!bytes) return wfail("null argument");
  *bytes = swq::layout(cells, cap_spans, n_q).total;
  return ISIM_OK;
}

int isim_service_window_quantiles_host(const isim_handler *h, const isim_timeline_params *p, const uint32_t *q_ppm,
                                       uint32_t n_q, const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_out) {
  uint64_t ns = 0, cells = 0;
  if (const int rc = swq::check(h, p, q_ppm, n_q, true, n_spans, ns, cells)) return rc;
  if (!h_out) return wfail("null table");
  if (n_spans && !h_spans) return wfail("null spans");
  if (((uintptr_t)h_out & 7u) || ((uintptr_t)h_spans & 7u)) return wfail("the buffers must be 8-byte aligned");
  swq::RowArgs a{};
  isim::tl::set_row_args(a, *p);
  swq::fold_host(a, (uint32_t)ns, q_ppm, n_q, h_spans, n_spans, h_out);
  return ISIM_OK;
}

}  // extern "C"
