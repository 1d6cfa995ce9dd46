// Per-service percentiles on the host (service_quantiles.h): the
// checks every entry point shares, the sizes and the table of a list of spans
// (svq::fold_host).  No HIP: these work without a GPU.
#include "service_quantiles.h"

#include <string>

#include "error.h"
#include "spans.h"

namespace {
namespace svq = isim::svq;
int qfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service quantiles: " + msg); }

}  // namespace

// the handler and the number of quantiles; n_services on success
int isim::svq::check_sizes(const isim_handler *h, uint32_t n_q, uint64_t n_spans, uint64_t &n_services) {
  if (!h) return qfail("null handler");
  if (const int rc = isim::svt::check_handler(h)) return rc;
  if (n_q == 0 || n_q > ISIM_MAX_QUANTILES) return qfail("n_q must be 1.." + std::to_string(ISIM_MAX_QUANTILES));
  if (n_spans > svq::kMaxSpans) return qfail("more than 2^32 - 1 spans");
  n_services = isim::spans::handler_view(h).graph->services.size();
  if (n_services > svq::kMaxServices) return qfail("more than 2^30 services");
  return ISIM_OK;
}

int isim::svq::check(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q, uint64_t n_spans,
                     uint64_t &n_services) {
  if (const int rc = check_sizes(h, n_q, n_spans, n_services)) return rc;
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return qfail(m);
  return ISIM_OK;
}

extern "C" {

int isim_service_quantiles_table_words(const isim_handler *h, uint32_t n_q, uint64_t *words) {
  uint64_t ns = 0;
  if (const int rc = svq::check_sizes(h, n_q, 0, ns)) return rc;
  if (!words) return qfail("null argument");
  *words = svq::table_words(ns, n_q);
  return ISIM_OK;
}

int isim_service_quantiles_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint32_t n_q, uint64_t *bytes) {
  uint64_t ns = 0;
  if (const int rc = svq::check_sizes(h, n_q, cap_spans, ns)) return rc;
  if (!bytes) return qfail("null argument");
  *bytes = svq::layout(ns, cap_spans, n_q).total;
  return ISIM_OK;
}

int isim_service_quantiles_host(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q,
                                const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_out) {
  uint64_t ns = 0;
  if (const int rc = svq::check(h, q_ppm, n_q, n_spans, ns)) return rc;
  if (!h_out) return qfail("null table");
  if (n_spans && !h_spans) return qfail("null spans");
  if (((uintptr_t)h_out & 7u) || ((uintptr_t)h_spans & 7u)) return qfail("the buffers must be 8-byte aligned");
  svq::fold_host((uint32_t)ns, q_ppm, n_q, h_spans, n_spans, h_out);
  return ISIM_OK;
}

}  // extern "C"
