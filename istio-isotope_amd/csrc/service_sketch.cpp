// The per-service latency sketch on the host (service_sketch.h):
// the checks every entry point shares, the sizes, the fold of a list of spans
// (svs::fold_host), the merge of two tables and the brackets of one.  No HIP:
// these work without a GPU.
#include "service_sketch.h"

#include <string>

#include "error.h"
#include "spans.h"

namespace {
namespace svs = isim::svs;
namespace sk = isim::sk;
int kfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service sketch: " + msg); }

}  // namespace

// the handler, sub_bits, the span bound and the table's bound; n_services on success
int isim::svs::check_sizes(const isim_handler *h, uint32_t sub_bits, uint64_t n_spans, uint64_t &n_services) {
  if (!h) return kfail("null handler");
  if (const int rc = isim::svt::check_handler(h)) return rc;
  if (sub_bits > sk::kMaxSubBits) return kfail("sub_bits must be 0..7");
  if (n_spans > svq::kMaxSpans) return kfail("more than 2^32 - 1 spans");
  n_services = isim::spans::handler_view(h).graph->services.size();
  // n_services is a container's size, far below 2^40: the product does not wrap
  if (n_services > svq::kMaxServices) return kfail("more than 2^30 services");
  if (table_words(n_services, sub_bits) >= kMaxWords) return kfail("the table has 2^32 words or more");
  return ISIM_OK;
}

extern "C" {

int isim_service_sketch_table_words(const isim_handler *h, uint32_t sub_bits, uint64_t *words) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, 0, ns)) return rc;
  if (!words) return kfail("null argument");
  *words = svs::table_words(ns, sub_bits);
  return ISIM_OK;
}

int isim_service_sketch_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, 0, cap_spans, ns)) return rc;
  if (!bytes) return kfail("null argument");
  *bytes = svs::layout(ns, cap_spans).total;
  return ISIM_OK;
}

int isim_service_sketch_merge(const isim_handler *h, uint32_t sub_bits, uint64_t *dst, const uint64_t *src) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, 0, ns)) return rc;
  if (!dst || !src) return kfail("null argument");
  const uint64_t words = svs::table_words(ns, sub_bits);
  for (uint64_t i = 0; i < words; ++i) dst[i] += src[i];
  return ISIM_OK;
}

int isim_service_sketch_quantiles(const isim_handler *h, uint32_t sub_bits, const uint64_t *table,
                                  const uint32_t *q_ppm, uint32_t n_q, uint64_t *out) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, 0, ns)) return rc;
  if (!table || !out) return kfail("null table or out");
  // the quantile list is isim_sketch_quantiles' to refuse: also with no service
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return kfail(m);
  const uint64_t bw = svs::block_words(sub_bits), ow = ISIM_SKQ_OUT_WORDS(n_q);
  for (uint64_t b = 0; b < ns * svs::kMeasures; ++b)
    if (const int rc = isim_sketch_quantiles(sub_bits, table + b * bw, q_ppm, n_q, out + b * ow)) return rc;
  return ISIM_OK;
}

int isim_service_sketch_host(const isim_handler *h, uint32_t sub_bits, const isim_des_span *h_spans, uint64_t n_spans,
                             uint64_t *h_table) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, n_spans, ns)) return rc;
  if (!h_table) return kfail("null table");
  if (n_spans && !h_spans) return kfail("null spans");
  if (((uintptr_t)h_table & 7u) || ((uintptr_t)h_spans & 7u)) return kfail("the buffers must be 8-byte aligned");
  svs::fold_host((uint32_t)ns, sub_bits, h_spans, n_spans, h_table);
  return ISIM_OK;
}

}  // extern "C"
