// C ABI of libisim (include/isim.h): the thread's error slot, the graph and
// units entry points, handler creation, info and free, and the folds of a
// stats buffer.  The walk on a device is walk_host.hip, the DES des_host.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/isim.h"
#include "gounits.h"
#include "graph.h"
#include "handler.h"
#include "k8s.h"
#include "marshal.h"
#include "spans.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

}  // namespace

namespace isim {
// error reporting of the other C-ABI translation units (error.h)
int set_error(int code, const std::string &msg) { return fail(code, msg); }
}  // namespace isim

using isim::stats_words;
using isim::svc_dur_rows;

struct isim_graph {
  isim::ServiceGraph g;
};

// what spans.cpp and spans.hip read of a handler (spans.h)
isim::spans::HandlerView isim::spans::handler_view(const isim_handler *h) {
  isim_handler *m = const_cast<isim_handler *>(h);
  return HandlerView{&h->prog, &h->graph, &h->params, &m->span_mu, &m->span_state};
}

extern "C" {

const char *isim_last_error(void) { return g_err.c_str(); }
int isim_abi_version(void) { return ISIM_ABI_VERSION; }

int isim_graph_unmarshal_json(const char *json, size_t len, isim_graph **out) {
  if (!json || !out) return fail(ISIM_EINVAL, "null argument");
  isim_graph *g = new (std::nothrow) isim_graph();
  if (!g) return fail(ISIM_ENOMEM, "out of memory");
  std::string err;
  if (!isim::unmarshal_service_graph(json, len, g->g, err)) {
    delete g;
    return fail(ISIM_EPARSE, err);
  }
  *out = g;
  return ISIM_OK;
}

void isim_graph_free(isim_graph *g) { delete g; }

int isim_graph_num_services(const isim_graph *g) { return g ? (int)g->g.services.size() : -1; }

int isim_graph_canonical_json(const isim_graph *g, char *buf, size_t cap, size_t *len) {
  if (!g) return fail(ISIM_EINVAL, "null graph");
  std::string s = isim::canonical_json(g->g);
  if (len) *len = s.size() + 1;
  if (buf && cap) {
    size_t n = std::min(cap - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return ISIM_OK;
}

static int emit(const std::string &s, char *buf, size_t cap, size_t *len) {
  if (len) *len = s.size() + 1;
  if (buf && cap) {
    size_t n = std::min(cap - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return ISIM_OK;
}

int isim_graph_marshal_json(const isim_graph *g, char *buf, size_t cap, size_t *len) {
  if (!g) return fail(ISIM_EINVAL, "null graph");
  return emit(isim::marshal_json(g->g), buf, cap, len);
}

int isim_graph_to_dot(const isim_graph *g, char *buf, size_t cap, size_t *len) {
  if (!g) return fail(ISIM_EINVAL, "null graph");
  return emit(isim::to_dot(g->g), buf, cap, len);
}

int isim_graph_to_k8s_manifests(const isim_graph *g, const isim_k8s_params *p, char *buf, size_t cap, size_t *len) {
  if (!g || !p) return fail(ISIM_EINVAL, "null argument");
  std::string out, err;
  const int rc = isim::k8s_manifests(g->g, *p, out, err);
  if (rc != ISIM_OK) return fail(rc, err);
  return emit(out, buf, cap, len);
}

int isim_graph_marshal_yaml(const isim_graph *g, char *buf, size_t cap, size_t *len) {
  if (!g) return fail(ISIM_EINVAL, "null graph");
  const std::string y = isim::graph_yaml(g->g);
  if (y.empty()) return fail(ISIM_EINVAL, "graph marshal failed");
  return emit(y, buf, cap, len);
}

int isim_graph_service_index(const isim_graph *g, const char *name) {
  if (!g || !name) return -1;
  return isim::service_index(g->g, name);
}

int isim_size_from_string(const char *s, uint64_t *out) {
  if (!s || !out) return fail(ISIM_EINVAL, "null argument");
  std::string err;
  if (!isim::size_from_string(s, *out, err)) return fail(ISIM_EPARSE, err);
  return ISIM_OK;
}

int isim_duration_parse(const char *s, int64_t *out_ns) {
  if (!s || !out_ns) return fail(ISIM_EINVAL, "null argument");
  std::string err;
  if (!isim::go_parse_duration(s, *out_ns, err)) return fail(ISIM_EPARSE, err);
  return ISIM_OK;
}

int isim_percentage_from_string(const char *s, double *out) {
  if (!s || !out) return fail(ISIM_EINVAL, "null argument");
  std::string err;
  if (!isim::pct_from_string(s, *out, err)) return fail(ISIM_EPARSE, err);
  return ISIM_OK;
}

int isim_handler_create(const isim_graph *g, const char *service_name, const isim_params *p,
                        isim_handler **out) {
  if (!g || !p || !out) return fail(ISIM_EINVAL, "null argument");
  int32_t entry = -1;
  if (service_name) {
    entry = isim::service_index(g->g, service_name);
    if (entry < 0) return fail(ISIM_ENOTFOUND, std::string("service with name ") + service_name + " does not exist");
  } else {
    for (size_t i = 0; i < g->g.services.size(); ++i)
      if (g->g.services[i].is_entrypoint) {
        entry = (int32_t)i;
        break;
      }
    if (entry < 0) return fail(ISIM_EINVAL, "no service has isEntrypoint: true");
  }
  isim_handler *h = new (std::nothrow) isim_handler();
  if (!h) return fail(ISIM_ENOMEM, "out of memory");
  h->params = *p;
  std::string err;
  int rc = isim::compile_program(g->g, entry, *p, h->prog, err);
  if (rc == ISIM_OK) h->graph = g->g;  // for the DES plan (des_ensure); the caller may free g
  if (rc != ISIM_OK) {
    delete h;
    return fail(rc, err);
  }
  *out = h;
  return ISIM_OK;
}

void isim_handler_free(isim_handler *h) { delete h; }

int isim_handler_info_get(const isim_handler *h, isim_handler_info *out) {
  if (!h || !out) return fail(ISIM_EINVAL, "null argument");
  const isim::Program &p = h->prog;
  out->n_services = p.n_services;
  out->n_sites = p.n_sites;
  out->n_slots = p.n_slots;
  out->entry = p.entry;
  out->max_depth = p.max_depth;
  out->static_walk = p.static_walk ? 1 : 0;
  out->time_bits = p.time_bits;
  out->program_len = (int32_t)p.code.size();
  out->max_latency_ns = p.max_latency;
  out->hops_upper = p.hops_upper;
  out->stats_words = stats_words(h);
  out->svc_dur_rows = (int32_t)svc_dur_rows(h);
  out->n_reachable = (int32_t)p.row_svc.size();
  out->draw_groups = 0;
  for (size_t g = 0; g + 3 < p.stream.size(); g += 4)
    out->draw_groups += (p.stream[g].thr | p.stream[g + 1].thr | p.stream[g + 2].thr | p.stream[g + 3].thr) != 0;
  return ISIM_OK;
}

int isim_handler_slots(const isim_handler *h, int32_t *slot_site, int32_t *slot_callee) {
  if (!h) return fail(ISIM_EINVAL, "null handler");
  const isim::Program &p = h->prog;
  if (slot_site) std::copy(p.slot_site.begin(), p.slot_site.end(), slot_site);
  if (slot_callee) std::copy(p.slot_callee.begin(), p.slot_callee.end(), slot_callee);
  return ISIM_OK;
}

int isim_stats_fold(const isim_handler *h, const uint64_t *stats, uint64_t *svc_calls, uint64_t *svc_errs,
                    uint64_t *site_calls) {
  if (!h || !stats) return fail(ISIM_EINVAL, "null argument");
  const isim::Program &p = h->prog;
  if (svc_calls) std::fill(svc_calls, svc_calls + p.n_services, 0);
  if (svc_errs) std::fill(svc_errs, svc_errs + p.n_services, 0);
  if (site_calls) std::fill(site_calls, site_calls + p.n_sites, 0);
  const uint64_t *calls = stats + ISIM_ST_SITES;
  const uint64_t *errs = calls + p.n_slots;
  for (int32_t s = 0; s < p.n_slots; ++s) {
    if (svc_calls) svc_calls[p.slot_callee[s]] += calls[s];
    if (svc_errs) svc_errs[p.slot_callee[s]] += errs[s];
    if (site_calls) site_calls[p.slot_site[s]] += calls[s];
  }
  // the client request into the entry is not a call site
  if (svc_calls) svc_calls[p.entry] += stats[ISIM_ST_N_TRACES];
  if (svc_errs) svc_errs[p.entry] += stats[ISIM_ST_N_500];
  return ISIM_OK;
}

int isim_stats_fold_durations(const isim_handler *h, const uint64_t *stats, uint64_t *svc_dur) {
  if (!h || !stats || !svc_dur) return fail(ISIM_EINVAL, "null argument");
  const isim::Program &p = h->prog;
  constexpr uint32_t W = ISIM_SVC_DUR_WORDS;
  std::fill(svc_dur, svc_dur + (size_t)p.n_services * W, 0);
  if (!p.static_walk) {
    if (!svc_dur_rows(h)) return fail(ISIM_EINVAL, "per-service durations disabled (ISIM_FLAG_NO_SVC_DUR)");
    const uint64_t *tab = stats + ISIM_ST_SVC_DUR(p.n_slots);
    for (size_t r = 0; r < p.row_svc.size(); ++r)
      std::copy(tab + r * W, tab + (r + 1) * W, svc_dur + (size_t)p.row_svc[r] * W);
    return ISIM_OK;
  }
  // static walk: every invocation of s lasts T(s); split by code with the counters
  std::vector<uint64_t> calls(p.n_services, 0), errs(p.n_services, 0);
  isim_stats_fold(h, stats, calls.data(), errs.data(), nullptr);
  for (int32_t s : p.row_svc) {
    const uint64_t T = p.svc_time[s];
    const uint32_t b = isim::prom_bucket_ns(T);
    uint64_t *row = svc_dur + (size_t)s * W;
    row[b] = calls[s] - errs[s];
    row[ISIM_N_PROM + b] = errs[s];
    row[2 * ISIM_N_PROM] = T * (calls[s] - errs[s]);
    row[2 * ISIM_N_PROM + 1] = T * errs[s];
  }
  return ISIM_OK;
}

}  // extern "C"
