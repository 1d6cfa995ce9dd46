// The closed-loop client on the host (closed_loop.h): the
// checks of a caller's isim_closed_loop and batch, the schedule of one request
// and the rule as a plain sequential loop.  No HIP: these work without a GPU.
#include "closed_loop.h"
#include "error.h"

#include <string>
#include <vector>

namespace isim {
namespace cl {

const char *client_error(const Client *cl) {
  if (!cl) return "null client";
  if (cl->connections == 0 || cl->connections > kMaxConnections) return "connections must be in [1, 65536]";
  if (cl->flags & ~ISIM_CL_UNIFORM) return "flags must be 0 or ISIM_CL_UNIFORM";
  if (cl->period_ns > kMaxPeriod) return "period_ns must be 0 or in [1, 2^40]";
  return "";
}

const char *batch_error(const Client *cl, uint64_t n) {
  if (const char *m = client_error(cl); *m) return m;
  if (cl->first_index > kMaxFirst) return "first_index is above 2^40";
  if (n > kMaxN) return "n is above 2^32";
  if (n) {
    const uint32_t C = cl->connections;
    // the batch's largest scheduled start is its last request's: o_c < p, so no earlier row passes it
    const uint64_t j_last = cl->first_index + n - 1, k_max = j_last / C;
    const unsigned __int128 last = (unsigned __int128)offset_of((uint32_t)(j_last % C), C, cl->period_ns, cl->flags) +
                                   (unsigned __int128)k_max * cl->period_ns;
    if (last >= kScheduleEnd) return "the batch's last scheduled start would reach 2^63";
  }
  return "";
}

}  // namespace cl
}  // namespace isim

namespace {
namespace cl = isim::cl;
int cfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "closed loop: " + msg); }
}  // namespace

extern "C" {

int isim_closed_loop_schedule(const cl::Client *p, uint64_t j, uint32_t *c, uint64_t *s_ns) {
  if (const char *m = cl::client_error(p); *m) return cfail(m);
  if (!c || !s_ns) return cfail("null argument");
  const uint32_t C = p->connections, conn = (uint32_t)(j % C);
  const unsigned __int128 s =
      (unsigned __int128)cl::offset_of(conn, C, p->period_ns, p->flags) + (unsigned __int128)(j / C) * p->period_ns;
  if (s >= cl::kScheduleEnd) return cfail("the scheduled start would reach 2^63");
  *c = conn;
  *s_ns = (uint64_t)s;
  return ISIM_OK;
}

int isim_closed_loop_workspace_bytes(uint64_t n, uint32_t connections, uint64_t *bytes) {
  if (!bytes) return cfail("null argument");
  if (connections == 0 || connections > cl::kMaxConnections) return cfail("connections must be in [1, 65536]");
  if (n > cl::kMaxN) return cfail("n is above 2^32");
  *bytes = cl::workspace_bytes(n, connections);
  return ISIM_OK;
}

int isim_closed_loop_host(const cl::Client *p, const isim_trace_rec *h_records, uint64_t n, uint64_t *h_free_at,
                          uint64_t *h_arrivals, uint64_t *h_info) {
  if (const char *m = cl::batch_error(p, n); *m) return cfail(m);
  if (!h_info) return cfail("null h_info");
  if (n && (!h_records || !h_arrivals)) return cfail("null h_records or h_arrivals");
  const uint32_t C = p->connections;
  std::vector<uint64_t> zeros;
  uint64_t *F = h_free_at;
  if (!F) {
    zeros.assign(C, 0);
    F = zeros.data();
  }
  uint64_t late = 0, sum_late = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t j = p->first_index + i;
    const uint32_t c = (uint32_t)(j % C);
    const uint64_t s = cl::start_of(c, j / C, C, p->period_ns, p->flags);
    const uint64_t a = F[c] > s ? F[c] : s;
    h_arrivals[i] = a;
    F[c] = cl::sat_add(a, h_records[i].latency_ns);
    late += a > s;
    sum_late += a - s;
  }
  uint64_t hi = 0, lo = ~0ull;
  for (uint32_t c = 0; c < C; ++c) {
    hi = F[c] > hi ? F[c] : hi;
    lo = F[c] < lo ? F[c] : lo;
  }
  h_info[ISIM_CL_MAKESPAN] = hi;
  h_info[ISIM_CL_MIN_FREE] = lo;
  h_info[ISIM_CL_LATE] = late;
  h_info[ISIM_CL_SUM_LATE] = sum_late;
  return ISIM_OK;
}

}  // extern "C"
