// The DES side of the C ABI (BASELINE config 5): the plan and
// its upload, both engines' batch entry points, the arrivals and load-profile
// entry points (§17), the span tap (§21) and the wait table's helpers.  Host
// code; the kernels are in des.hip, des_items.hip and load_profile.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "des_critical_path.h"
#include "handler.h"
#include "host_stage.h"
#include "service_timeline.h"
#include "spans.h"

using isim::set_error;

namespace {

using isim::DevState;

// Builds the DES plan on first use (host only); ISIM_OK or the reason the
// graph is outside the DES class.
int des_ensure(const isim_handler *hc) {
  isim_handler *h = const_cast<isim_handler *>(hc);
  std::lock_guard<std::mutex> lk(h->des_mu);
  if (!h->des_built) {
    h->des_rc = isim::build_des_plan(h->graph, h->prog, h->params.error_mode == ISIM_MODE_B, h->des, h->des_err);
    h->des_built = true;
  }
  return h->des_rc == ISIM_OK ? ISIM_OK : set_error(h->des_rc, h->des_err);
}

// the plan's device copies; on failure the caller drops whatever `t` holds by then
int upload_des(const isim_handler *h, int device, isim::DesTables &t) {
  using isim::upload;
  const isim::DesPlan &d = h->des;
  std::vector<uint32_t> pipe(d.pipe_pos);
  pipe.insert(pipe.end(), d.pipe_dep.begin(), d.pipe_dep.end());
  if (upload(t.pos, d.pos) || upload(t.child, d.child) || upload(t.level, d.fin_pos) || upload(t.arr, d.arr_ops) ||
      upload(t.ext, d.ext) || upload(t.steps, d.steps) || upload(t.mult, d.slot_mult) || upload(t.fast, d.fast_pos) ||
      upload(t.sort, d.sort_pos) || upload(t.zero, d.zero_pos) || upload(t.pipe, pipe))
    return set_error(ISIM_EHIP, "DES plan upload failed");
  if (!d.items) return ISIM_OK;
  const isim::Program &p = h->prog;
  // the per-batch item arrays come from a pool of this handler's own (kept
  // between batches: a release threshold of ~0 on a pool nobody else uses)
  hipMemPoolProps props{};
  props.allocType = hipMemAllocationTypePinned;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = device;
  uint64_t keep = ~0ull;
  hipMemPool_t pool = nullptr;
  if (hipMemPoolCreate(&pool, &props) != hipSuccess) return set_error(ISIM_EHIP, "DES item pool creation failed");
  t.pool.reset(pool);
  if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess)
    return set_error(ISIM_EHIP, "DES item pool creation failed");
  if (upload(t.ipos, d.item_pos) || upload(t.sround, d.step_round) ||
      (p.tree_wide ? upload(t.nodes, p.tree_nodes_w) : upload(t.nodes, p.tree_nodes)) || upload(t.text, p.tree_ext) ||
      upload(t.tstep, p.tree_step))
    return set_error(ISIM_EHIP, "DES plan upload failed");
  return ISIM_OK;
}

int des_prepare(isim_handler *h, int device, DevState *&st) {
  int rc = des_ensure(h);
  if (rc != ISIM_OK) return rc;
  rc = isim::prepare_device(h, device, st);
  if (rc != ISIM_OK) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (st->des.ready) return ISIM_OK;
  st->des = isim::DesTables{};  // the remains of an earlier attempt that failed part-way
  rc = upload_des(h, device, st->des);
  if (rc != ISIM_OK) st->des = isim::DesTables{};
  st->des.ready = rc == ISIM_OK;
  return rc;
}

uint64_t des_ws_bytes(const isim_handler *h, uint64_t n_traces) {
  return h->des.items ? isim::des_items_workspace_bytes(n_traces)
                      : isim::des_workspace_bytes(h->des, n_traces, isim::stats_words(h), h->prog.row_svc.size());
}

// The offered load of one DES batch: a constant mean, or a compiled profile
// with the batch's horizon (load_profile.h).
struct DesLoad {
  uint64_t mean_ns;
  const isim::lp::Compiled *profile;  // null: mean_ns
  uint64_t horizon;                   // profile: no arrival of the batch passes it (< 2^62)
  uint32_t flags;                     // 0 or ISIM_DES_FLAG_WIDE
  const isim_des_tap *tap = nullptr;  // the span tap: item engine only, checked by the caller
};

// One DES batch on the current device, the arguments checked by the caller:
// under load.mean_ns, or under load.profile with its horizon.
int serve_des_device(isim_handler *h, const DesLoad &load, uint64_t trace_begin, uint64_t n_traces,
                     isim_trace_rec *d_records, uint64_t *d_stats, uint64_t *d_des_table, void *d_workspace,
                     uint64_t workspace_bytes, void *hip_stream) {
  // no arrival of the batch passes this time (an exponential gap is at most 24 ln 2 = 16.6 means)
  const long double arrival_span =
      load.profile ? (long double)load.horizon : (long double)n_traces * load.mean_ns * 17.0L;
  int device = 0;
  ISIM_HIPCHK(hipGetDevice(&device));
  DevState *st = nullptr;
  int rc = des_prepare(h, device, st);
  if (rc != ISIM_OK) return rc;
  const isim::DesPlan &d = h->des;
  isim::DesTables &t = st->des;
  // the profile's table goes up on the stream once every check has passed, just ahead of the batch that
  // reads it: a refused call leaves the stream and the handler's table as they were
  isim::lp::DeviceProfile dprof_store{};
  auto upload_profile = [&](const isim::lp::DeviceProfile *&out) -> int {
    out = nullptr;
    if (!load.profile) return ISIM_OK;
    {
      std::lock_guard<std::mutex> lk(h->mu);
      if (!t.lp_table && isim::alloc(t.lp_table, isim::lp::table_bytes(isim::lp::kMaxSegments)) != ISIM_OK)
        return set_error(ISIM_EHIP, "hipMalloc(load profile table) failed");
    }
    if (isim::lp::upload(*load.profile, t.lp_table.get(), hip_stream) != 0)
      return set_error(ISIM_EHIP, "load profile upload failed");
    dprof_store = {t.lp_table.get(), (uint32_t)load.profile->seg.size(), load.profile->paced() ? 1u : 0u};
    out = &dprof_store;
    return ISIM_OK;
  };
  if (d.items) {
    // a dynamic walk: the item engine (des_items.hip); 64-bit times throughout
    if (!d_workspace || workspace_bytes < isim::des_items_workspace_bytes(n_traces))
      return set_error(ISIM_EINVAL, "DES workspace smaller than isim_des_workspace_bytes()");
    isim::DesItemsLaunch L{};
    L.plan = &d;
    L.d_pos = t.pos.get();
    L.d_item_pos = t.ipos.get();
    L.d_steps = t.steps.get();
    L.d_step_round = t.sround.get();
    L.d_nodes = t.nodes.get();
    L.d_ext = t.text.get();
    L.d_tstep = t.tstep.get();
    L.tree_frames = h->prog.tree_frames;
    L.tree_t64 = h->prog.tree_t64 ? 1u : 0u;
    L.tree_flags = h->prog.tree_flags;
    L.n_nodes = h->prog.tree_positions();
    L.tree_wide = h->prog.tree_wide ? 1u : 0u;
    L.workspace = d_workspace;
    L.d_stats = d_stats;
    L.d_table = d_des_table;
    L.d_records = d_records;
    L.n_traces = n_traces;
    L.trace_begin = trace_begin;
    L.mean_ns = load.mean_ns;
    L.seed = h->params.seed;
    L.n_slots = (uint32_t)h->prog.n_slots;
    L.flags = h->params.flags;
    L.pool = t.pool.get();
    // the workers of this batch (handler state, read here once): per duration-table row; none set, or all 1,
    // is the engine without pools
    std::vector<uint32_t> row_workers;
    {
      std::lock_guard<std::mutex> lk(h->mu);
      if (std::any_of(h->des_workers.begin(), h->des_workers.end(), [](uint32_t w) { return w > 1; })) {
        row_workers.resize(h->prog.row_svc.size());
        for (size_t r = 0; r < row_workers.size(); ++r) row_workers[r] = h->des_workers[h->prog.row_svc[r]];
      }
    }
    L.row_workers = row_workers.empty() ? nullptr : row_workers.data();
    isim::DesItemsReport rep{};
    L.report = &rep;
    if (load.tap) {  // the slot-to-callee table of the span code (uploaded once per handler and device)
      isim::spans::DevTables tabs;
      if (const int trc = isim::spans::device_tables(isim::spans::handler_view(h), tabs)) return trc;
      L.tap = load.tap;
      L.d_slot_callee = tabs.slot_callee;
      L.entry_service = (uint32_t)h->prog.entry;
      L.n_services = (uint32_t)h->prog.n_services;
    }
    if (const int urc = upload_profile(L.profile)) return urc;
    std::string e;
    const int irc = isim::des_items_launch(L, hip_stream, e);
    {
      std::lock_guard<std::mutex> lk(h->report_mu);
      h->des_report = rep;
    }
    if (irc == 2) return set_error(ISIM_EINVAL, e);
    if (irc) return set_error(ISIM_EHIP, e);
    return ISIM_OK;
  }
  if (n_traces * (uint64_t)std::max<uint32_t>(1, d.max_sort_pos) > 0xFFFFFFFFull)
    return set_error(ISIM_EINVAL, "n_traces x positions of one service above 2^32 per DES batch");
  // the queue scans' keys a_t - t * hold are signed 64-bit (des.hip down passes)
  if ((long double)n_traces * (long double)d.max_hold + arrival_span >= std::ldexp(1.0L, 62))
    return set_error(ISIM_EINVAL, "DES batch too long for its worker hold times (n_traces x hold above 2^62 ns)");
  if (d.max_rep_bits) {
    // sort keys hold replica | arrival: the batch's arrival span plus the static latency must fit
    const long double span = arrival_span + (long double)h->prog.max_latency;
    if (span >= std::ldexp(1.0L, 64 - (int)d.max_rep_bits - 1))
      return set_error(ISIM_EINVAL, "DES batch too long for the sort keys of a replicated service (arrival span)");
  }
  const uint64_t words = isim::stats_words(h);
  const uint32_t rows = (uint32_t)h->prog.row_svc.size();
  if (!d_workspace || workspace_bytes < isim::des_workspace_bytes(d, n_traces, words, rows))
    return set_error(ISIM_EINVAL, "DES workspace smaller than isim_des_workspace_bytes()");
  isim::DesLaunch L{};
  L.plan = &d;
  L.d_pos = t.pos.get();
  L.d_ext = t.ext.get();
  L.d_steps = t.steps.get();
  L.d_child = t.child.get();
  L.d_fin_pos = t.level.get();
  L.d_arr_ops = t.arr.get();
  L.d_fast_pos = t.fast.get();
  L.d_zero_pos = t.zero.get();
  L.d_pipe = t.pipe.get();
  L.d_sort_pos = t.sort.get();
  L.d_mult = t.mult.get();
  L.d_stats = d_stats;
  L.d_table = d_des_table;
  L.d_records = d_records;
  L.n_traces = n_traces;
  L.trace_begin = trace_begin;
  L.mean_ns = load.mean_ns;
  L.seed = h->params.seed;
  L.stats_words = words;
  L.table_rows = rows;
  L.n_pos = (uint32_t)d.pos.size();
  L.n_slots = (uint32_t)h->prog.n_slots;
  L.modeb = h->params.error_mode == ISIM_MODE_B ? 1u : 0u;
  L.wide = (load.flags & ISIM_DES_FLAG_WIDE) != 0;
  if (const int urc = upload_profile(L.profile)) return urc;
  isim::des_carve(L, d_workspace);
  if (isim::des_launch(L, hip_stream) != 0) return set_error(ISIM_EHIP, "DES kernel launch failed");
  return ISIM_OK;
}

// The synchronous call of both entry points: host buffers, 32-bit rows first
// and 64-bit rows on retry.  `enqueue` validates one batch's arguments and
// enqueues it with the given row flags (isim_serve_des_device, or the profile twin).
template <typename Enqueue>
int serve_des_host(isim_handler *h, int device, uint32_t flags0, uint64_t n_traces, isim_trace_rec *h_records,
                   uint64_t *h_stats, uint64_t *h_des_table, Enqueue enqueue, bool device_records = false) {
  const uint64_t words = isim::stats_words(h);
  const uint64_t tab_words = (uint64_t)h->prog.row_svc.size() * ISIM_DES_ROW_WORDS;
  const uint64_t ws_bytes = des_ws_bytes(h, n_traces);
  const uint64_t rec_bytes = h_records || device_records ? n_traces * sizeof(isim_trace_rec) : 0;
  isim::HostStage stage(device);
  uint64_t *d_stats = (uint64_t *)stage.alloc(words * 8), *d_tab = (uint64_t *)stage.alloc(tab_words * 8 + 8);
  void *d_ws = stage.alloc(ws_bytes + 8);
  isim_trace_rec *d_rec = (isim_trace_rec *)stage.alloc(rec_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  const hipStream_t s = stage.stream();
  // 32-bit rows first; a batch they cannot hold (ISIM_ST_DES_RETRY) again with 64-bit rows
  uint32_t flags = flags0;
  for (int pass = 0; pass < 2; ++pass) {
    if (hipMemsetAsync(d_stats, 0, words * 8, s) != hipSuccess ||
        hipMemsetAsync(d_tab, 0, tab_words * 8 + 8, s) != hipSuccess)
      return set_error(ISIM_EHIP, "hipMemset failed");
    if (const int rc = enqueue(flags, d_rec, d_stats, d_tab, d_ws, ws_bytes + 8, s)) return rc;
    uint64_t retry = 0;
    if (hipMemcpyAsync(&retry, d_stats + ISIM_ST_DES_RETRY, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return set_error(ISIM_EHIP, "DES retry check failed");
    if (!retry) break;
    if (retry >= isim::kDesFaultUnit)
      return set_error(ISIM_EHIP, "DES batch failed: a queue pass's look-back gave up waiting for an earlier chunk "
                                  "(device fault flag); the batch was not accumulated");
    if ((flags & ISIM_DES_FLAG_WIDE) || h->des.items)
      return set_error(ISIM_EINVAL, "DES batch not accumulated with 64-bit rows: the cyclic schedule found no fixed "
                                    "point within 4096 passes (or arrivals beyond the sort keys)");
    flags |= ISIM_DES_FLAG_WIDE;
  }
  if (h_stats)
    if (const int rc = stage.download(h_stats, d_stats, words * 8)) return rc;
  if (h_des_table)
    if (const int rc = stage.download(h_des_table, d_tab, tab_words * 8)) return rc;
  return stage.download(h_records, d_rec, h_records ? rec_bytes : 0);
}

// ---- the checks of the entry points, all on the host before any HIP call

int des_params_check(const isim_des_params *dp) {
  if (dp->mean_interarrival_ns == 0 || dp->mean_interarrival_ns > (1ull << 34))
    return set_error(ISIM_EINVAL, "mean_interarrival_ns must be in [1, 2^34]");
  if (dp->reserved != 0 || (dp->flags & ~ISIM_DES_FLAG_WIDE) != 0)
    return set_error(ISIM_EINVAL, "isim_des_params.flags must be 0 or ISIM_DES_FLAG_WIDE, reserved 0");
  return ISIM_OK;
}

// the load of a batch under a constant mean
int mean_des_check(const isim_des_params *dp, uint64_t n_traces, DesLoad &load) {
  if (const int rc = des_params_check(dp)) return rc;
  if (n_traces > (1ull << 31)) return set_error(ISIM_EINVAL, "n_traces above 2^31 per DES batch");
  load = DesLoad{dp->mean_interarrival_ns, nullptr, 0, dp->flags};
  return ISIM_OK;
}

int profile_compile(const isim_load_profile *lp, isim::lp::Compiled &c) {
  std::string e;
  const int rc = isim::lp::compile(lp, c, e);
  return rc == ISIM_OK ? ISIM_OK : set_error(rc, e);
}

// the batch's horizon, or ISIM_EINVAL: the device's sums and products need it below 2^62
int profile_horizon(const isim::lp::Compiled &c, uint64_t n_traces, uint64_t &t) {
  if (!isim::lp::horizon(c, n_traces, t))
    return set_error(ISIM_EINVAL, "load profile: the batch's horizon (the time at the largest work its traces can "
                                  "reach) is at or above 2^62 ns");
  return ISIM_OK;
}

// the load of a batch under a profile
int profile_des_check(isim_handler *h, const isim_load_profile *lp, uint32_t des_flags, uint64_t n_traces,
                      isim::lp::Compiled &c, DesLoad &load) {
  if (!h) return set_error(ISIM_EINVAL, "null argument");
  if (const int rc = profile_compile(lp, c)) return rc;
  if (des_flags & ~ISIM_DES_FLAG_WIDE) return set_error(ISIM_EINVAL, "des_flags must be 0 or ISIM_DES_FLAG_WIDE");
  if (n_traces > (1ull << 31)) return set_error(ISIM_EINVAL, "n_traces above 2^31 per DES batch");
  load = DesLoad{0, &c, 0, des_flags};
  return profile_horizon(c, n_traces, load.horizon);
}

// the load of isim_serve_des_spans*: under a profile the parameters carry the row flags alone
int spans_load_check(isim_handler *h, const isim_des_params *dp, const isim_load_profile *lp, uint64_t n_traces,
                     isim::lp::Compiled &c, DesLoad &load) {
  if (!lp) return mean_des_check(dp, n_traces, load);
  if (dp->reserved != 0) return set_error(ISIM_EINVAL, "isim_des_params.reserved must be 0");
  return profile_des_check(h, lp, dp->flags, n_traces, c, load);
}

int tfail(const std::string &msg) { return set_error(ISIM_EINVAL, "DES spans: " + msg); }

// a handler that has DES spans: its DES runs on the item engine
int des_items_check(const isim_handler *h) {
  if (const int drc = des_ensure(h)) return drc;
  if (!h->des.items)
    return tfail("this handler's DES runs on the static engine, which keeps no invocations: create the handler "
                 "with ISIM_FLAG_DYNAMIC");
  return ISIM_OK;
}

// every check of a tap that needs no GPU; `aligned`: the five pointers are device buffers
int des_tap_check(const isim_handler *h, const isim_des_tap *tap, bool have_records, bool aligned) {
  if (const int hrc = des_items_check(h)) return hrc;
  if (!have_records) return tfail("a tap needs d_records");
  if (tap->reserved[0] || tap->reserved[1]) return tfail("isim_des_tap.reserved must be 0");
  if (tap->cls > ISIM_Q_500) return tfail("the class must be ISIM_Q_ALL, ISIM_Q_200 or ISIM_Q_500");
  if (tap->q_ppm > 1000000u) return tfail("q_ppm is above 1000000");
  if (tap->max_traces > (1ull << 32)) return tfail("max_traces is above 2^32");
  if (tap->cap_spans > (1ull << 40)) return tfail("cap_spans is above 2^40");
  if (!tap->d_off || !tap->d_info || (tap->max_traces && !tap->d_ids) || (tap->cap_spans && !tap->d_spans))
    return tfail("null tap buffer");
  if (aligned && ((((uintptr_t)tap->d_ids | (uintptr_t)tap->d_off | (uintptr_t)tap->d_info |
                    (uintptr_t)tap->d_wait_table) & 7u) || ((uintptr_t)tap->d_spans & 15u)))
    return tfail("the tap's buffers must be 8-byte aligned, d_spans 16-byte aligned");
  return ISIM_OK;
}

// The device buffers of a batch whose load has passed its check: null
// pointers, the tap when there is one, alignment, the workspace's size.  A
// batch of no traces without a tap does nothing: its buffers are looked at no further.
int des_buffers_check(const isim_handler *h, const isim_des_tap *tap, uint64_t n_traces,
                      const isim_trace_rec *d_records, const uint64_t *d_stats, const uint64_t *d_des_table,
                      const void *d_workspace, uint64_t workspace_bytes) {
  if (!d_stats || !d_des_table) return set_error(ISIM_EINVAL, "null argument");
  if (tap) {
    if (const int rc = des_tap_check(h, tap, d_records || !n_traces, true)) return rc;
  } else if (n_traces == 0) {
    return ISIM_OK;
  }
  if (((uintptr_t)d_stats & 7u) || ((uintptr_t)d_des_table & 7u) || ((uintptr_t)d_workspace & 7u) ||
      ((uintptr_t)d_records & 15u))
    return set_error(ISIM_EINVAL, "d_stats, d_des_table and d_workspace must be 8-byte, d_records 16-byte aligned");
  if (n_traces == 0) return ISIM_OK;
  if (const int drc = des_ensure(h)) return drc;
  if (!d_workspace || workspace_bytes < des_ws_bytes(h, n_traces))
    return set_error(ISIM_EINVAL, "DES workspace smaller than isim_des_workspace_bytes()");
  return ISIM_OK;
}

// ---- the arrival times alone (the engine's kernels, des.hip des_arrivals_launch)
uint64_t des_arrivals_ws_bytes(uint64_t n) { return ((isim::des_arrivals_blocks(n) + 1) * 8 + 255) & ~255ull; }

int des_arrivals_check(const isim_handler *h, const isim_des_params *dp, uint64_t n_traces, const void *out) {
  if (!h || !dp) return set_error(ISIM_EINVAL, "null argument");
  if (const int rc = des_params_check(dp)) return rc;
  if (n_traces > (1ull << 40)) return set_error(ISIM_EINVAL, "n_traces above 2^40");
  if (n_traces && !out) return set_error(ISIM_EINVAL, "null arrivals buffer");
  return ISIM_OK;
}

// chunk sums, then the segment table (always room for ISIM_LP_MAX_SEGMENTS: the size depends on n alone)
uint64_t profile_arrivals_blk_bytes(uint64_t n) { return ((isim::lp::arrival_blocks(n) + 1) * 8 + 255) & ~255ull; }
uint64_t profile_arrivals_ws_bytes(uint64_t n) {
  return profile_arrivals_blk_bytes(n) + ((isim::lp::table_bytes(isim::lp::kMaxSegments) + 255) & ~255ull);
}

int profile_arrivals_check(const isim_handler *h, const isim_load_profile *lp, uint64_t n_traces, const void *out,
                           isim::lp::Compiled &c) {
  if (!h) return set_error(ISIM_EINVAL, "null argument");
  if (const int rc = profile_compile(lp, c)) return rc;
  if (n_traces > isim::lp::kMaxTraces) return set_error(ISIM_EINVAL, "n_traces above 2^32 per profile arrivals call");
  if (n_traces && !out) return set_error(ISIM_EINVAL, "null arrivals buffer");
  uint64_t t;
  return profile_horizon(c, n_traces, t);
}

// the workspace and alignment of both arrivals calls; `api`: the function that sizes the workspace
int arrivals_buffers_check(const void *d_arrivals, const void *d_workspace, uint64_t workspace_bytes, uint64_t need,
                           const char *api) {
  if (!d_workspace || workspace_bytes < need)
    return set_error(ISIM_EINVAL, std::string("arrivals workspace smaller than ") + api + "()");
  if (((uintptr_t)d_arrivals & 7u) || ((uintptr_t)d_workspace & 7u))
    return set_error(ISIM_EINVAL, "d_arrivals and d_workspace must be 8-byte aligned");
  return ISIM_OK;
}

}  // namespace

// des_critical_path.h: the handlers isim_serve_des_spans_device refuses with a tap
int isim::dcp::check_handler(const isim_handler *h) {
  if (!h) return set_error(ISIM_EINVAL, "DES critical path: null handler");
  return des_items_check(h);
}

// service_timeline.h: the same handlers
int isim::svt::check_handler(const isim_handler *h) {
  if (!h) return set_error(ISIM_EINVAL, "service timeline: null handler");
  return des_items_check(h);
}

extern "C" {

int isim_des_info_get(const isim_handler *h, isim_des_info *out) {
  if (!h || !out) return set_error(ISIM_EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (const int drc = des_ensure(h)) return drc;
  out->n_positions = (int32_t)h->des.pos.size();
  out->n_levels = (int32_t)h->des.n_levels;
  out->max_width = (int32_t)h->des.max_width;
  out->table_rows = (int32_t)h->prog.row_svc.size();
  for (const auto &q : h->des.pos) out->n_fused += (q.flags & isim::kDesFlagFused) ? 1 : 0;
  out->cyclic = h->des.cyclic ? 1 : 0;
  uint32_t rr = 0, rw = 0;
  isim::des_row_traffic(h->des, rr, rw);
  out->row_reads = (int32_t)rr;
  out->row_writes = (int32_t)rw;
  out->items = h->des.items ? 1 : 0;
  return ISIM_OK;
}

// ---- worker pools: host state, every check before any HIP call
int isim_des_workers_set(isim_handler *h, const uint32_t *workers, uint32_t n_services) {
  if (!h) return set_error(ISIM_EINVAL, "DES workers: null handler");
  if (!workers) {  // every service back to one worker
    std::lock_guard<std::mutex> lk(h->mu);
    h->des_workers.clear();
    return ISIM_OK;
  }
  if (n_services != (uint32_t)h->prog.n_services)
    return set_error(ISIM_EINVAL, "DES workers: n_services is " + std::to_string(n_services) + ", the graph has " +
                                      std::to_string(h->prog.n_services) + " services");
  bool pooled = false;
  for (uint32_t s = 0; s < n_services; ++s) {
    if (workers[s] == 0 || workers[s] > isim::kDesMaxWorkers)
      return set_error(ISIM_EINVAL, "DES workers: service " + std::to_string(s) + " has " + std::to_string(workers[s]) +
                                        " workers, outside 1 .. 65536");
    pooled = pooled || workers[s] > 1;
  }
  if (pooled) {
    if (const int drc = des_ensure(h)) return drc;
    if (!h->des.items)
      return set_error(ISIM_EINVAL, "DES workers: more than one worker per replica needs the item engine, and this "
                                    "handler's DES runs on the static engine: create the handler with "
                                    "ISIM_FLAG_DYNAMIC");
    if (h->des.cyclic)
      return set_error(ISIM_EINVAL, "DES workers: more than one worker per replica on a cyclic call-step schedule "
                                    "(isim_des_info.cyclic) is not built");
  }
  std::lock_guard<std::mutex> lk(h->mu);
  h->des_workers.assign(workers, workers + n_services);
  return ISIM_OK;
}

int isim_des_workers_get(const isim_handler *h, uint32_t *workers) {
  if (!h || !workers) return set_error(ISIM_EINVAL, "DES workers: null argument");
  isim_handler *hm = const_cast<isim_handler *>(h);
  std::lock_guard<std::mutex> lk(hm->mu);
  for (int32_t s = 0; s < h->prog.n_services; ++s) workers[s] = h->des_workers.empty() ? 1u : h->des_workers[s];
  return ISIM_OK;
}

int isim_des_last_batch(const isim_handler *h, isim_des_batch_stats *out) {
  if (!h || !out) return set_error(ISIM_EINVAL, "null argument");
  isim_handler *hm = const_cast<isim_handler *>(h);
  std::lock_guard<std::mutex> lk(hm->report_mu);
  out->passes = h->des_report.passes;
  out->syncs = h->des_report.syncs;
  out->items = h->des_report.items;
  return ISIM_OK;
}

int isim_des_workspace_bytes(const isim_handler *h, uint64_t n_traces, uint64_t *bytes) {
  if (!h || !bytes) return set_error(ISIM_EINVAL, "null argument");
  if (const int drc = des_ensure(h)) return drc;
  *bytes = des_ws_bytes(h, n_traces);
  return ISIM_OK;
}

int isim_serve_des_device(isim_handler *h, const isim_des_params *dp, uint64_t trace_begin, uint64_t n_traces,
                          isim_trace_rec *d_records, uint64_t *d_stats, uint64_t *d_des_table, void *d_workspace,
                          uint64_t workspace_bytes, void *hip_stream) {
  if (!h || !dp || !d_stats || !d_des_table) return set_error(ISIM_EINVAL, "null argument");
  DesLoad load{};
  if (const int rc = mean_des_check(dp, n_traces, load)) return rc;
  if (n_traces == 0) return ISIM_OK;
  return serve_des_device(h, load, trace_begin, n_traces, d_records, d_stats, d_des_table, d_workspace,
                          workspace_bytes, hip_stream);
}

int isim_serve_des(isim_handler *h, int device, const isim_des_params *dp, uint64_t trace_begin, uint64_t n_traces,
                   isim_trace_rec *h_records, uint64_t *h_stats, uint64_t *h_des_table) {
  if (!h || !dp) return set_error(ISIM_EINVAL, "null argument");
  if (const int drc = des_ensure(h)) return drc;
  return serve_des_host(h, device, dp->flags, n_traces, h_records, h_stats, h_des_table,
                        [&](uint32_t flags, isim_trace_rec *d_rec, uint64_t *d_stats, uint64_t *d_tab, void *d_ws,
                            uint64_t ws_bytes, hipStream_t s) {
                          isim_des_params p = *dp;
                          p.flags = flags;
                          return isim_serve_des_device(h, &p, trace_begin, n_traces, d_rec, d_stats, d_tab, d_ws,
                                                       ws_bytes, s);
                        });
}

int isim_des_arrivals_workspace_bytes(uint64_t n_traces, uint64_t *bytes) {
  if (!bytes) return set_error(ISIM_EINVAL, "null argument");
  if (n_traces > (1ull << 40)) return set_error(ISIM_EINVAL, "n_traces above 2^40");
  *bytes = des_arrivals_ws_bytes(n_traces);
  return ISIM_OK;
}

int isim_des_arrivals_device(const isim_handler *h, const isim_des_params *dp, uint64_t trace_begin,
                             uint64_t n_traces, uint64_t *d_arrivals, void *d_workspace, uint64_t workspace_bytes,
                             void *hip_stream) {
  if (const int rc = des_arrivals_check(h, dp, n_traces, d_arrivals)) return rc;
  if (n_traces == 0) return ISIM_OK;
  if (const int rc = arrivals_buffers_check(d_arrivals, d_workspace, workspace_bytes, des_arrivals_ws_bytes(n_traces),
                                            "isim_des_arrivals_workspace_bytes"))
    return rc;
  if (isim::des_arrivals_launch(h->params.seed, dp->mean_interarrival_ns, trace_begin, n_traces, d_arrivals,
                                (uint64_t *)d_workspace, hip_stream) != 0)
    return set_error(ISIM_EHIP, "arrivals kernel launch failed");
  return ISIM_OK;
}

int isim_des_arrivals(const isim_handler *h, int device, const isim_des_params *dp, uint64_t trace_begin,
                      uint64_t n_traces, uint64_t *h_arrivals) {
  if (const int rc = des_arrivals_check(h, dp, n_traces, h_arrivals)) return rc;
  if (n_traces == 0) return ISIM_OK;
  const uint64_t ws_bytes = des_arrivals_ws_bytes(n_traces);
  isim::HostStage stage(device);
  void *d_a = stage.alloc(n_traces * 8), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_des_arrivals_device(h, dp, trace_begin, n_traces, (uint64_t *)d_a, d_ws, ws_bytes,
                                              stage.stream()))
    return rc;
  return stage.download(h_arrivals, d_a, n_traces * 8);
}

// ---- load profiles (load_profile.h, load_profile.hip)
int isim_load_profile_time(const isim_load_profile *lp, uint64_t work_q24, uint64_t *t_ns) {
  if (!t_ns) return set_error(ISIM_EINVAL, "null argument");
  isim::lp::Compiled c;
  if (const int rc = profile_compile(lp, c)) return rc;
  if (isim::lp::time_of(c, work_q24, *t_ns) != ISIM_OK)
    return set_error(ISIM_ERANGE, "load profile: work or time at or above 2^63");
  return ISIM_OK;
}

int isim_profile_arrivals_workspace_bytes(uint64_t n_traces, uint64_t *bytes) {
  if (!bytes) return set_error(ISIM_EINVAL, "null argument");
  if (n_traces > isim::lp::kMaxTraces) return set_error(ISIM_EINVAL, "n_traces above 2^32 per profile arrivals call");
  *bytes = profile_arrivals_ws_bytes(n_traces);
  return ISIM_OK;
}

int isim_profile_arrivals_device(const isim_handler *h, const isim_load_profile *lp, uint64_t trace_begin,
                                 uint64_t n_traces, uint64_t *d_arrivals, void *d_workspace,
                                 uint64_t workspace_bytes, void *hip_stream) {
  isim::lp::Compiled c;
  if (const int rc = profile_arrivals_check(h, lp, n_traces, d_arrivals, c)) return rc;
  if (n_traces == 0) return ISIM_OK;
  if (const int rc = arrivals_buffers_check(d_arrivals, d_workspace, workspace_bytes,
                                            profile_arrivals_ws_bytes(n_traces),
                                            "isim_profile_arrivals_workspace_bytes"))
    return rc;
  isim::lp::Seg *d_seg = (isim::lp::Seg *)((char *)d_workspace + profile_arrivals_blk_bytes(n_traces));
  const isim::lp::DeviceProfile dp{d_seg, (uint32_t)c.seg.size(), c.paced() ? 1u : 0u};
  if (isim::lp::upload(c, d_seg, hip_stream) != 0 ||
      isim::lp::arrivals_launch(h->params.seed, dp, trace_begin, n_traces, d_arrivals, (uint64_t *)d_workspace,
                                hip_stream) != 0)
    return set_error(ISIM_EHIP, "profile arrivals kernel launch failed");
  return ISIM_OK;
}

int isim_profile_arrivals(const isim_handler *h, int device, const isim_load_profile *lp, uint64_t trace_begin,
                          uint64_t n_traces, uint64_t *h_arrivals) {
  isim::lp::Compiled c;
  if (const int rc = profile_arrivals_check(h, lp, n_traces, h_arrivals, c)) return rc;
  if (n_traces == 0) return ISIM_OK;
  const uint64_t ws_bytes = profile_arrivals_ws_bytes(n_traces);
  isim::HostStage stage(device);
  void *d_a = stage.alloc(n_traces * 8), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_profile_arrivals_device(h, lp, trace_begin, n_traces, (uint64_t *)d_a, d_ws, ws_bytes,
                                                  stage.stream()))
    return rc;
  return stage.download(h_arrivals, d_a, n_traces * 8);
}

int isim_serve_des_profile_device(isim_handler *h, const isim_load_profile *lp, uint32_t des_flags,
                                  uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records,
                                  uint64_t *d_stats, uint64_t *d_des_table, void *d_workspace,
                                  uint64_t workspace_bytes, void *hip_stream) {
  isim::lp::Compiled c;
  DesLoad load{};
  if (const int rc = profile_des_check(h, lp, des_flags, n_traces, c, load)) return rc;
  if (const int rc = des_buffers_check(h, nullptr, n_traces, d_records, d_stats, d_des_table, d_workspace,
                                       workspace_bytes))
    return rc;
  if (n_traces == 0) return ISIM_OK;
  return serve_des_device(h, load, trace_begin, n_traces, d_records, d_stats, d_des_table, d_workspace,
                          workspace_bytes, hip_stream);
}

int isim_serve_des_profile(isim_handler *h, int device, const isim_load_profile *lp, uint64_t trace_begin,
                           uint64_t n_traces, isim_trace_rec *h_records, uint64_t *h_stats, uint64_t *h_des_table) {
  isim::lp::Compiled c;
  DesLoad load{};
  if (const int rc = profile_des_check(h, lp, 0, n_traces, c, load)) return rc;
  if (const int drc = des_ensure(h)) return drc;
  return serve_des_host(h, device, 0, n_traces, h_records, h_stats, h_des_table,
                        [&](uint32_t flags, isim_trace_rec *d_rec, uint64_t *d_stats, uint64_t *d_tab, void *d_ws,
                            uint64_t ws_bytes, hipStream_t s) {
                          return isim_serve_des_profile_device(h, lp, flags, trace_begin, n_traces, d_rec, d_stats,
                                                               d_tab, d_ws, ws_bytes, s);
                        });
}

void isim_debug_set_spin_limit(uint32_t polls) { isim::des_set_spin_limit(polls); }

uint32_t isim_debug_spin_limit(void) { return isim::des_spin_limit(); }

int isim_des_fold(const isim_handler *h, const uint64_t *des_table, uint64_t *svc_rows) {
  if (!h || !des_table || !svc_rows) return set_error(ISIM_EINVAL, "null argument");
  const isim::Program &p = h->prog;
  constexpr uint32_t W = ISIM_DES_ROW_WORDS;
  std::fill(svc_rows, svc_rows + (size_t)p.n_services * W, 0);
  for (size_t r = 0; r < p.row_svc.size(); ++r)
    std::copy(des_table + r * W, des_table + (r + 1) * W, svc_rows + (size_t)p.row_svc[r] * W);
  return ISIM_OK;
}

// ---- DES trace spans: the tap on an item-engine batch (des_items.hip)
int isim_des_wait_table_words(const isim_handler *h, uint64_t *words) {
  if (!h || !words) return tfail("null argument");
  *words = ((uint64_t)h->prog.n_services + 1) * ISIM_DW_ROW_WORDS;
  return ISIM_OK;
}

int isim_des_wait_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src) {
  if (!h || !dst || !src) return tfail("null argument");
  const uint64_t ns = (uint64_t)h->prog.n_services;
  for (uint64_t r = 0; r <= ns; ++r)
    for (uint32_t w = 0; w < ISIM_DW_ROW_WORDS; ++w) {
      uint64_t &d = dst[r * ISIM_DW_ROW_WORDS + w];
      const uint64_t v = src[r * ISIM_DW_ROW_WORDS + w];
      d = r < ns && w == ISIM_DW_MAX_WAIT ? std::max(d, v) : d + v;
    }
  return ISIM_OK;
}

int isim_serve_des_spans_device(isim_handler *h, const isim_des_params *dp, const isim_load_profile *lp,
                                uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records, uint64_t *d_stats,
                                uint64_t *d_des_table, void *d_workspace, uint64_t workspace_bytes,
                                const isim_des_tap *tap, void *hip_stream) {
  if (!h || !dp) return set_error(ISIM_EINVAL, "null argument");
  if (!tap)  // the existing path, whatever it checks
    return lp ? isim_serve_des_profile_device(h, lp, dp->flags, trace_begin, n_traces, d_records, d_stats,
                                              d_des_table, d_workspace, workspace_bytes, hip_stream)
              : isim_serve_des_device(h, dp, trace_begin, n_traces, d_records, d_stats, d_des_table, d_workspace,
                                      workspace_bytes, hip_stream);
  // the load's checks, the buffers' and the tap's, all before any HIP call
  isim::lp::Compiled c;
  DesLoad load{};
  if (const int rc = spans_load_check(h, dp, lp, n_traces, c, load)) return rc;
  if (const int rc = des_buffers_check(h, tap, n_traces, d_records, d_stats, d_des_table, d_workspace,
                                       workspace_bytes))
    return rc;
  if (n_traces == 0)  // no batch: an empty list (spans.hip's scan of nothing) with no match
    return isim::des_items_tap_none(*tap, hip_stream) ? set_error(ISIM_EHIP, "DES spans: kernel launch failed")
                                                      : ISIM_OK;
  load.tap = tap;
  return serve_des_device(h, load, trace_begin, n_traces, d_records, d_stats, d_des_table, d_workspace,
                          workspace_bytes, hip_stream);
}

int isim_serve_des_spans(isim_handler *h, int device, const isim_des_params *dp, const isim_load_profile *lp,
                         uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *h_records, uint64_t *h_stats,
                         uint64_t *h_des_table, const isim_des_tap *tap) {
  if (!h || !dp) return set_error(ISIM_EINVAL, "null argument");
  if (!tap)
    return lp ? isim_serve_des_profile(h, device, lp, trace_begin, n_traces, h_records, h_stats, h_des_table)
              : isim_serve_des(h, device, dp, trace_begin, n_traces, h_records, h_stats, h_des_table);
  if (const int rc = des_tap_check(h, tap, true, false)) return rc;
  {
    isim::lp::Compiled c;
    DesLoad load{};
    if (const int rc = spans_load_check(h, dp, lp, n_traces, c, load)) return rc;
  }
  uint64_t tab_words = 0;
  (void)isim_des_wait_table_words(h, &tab_words);
  const uint64_t n_ids = std::min<uint64_t>(tap->max_traces, n_traces);  // the list is no longer than the batch
  isim_des_tap dt = *tap;
  dt.max_traces = n_ids;
  isim::HostStage stage(device);  // the tap's buffers on `device`; the batch itself runs on serve_des_host's stream
  dt.d_ids = (uint64_t *)stage.alloc(n_ids * 8);
  dt.d_off = (uint64_t *)stage.alloc((n_ids + 1) * 8);
  dt.d_spans = (isim_des_span *)stage.alloc(tap->cap_spans * sizeof(isim_des_span));
  dt.d_info = (uint64_t *)stage.alloc(ISIM_DES_SPAN_INFO_WORDS * 8);
  dt.d_wait_table = tap->d_wait_table ? (uint64_t *)stage.upload(tap->d_wait_table, tab_words * 8) : nullptr;
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (hipStreamSynchronize(stage.stream()) != hipSuccess)
    return set_error(ISIM_EHIP, "DES spans: table upload failed");
  int rc = serve_des_host(h, device, dp->flags, n_traces, h_records, h_stats, h_des_table,
                          [&](uint32_t flags, isim_trace_rec *d_rec, uint64_t *d_stats, uint64_t *d_tab, void *d_ws,
                              uint64_t ws_bytes, hipStream_t s) {
                            isim_des_params p = *dp;
                            p.flags = flags;
                            return isim_serve_des_spans_device(h, &p, lp, trace_begin, n_traces, d_rec, d_stats,
                                                               d_tab, d_ws, ws_bytes, &dt, s);
                          },
                          true);
  if (rc != ISIM_OK) return rc;
  uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {};
  if ((rc = stage.download(info, dt.d_info, sizeof info)) != ISIM_OK) return rc;
  std::memcpy(tap->d_info, info, sizeof info);
  const uint64_t listed = info[ISIM_SPAN_N_IDS], written = info[ISIM_SPAN_WRITTEN];
  if ((rc = stage.download(tap->d_off, dt.d_off, (listed + 1) * 8)) != ISIM_OK) return rc;
  if ((rc = stage.download(tap->d_ids, dt.d_ids, listed * 8)) != ISIM_OK) return rc;
  if ((rc = stage.download(tap->d_spans, dt.d_spans, tap->d_off[written] * sizeof(isim_des_span))) != ISIM_OK) return rc;
  if (dt.d_wait_table) rc = stage.download(tap->d_wait_table, dt.d_wait_table, tab_words * 8);
  return rc;
}

}  // extern "C"
