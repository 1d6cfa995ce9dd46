// Critical path on the device (critical_path.h).
//
// isim_critical_path_device: one kernel after a zeroing one.  One trace per
// lane; a lane runs cp::Fold one step (one span of the check, the links or the
// forward pass) per turn, and a lane whose trace is finished takes the next
// entry of its wave's batch of 64 LIST ENTRIES, the wave claiming batches from a
// counter as it runs dry (spans.hip k_span_walk's refill): tail traces run from
// one span to hundreds.  The number of traces is read on the device, from the
// d_info the span call wrote.  The rows of the entry service and the header take
// an add from every trace: a lane keeps them in registers and the wave reduces
// them once, before its global atomics; every other row takes plain u64 global
// atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "critical_path.h"
#include "hip_check.h"
#include "host_stage.h"

namespace isim {
namespace cp {
namespace {

constexpr uint32_t kHdrWords = 5;

struct CK {
  const uint64_t *off;   // [n_ids + 1]
  const uint64_t *info;  // ISIM_SPAN_WRITTEN: the traces to process
  isim_span *spans;
  uint64_t cap, n_ids;
  unsigned long long *table;
  uint32_t *links;
  const void *nodes;
  ScriptView view;
  uint32_t entry;
};

// the table on the device: the entry service's row and the header in registers, the rest by global atomics
struct DevAcc {
  unsigned long long *table;
  uint32_t entry, n_services;
  uint64_t e[ISIM_CP_ROW_WORDS] = {}, h[kHdrWords] = {};
  __device__ __forceinline__ void add(uint32_t row, uint32_t word, uint64_t v) {
    if (row == entry) e[word] += v;
    else atomicAdd(table + (uint64_t)row * ISIM_CP_ROW_WORDS + word, (unsigned long long)v);
  }
  __device__ __forceinline__ void hdr(uint32_t word, uint64_t v) { h[word] += v; }
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
  return v;
}

template <bool W>
__global__ void __launch_bounds__(spans::kT) k_critical_path(CK k, unsigned long long *work) {
  using KOf = std::conditional_t<W, K16, K8>;
  Fold<KOf> F;
  F.v = k.view;
  F.kof = KOf{(decltype(KOf::p))k.nodes};
  DevAcc acc{k.table, k.entry, k.view.n_services};
  const uint64_t written = k.info[ISIM_SPAN_WRITTEN];
  const uint64_t n = written < k.n_ids ? written : k.n_ids;
  const uint64_t end = k.off[n];                       // no trace of the list reaches past the written spans
  const uint64_t cap = end < k.cap ? end : k.cap;      // ... nor past the buffer
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint64_t nxt = 0, lim = 0;
  bool dry = false, active = false;
  while (true) {
    unsigned long long idle = __ballot(!active);
    while (idle && !dry) {
      if (nxt >= lim) {
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(work, 1ull);
        b = __shfl(b, 0, 64);
        if (b * 64 >= n) {
          dry = true;
          break;
        }
        nxt = b * 64;
        lim = nxt + 64 < n ? nxt + 64 : n;
      }
      const uint32_t rank = (uint32_t)__popcll(idle & lt);
      const bool take = ((idle >> lane) & 1ull) && rank < lim - nxt;
      if (take && F.begin(k.off, nxt + rank, cap, k.spans, acc)) {
        F.link = k.links + 2 * F.base;
        active = true;
      }
      const unsigned long long took = __ballot(take);
      nxt += (uint64_t)__popcll(took);
      idle &= ~__ballot(active);
    }
    if (!__ballot(active)) break;
    if (active) active = F.step(acc);
  }
  // one add per wave and word for the entry's row and the header
#pragma unroll
  for (uint32_t w = 0; w < ISIM_CP_ROW_WORDS; ++w) {
    const uint64_t v = wave_sum(acc.e[w]);
    if (lane == 0 && v) atomicAdd(k.table + (uint64_t)k.entry * ISIM_CP_ROW_WORDS + w, (unsigned long long)v);
  }
#pragma unroll
  for (uint32_t w = 0; w < kHdrWords; ++w) {
    const uint64_t v = wave_sum(acc.h[w]);
    if (lane == 0 && v) atomicAdd(k.table + (uint64_t)k.view.n_services * ISIM_CP_ROW_WORDS + w, (unsigned long long)v);
  }
}

// the batch counter of a call, by a kernel like every other step (a captured call is kernel nodes only)
__global__ void k_zero_counter(unsigned long long *work) {
  if (threadIdx.x == 0) *work = 0;
}

}  // namespace

int launch(const isim_handler *h, const uint64_t *d_off, isim_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
           uint64_t n_ids, uint64_t *d_table, void *d_workspace, void *stream) {
  if (n_ids == 0) return ISIM_OK;  // no trace, no add
  hipStream_t s = (hipStream_t)stream;
  const spans::HandlerView v = spans::handler_view(h);
  const Program &p = *v.prog;
  spans::DevTables t;
  if (const int rc = spans::device_tables(v, t)) return rc;
  CK k{};
  k.off = d_off;
  k.info = d_info;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.n_ids = n_ids;
  k.table = (unsigned long long *)d_table;
  k.links = (uint32_t *)((char *)d_workspace + kWsHead);
  k.nodes = t.nodes;
  k.view = ScriptView{t.cmd_off, t.cmds, (uint32_t)v.graph->services.size(), p.tree_positions()};
  k.entry = (uint32_t)p.entry;
  unsigned long long *work = (unsigned long long *)d_workspace;
  hipLaunchKernelGGL(k_zero_counter, dim3(1), dim3(64), 0, s, work);
  hipLaunchKernelGGL(p.tree_wide ? k_critical_path<true> : k_critical_path<false>, dim3(spans::walk_blocks(n_ids)),
                     dim3(spans::kT), 0, s, k, work);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace cp
}  // namespace isim

namespace {
namespace cp = isim::cp;
namespace sp = isim::spans;
int cfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "critical path: " + msg); }
}  // namespace

extern "C" {

int isim_critical_path_device(const isim_handler *h, const uint64_t *d_off, isim_span *d_spans, uint64_t cap_spans,
                              const uint64_t *d_info, uint64_t n_ids, uint64_t *d_table, void *d_workspace,
                              uint64_t workspace_bytes, void *hip_stream) {
  if (const int rc = cp::check_handler(h)) return rc;
  if (n_ids > sp::kMaxIds) return cfail("n_ids is above 2^32");
  if (cap_spans > sp::kMaxRecords) return cfail("cap_spans is above 2^40");
  if (!d_off || !d_info || !d_table) return cfail("null offsets, info or table");
  if (cap_spans && !d_spans) return cfail("null spans with cap_spans > 0");
  if (((uintptr_t)d_off | (uintptr_t)d_spans | (uintptr_t)d_info | (uintptr_t)d_table | (uintptr_t)d_workspace) & 7u)
    return cfail("the buffers must be 8-byte aligned");
  if (n_ids && (!d_workspace || workspace_bytes < cp::ws_bytes(cap_spans)))
    return cfail("the workspace is smaller than isim_critical_path_workspace_bytes()");
  return cp::launch(h, d_off, d_spans, cap_spans, d_info, n_ids, d_table, d_workspace, hip_stream);
}

int isim_critical_path(int device, const isim_handler *h, const uint64_t *h_off, uint64_t n_written, isim_span *h_spans,
                       uint64_t *h_table) {
  if (const int rc = cp::check_handler(h)) return rc;
  if (n_written > sp::kMaxIds) return cfail("n_written is above 2^32");
  if (!h_off || !h_table) return cfail("null offsets or table");
  const uint64_t cap = h_off[n_written];
  if (cap > sp::kMaxRecords) return cfail("the offsets end above 2^40 spans");
  if (cap && !h_spans) return cfail("null spans");
  const uint64_t words = (uint64_t)(sp::handler_view(h).graph->services.size() + 1) * ISIM_CP_ROW_WORDS;
  const uint64_t info[ISIM_SPAN_INFO_WORDS] = {cap, n_written, n_written, n_written};
  const uint64_t ws_bytes = cp::ws_bytes(cap);
  isim::HostStage stage(device);
  void *d_off = stage.upload(h_off, (n_written + 1) * 8), *d_spans = stage.upload(h_spans, cap * sizeof(isim_span));
  void *d_info = stage.upload(info, sizeof info), *d_table = stage.upload(h_table, words * 8);
  void *d_ws = stage.alloc(n_written ? ws_bytes : 0);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_critical_path_device(h, (const uint64_t *)d_off, (isim_span *)d_spans, cap,
                                               (const uint64_t *)d_info, n_written, (uint64_t *)d_table, d_ws, ws_bytes,
                                               stage.stream()))
    return rc;
  if (const int rc = stage.download(h_table, d_table, words * 8)) return rc;
  return stage.download(h_spans, d_spans, cap * sizeof(isim_span));
}

}  // extern "C"
