// Critical path of DES trace spans on the device (des_critical_path.h,
// DESIGN.md §22).
//
// isim_des_critical_path_device: one kernel after a zeroing one.  One trace per
// wave, a wave per workgroup: the lanes stride over the trace's spans in every
// phase of dcp::Fold, __syncthreads() between two phases is a barrier of that
// one wave with workgroup-scope ordering for the links one lane writes and
// another reads, and no wave ever waits for another.  A wave claims list
// entries one at a time from a counter until the list is dry: a tail trace runs
// from one span to hundreds.  The number of traces is read on the device, from
// the d_info the tap wrote.  A trace is refused by a wave-wide vote before
// anything of it is written.  The header's words and a trace's critical wait
// are reduced over the wave; the service rows take plain u64 global atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "des_critical_path.h"
#include "hip_check.h"
#include "host_stage.h"

namespace isim {
namespace dcp {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kMaxBlocks = 8192;  // 8 waves on every SIMD of 256 CUs; a wave without an entry ends at once

struct CK {
  const uint64_t *off;   // [n_ids + 1]
  const uint64_t *info;  // ISIM_SPAN_WRITTEN: the traces to process
  isim_des_span *spans;
  uint64_t cap, n_ids;
  unsigned long long *table;
  uint64_t *trace_wait;  // nullptr or [n_ids]
  Link *links;
  const void *nodes;
  cp::ScriptView view;
};

// the table on the device: the header in registers, the service rows by global atomics
struct DevAcc {
  unsigned long long *table;
  uint64_t h[kHdrWords] = {};
  __device__ __forceinline__ void add(uint32_t row, uint32_t word, uint64_t v) {
    if (v) atomicAdd(table + (uint64_t)row * ISIM_DCP_ROW_WORDS + word, (unsigned long long)v);
  }
  __device__ __forceinline__ void hdr(uint32_t word, uint64_t v) { h[word] += v; }
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
  return v;
}

template <bool W>
__global__ void __launch_bounds__(kWave) k_des_critical_path(CK k, unsigned long long *work) {
  using KOf = std::conditional_t<W, cp::K16, cp::K8>;
  Fold<KOf> F;
  F.v = k.view;
  F.kof = KOf{(decltype(KOf::p))k.nodes};
  DevAcc acc{k.table};
  const uint64_t written = k.info[ISIM_SPAN_WRITTEN];
  const uint64_t n = written < k.n_ids ? written : k.n_ids;
  const uint64_t end = k.off[n];                   // no trace of the list reaches past the written spans
  const uint64_t cap = end < k.cap ? end : k.cap;  // ... nor past the buffer
  const uint32_t lane = threadIdx.x;
  while (true) {
    unsigned long long i = 0;
    if (lane == 0) i = atomicAdd(work, 1ull);
    i = __shfl(i, 0, 64);
    if (i >= n) break;
    bool ok = F.begin(k.off, i, cap, k.spans);  // the same for every lane, as every vote below
    if (ok) {  // phase 0, read-only
      F.w = k.links + F.base;
      bool good = true;
      for (uint32_t j = lane; j < F.m; j += kWave) good &= F.check(j);
      ok = __ballot(!good) == 0;
    }
    if (ok) {
      for (uint32_t j = lane; j < F.m; j += kWave) F.link(j);  // phase 1
      __syncthreads();
      bool good = true;
      for (uint32_t j = lane; j < F.m; j += kWave) good &= F.callers(j);  // phase 2
      __syncthreads();
      ok = __ballot(!good) == 0;  // spans and table untouched so far: a refused trace ends here
    }
    uint64_t wait = UINT64_MAX;
    if (ok) {  // phases 3 and 4
      wait = 0;
      for (uint32_t j = lane; j < F.m; j += kWave) wait += F.finish(j, acc);
      wait = wave_sum(wait);
    } else if (lane == 0) {
      acc.hdr(ISIM_DCP_H_REFUSED, 1);
    }
    if (lane == 0 && k.trace_wait) k.trace_wait[i] = wait;
  }
  // one add per wave and word for the header
#pragma unroll
  for (uint32_t w = 0; w < kHdrWords; ++w) {
    const uint64_t v = wave_sum(acc.h[w]);
    if (lane == 0 && v)
      atomicAdd(k.table + (uint64_t)k.view.n_services * ISIM_DCP_ROW_WORDS + w, (unsigned long long)v);
  }
}

// the entry counter of a call, by a kernel like every other step (a captured call is kernel nodes only)
__global__ void k_zero_counter(unsigned long long *work) {
  if (threadIdx.x == 0) *work = 0;
}

}  // namespace

int launch(const isim_handler *h, const uint64_t *d_off, isim_des_span *d_spans, uint64_t cap_spans,
           const uint64_t *d_info, uint64_t n_ids, uint64_t *d_table, uint64_t *d_trace_wait, void *d_workspace,
           void *stream) {
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
  k.trace_wait = d_trace_wait;
  k.links = (Link *)((char *)d_workspace + kWsHead);
  k.nodes = t.nodes;
  k.view = cp::ScriptView{t.cmd_off, t.cmds, (uint32_t)v.graph->services.size(), p.tree_positions()};
  unsigned long long *work = (unsigned long long *)d_workspace;
  const uint32_t blocks = (uint32_t)(n_ids < kMaxBlocks ? n_ids : kMaxBlocks);
  hipLaunchKernelGGL(k_zero_counter, dim3(1), dim3(64), 0, s, work);
  hipLaunchKernelGGL(p.tree_wide ? k_des_critical_path<true> : k_des_critical_path<false>, dim3(blocks), dim3(kWave), 0,
                     s, k, work);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace dcp
}  // namespace isim

namespace {
namespace dcp = isim::dcp;
namespace sp = isim::spans;
int dfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "DES critical path: " + msg); }
}  // namespace

extern "C" {

int isim_des_critical_path_device(const isim_handler *h, const uint64_t *d_off, isim_des_span *d_spans,
                                  uint64_t cap_spans, const uint64_t *d_info, uint64_t n_ids, uint64_t *d_table,
                                  uint64_t *d_trace_wait, void *d_workspace, uint64_t workspace_bytes,
                                  void *hip_stream) {
  if (const int rc = dcp::check_handler(h)) return rc;
  if (n_ids > sp::kMaxIds) return dfail("n_ids is above 2^32");
  if (cap_spans > sp::kMaxRecords) return dfail("cap_spans is above 2^40");
  if (!d_off || !d_info || !d_table) return dfail("null offsets, info or table");
  if (cap_spans && !d_spans) return dfail("null spans with cap_spans > 0");
  if ((((uintptr_t)d_off | (uintptr_t)d_info | (uintptr_t)d_table | (uintptr_t)d_trace_wait | (uintptr_t)d_workspace) &
       7u) || ((uintptr_t)d_spans & 15u))
    return dfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (n_ids && (!d_workspace || workspace_bytes < dcp::ws_bytes(cap_spans)))
    return dfail("the workspace is smaller than isim_des_critical_path_workspace_bytes()");
  return dcp::launch(h, d_off, d_spans, cap_spans, d_info, n_ids, d_table, d_trace_wait, d_workspace, hip_stream);
}

int isim_des_critical_path(int device, const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                           isim_des_span *h_spans, uint64_t *h_table, uint64_t *h_trace_wait) {
  if (const int rc = dcp::check_handler(h)) return rc;
  if (n_written > sp::kMaxIds) return dfail("n_written is above 2^32");
  if (!h_off || !h_table) return dfail("null offsets or table");
  const uint64_t cap = h_off[n_written];
  if (cap > sp::kMaxRecords) return dfail("the offsets end above 2^40 spans");
  if (cap && !h_spans) return dfail("null spans");
  const uint64_t words = (uint64_t)(sp::handler_view(h).graph->services.size() + 1) * ISIM_DCP_ROW_WORDS;
  const uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {cap, n_written, n_written, n_written, n_written};
  const uint64_t ws_bytes = dcp::ws_bytes(cap);
  isim::HostStage stage(device);
  void *d_off = stage.upload(h_off, (n_written + 1) * 8), *d_spans = stage.upload(h_spans, cap * sizeof(isim_des_span));
  void *d_info = stage.upload(info, sizeof info), *d_table = stage.upload(h_table, words * 8);
  void *d_ws = stage.alloc(n_written ? ws_bytes : 0);
  void *d_wait = stage.alloc(h_trace_wait ? n_written * 8 : 0);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_des_critical_path_device(h, (const uint64_t *)d_off, (isim_des_span *)d_spans, cap,
                                                   (const uint64_t *)d_info, n_written, (uint64_t *)d_table,
                                                   (uint64_t *)d_wait, d_ws, ws_bytes, stage.stream()))
    return rc;
  if (const int rc = stage.download(h_table, d_table, words * 8)) return rc;
  if (const int rc = stage.download(h_trace_wait, d_wait, d_wait ? n_written * 8 : 0)) return rc;
  return stage.download(h_spans, d_spans, cap * sizeof(isim_des_span));
}

}  // extern "C"
