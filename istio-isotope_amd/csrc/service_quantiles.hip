// Per-service percentiles on the device (service_quantiles.h):
// a segmented radix select over the three measures of the tapped spans.
//
// isim_service_quantiles_device: a fixed sequence of kernels on the caller's
// stream, no host synchronisation, no workgroup waits for another.
//   k_svq_clear    the ticket, the counts and the table's header
//   k_svq_count    spans per (service, code), wave-aggregated; folded / refused
//   k_svq_scan     one workgroup: segment offsets and cursors, and the long
//                  segments (more than kStage spans) numbered into slots, each
//                  with the first of its chunks of kChunk elements
//   k_svq_scatter  the three measures of a span to its segment, three arrays
//   k_svq_short    a workgroup claims a service by ticket; a short segment is
//                  staged in LDS and selected there, once per measure
//   k_svq_long_or, k_svq_long_setup, then per byte 7 .. 0 k_svq_long_hist and
//   k_svq_long_resolve: §13's launches, segmented.  grid.y is the measure; a
//   workgroup of _or and _hist takes chunks, each inside one long segment, and
//   flushes into that segment's bins; _setup and _resolve take one (segment,
//   measure) each.  All of them read the long segments' count on the device
//   and leave when there is nothing for them.
// The select itself, in LDS and as launches, is segmented_select.h's; the span
// load, the count, the scatter and the long segments' kernels are
// span_segments.h's, which service_window_quantiles.hip (§29) shares; the scan
// is service_scan.h's, which service_sketch.hip (§30) shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hip_check.h"
#include "host_stage.h"
#include "service_scan.h"
#include "span_segments.h"

namespace isim {
namespace svq {
namespace {

// The short segments.  A workgroup claims services through the ticket until none is left.  An empty service
// gets its zeros, a long one is the long kernels'.  Otherwise, per measure, the segment is staged in LDS and
// selected there (segmented_select.h); the ticket is s.sel.owner_word.
__global__ __launch_bounds__(kSelThreads) void k_svq_short(SelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[kClasses * kMaxQ * kBins];
  __shared__ unsigned long long s_stage[kStage];
  __shared__ rs::SelState s;
  const uint32_t t = threadIdx.x, ow = 1u + a.n_q;
  for (;;) {
    __syncthreads();  // the previous segment's state has been read
    if (t == 0) s.sel.owner_word = atomicAdd(&a.head->ticket, 1u);
    __syncthreads();
    const uint32_t svc = s.sel.owner_word;
    if (svc >= a.n_services) return;  // workgroup-uniform
    const uint32_t n200 = a.cnt[2 * svc], n500 = a.cnt[2 * svc + 1];
    const uint32_t n_seg = n200 + n500;
    unsigned long long *out = a.out + (uint64_t)svc * kMeasures * kClasses * ow;
    if (n_seg == 0) {
      for (uint32_t i = t; i < kMeasures * kClasses * ow; i += kSelThreads) out[i] = 0;
      continue;
    }
    const uint64_t off = a.off[2 * svc];
    // A long segment's cells are written by k_svq_long_setup (the counts) and k_svq_long_resolve at byte 0 (the
    // values), whatever its chunks find.  Counts that are not of these spans (the spans changed under the call)
    // can leave the long kernels nothing (n_long 0) or put a short segment past the arrays: zeros then, so
    // that every word of the table is written.
    const bool astray = n_seg > kStage ? a.head->n_long == 0 : off + n_seg > a.cap;
    if (astray)
      for (uint32_t i = t; i < kMeasures * kClasses * ow; i += kSelThreads) out[i] = 0;
    if (n_seg > kStage || astray) continue;
    for (uint32_t m = 0; m < kMeasures; ++m) {
      __syncthreads();  // the previous measure's state has been read
      rs::select_segment<true>(hist, s_stage, s, a.seg + m * a.cap + off, n_seg, n200, true, a.n_q, a.ppm,
                         out + (uint64_t)m * kClasses * ow);
    }
  }
}

}  // namespace

int launch(uint32_t n_services, const uint32_t *q_ppm, uint32_t n_q, const uint64_t *d_off,
           const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_out,
           void *d_workspace, void *stream) {
  const hipStream_t s = (hipStream_t)stream;
  const uint64_t words = table_words(n_services, n_q);
  if (cap_spans == 0) {  // no span: zeros
    hipLaunchKernelGGL(k_svq_clear, dim3(rs::grid_for(2 * words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
                       (uint32_t *)d_out, 2 * words, (uint32_t *)nullptr, (uint64_t)0);
    ISIM_HIPCHK(hipGetLastError());
    return ISIM_OK;
  }
  const Layout l = layout(n_services, cap_spans, n_q);
  char *ws = (char *)d_workspace;
  SK k{};
  k.off = d_off;
  k.info = d_info;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.n_services = n_services;
  k.cnt = (uint32_t *)(ws + l.cnt);
  k.cur = (uint32_t *)(ws + l.cur);
  k.seg = (unsigned long long *)(ws + l.seg);
  k.hdr = (unsigned long long *)d_out + (words - ISIM_SVQ_HEADER_WORDS);
  SelArgs a{};
  a.cnt = k.cnt;
  a.off = (const uint32_t *)(ws + l.off);
  a.seg = k.seg;
  a.cap = cap_spans;
  a.head = (Head *)ws;
  a.slots = (Slot *)(ws + l.slots);
  a.bins = (uint32_t *)(ws + l.bins);
  a.out = (unsigned long long *)d_out;
  a.n_services = n_services;
  a.n_q = n_q;
  a.n_slots = (uint32_t)l.n_slots;
  a.ppm = rs::ppm_of(q_ppm, n_q);

  // the head and the counts, contiguous from the workspace's start, and the table's header (every clear is a kernel)
  const uint64_t clear_words = l.cnt / 4 + l.counters;
  hipLaunchKernelGGL(k_svq_clear, dim3(rs::grid_for(clear_words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
                     (uint32_t *)ws, clear_words, (uint32_t *)k.hdr, (uint64_t)2 * ISIM_SVQ_HEADER_WORDS);
  const uint32_t grid = rs::grid_for(cap_spans, kThreads * kUnroll, kMaxGrid);
  hipLaunchKernelGGL(k_svq_count<ServiceKey>, dim3(grid), dim3(kThreads), 0, s, k, ServiceKey{});
  hipLaunchKernelGGL(k_svq_scan<kStage>, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)k.cnt, (uint32_t *)(ws + l.off),
                     k.cur, n_services, a.slots, a.n_slots, a.head);
  hipLaunchKernelGGL(k_svq_scatter<ServiceKey>, dim3(grid), dim3(kThreads), 0, s, k, ServiceKey{});
  hipLaunchKernelGGL(k_svq_short, dim3(std::min(n_services, kSelMaxGrid)), dim3(kSelThreads), 0, s, a);
  launch_long(a, cap_spans, s);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace svq
}  // namespace isim

namespace {
namespace svq = isim::svq;
int qfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service quantiles: " + msg); }

}  // namespace

extern "C" {

int isim_service_quantiles_device(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q, const uint64_t *d_off,
                                  const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
                                  uint64_t *d_out, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  uint64_t ns = 0;
  if (const int rc = svq::check(h, q_ppm, n_q, cap_spans, ns)) return rc;
  if (!d_off || !d_info || !d_out) return qfail("null offsets, info or table");
  if (cap_spans && !d_spans) return qfail("null spans with cap_spans > 0");
  if ((((uintptr_t)d_off | (uintptr_t)d_info | (uintptr_t)d_out | (uintptr_t)d_workspace) & 7u) ||
      ((uintptr_t)d_spans & 15u))
    return qfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (cap_spans && (!d_workspace || workspace_bytes < svq::layout(ns, cap_spans, n_q).total))
    return qfail("the workspace is smaller than isim_service_quantiles_workspace_bytes()");
  return svq::launch((uint32_t)ns, q_ppm, n_q, d_off, d_spans, cap_spans, d_info, d_out, d_workspace, hip_stream);
}

int isim_service_quantiles(int device, const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q,
                           const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_out) {
  uint64_t ns = 0;
  if (const int rc = svq::check(h, q_ppm, n_q, n_spans, ns)) return rc;
  if (!h_out) return qfail("null table");
  if (n_spans && !h_spans) return qfail("null spans");
  // the tap's offsets and info of one list entry that holds every span
  const uint64_t off[2] = {0, n_spans};
  const uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {n_spans, 1, 1, 1, 1};
  const uint64_t bytes = svq::table_words(ns, n_q) * 8, ws_bytes = n_spans ? svq::layout(ns, n_spans, n_q).total : 0;
  isim::HostStage stage(device);
  void *d_out = stage.alloc(bytes);
  void *d_off = stage.upload(off, sizeof off), *d_info = stage.upload(info, sizeof info);
  void *d_spans = stage.upload(h_spans, n_spans * sizeof(isim_des_span)), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_service_quantiles_device(h, q_ppm, n_q, (const uint64_t *)d_off,
                                                   (const isim_des_span *)d_spans, n_spans, (const uint64_t *)d_info,
                                                   (uint64_t *)d_out, d_ws, ws_bytes, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, bytes);
}

}  // extern "C"
