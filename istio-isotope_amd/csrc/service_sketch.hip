// The per-service latency sketch on the device (service_sketch.h, DESIGN.md
// §30): one §16 table per (service, measure), filled from the tapped spans and
// accumulated into the caller's table.
//
// isim_service_sketch_device: a fixed sequence of kernels on the caller's
// stream, no host synchronisation, no workgroup waits for another.
//   k_svq_clear    the head and the counts (not the table: it is added into)
//   k_svq_count    spans per (service, code), wave-aggregated; folded / refused
//                  added to the table's header
//   k_svq_scan     one workgroup: segment offsets and cursors, and the long
//                  segments (more than kShort spans) numbered into slots, each
//                  with the first of its chunks of kChunk elements
//   k_svq_scatter  the three measures of a span to its segment, three arrays
//   k_svs_fill     the work list is the scan's: first the (chunk, measure)
//                  pairs of the long segments, one per workgroup and turn, into
//                  a u32 [2][bins] block in LDS that is flushed with u64 atomics
//                  where it is nonzero; then the short segments, whole segments
//                  per wave, each element's word added to the table through the
//                  peel (wave_peel.h), so lanes on one word add once.
// Grouping first keeps the entry service, which has a span of every trace, off
// one global word per span: its chunks meet in LDS.  The count, the scatter and
// the slots are span_segments.h's, the scan is service_scan.h's (§28's own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hip_check.h"
#include "host_stage.h"
#include "service_scan.h"
#include "service_sketch.h"
#include "span_segments.h"

namespace isim {
namespace svs {
namespace {

using svq::Head;
using svq::kChunk;
using svq::kNone;
using svq::Slot;

constexpr uint32_t kFillThreads = 512;
constexpr uint32_t kFillWaves = kFillThreads / 64;
constexpr uint32_t kLdsWords = 2 * ISIM_SK_BINS(7);  // 59,392 B of u32: two workgroups share a CU, as k_sketch's
constexpr uint32_t kFillMaxGrid = 512;
static_assert(kChunk <= 0xFFFFFFFFull / 2, "a chunk's counts fit the u32 words in LDS");

struct FillArgs {
  const uint32_t *cnt;            // [services][2]
  const uint32_t *off;            // [services][2]
  const unsigned long long *seg;  // [kMeasures][cap]
  uint64_t cap;
  const Head *head;
  const Slot *slots;
  unsigned long long *out;  // the table
  uint32_t n_services, sub_bits, bins;
};

// word[key] += 1 per lane (kNone: no update), in LDS or in the table: the peel of wave_peel.h
template <typename Word, typename Inc>
__device__ __forceinline__ void wave_inc(Word *words, uint32_t key, uint32_t lane) {
  dev::wave_peel<dev::kPeelAll>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        if ((int)lane == lead) atomicAdd(&words[k0], (Inc)__popcll(m));
      },
      [&](uint32_t k) { atomicAdd(&words[k], (Inc)1); });
}

__global__ __launch_bounds__(kFillThreads) void k_svs_fill(FillArgs a) {
  __shared__ uint32_t s_tab[kLdsWords];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t bins = a.bins, block = 2u * bins;  // block <= kLdsWords for sub_bits <= 7

  // ---- the long tier: (chunk, measure) pairs, workgroup-uniform
  const uint32_t n_long = a.head->n_long, n_chunks = a.head->n_chunks;
  const uint64_t n_items = (uint64_t)n_chunks * kMeasures;
  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const uint32_t chunk = (uint32_t)(item / kMeasures), m = (uint32_t)(item % kMeasures);
    const Slot &x = a.slots[svq::find_slot(a.slots, n_long, chunk)];
    uint32_t begin, end;
    if (!svq::chunk_range(x, chunk, a.cap, begin, end)) continue;
    for (uint32_t i = t; i < block; i += kFillThreads) s_tab[i] = 0;
    __syncthreads();
    const unsigned long long *seg = a.seg + m * a.cap + x.off;
    const uint32_t n200 = x.n200;
    // a wave takes 64 consecutive elements per step; the loop bound is wave-uniform
    for (uint32_t base = begin + wave * 64u; base < end; base += kFillThreads) {
      const uint32_t i = base + lane;
      const uint32_t key = i < end ? (i >= n200 ? bins : 0u) + sk::bucket(a.sub_bits, seg[i]) : kNone;
      wave_inc<uint32_t, uint32_t>(s_tab, key, lane);
    }
    __syncthreads();
    unsigned long long *out = a.out + ((uint64_t)x.svc * kMeasures + m) * block;
    for (uint32_t i = t; i < block; i += kFillThreads) {
      const uint32_t v = s_tab[i];
      if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
    __syncthreads();  // the flush has read the block before the next turn clears it
  }

  // ---- the short tier: whole segments per wave
  const uint32_t n_waves = gridDim.x * kFillWaves;
  for (uint32_t svc = blockIdx.x * kFillWaves + wave; svc < a.n_services; svc += n_waves) {  // wave-uniform
    const uint32_t n200 = a.cnt[2 * svc], n_seg = n200 + a.cnt[2 * svc + 1];
    const uint64_t off = a.off[2 * svc];
    // counts that are not of these spans (the spans changed under the call) can put a segment past the arrays
    if (n_seg == 0 || n_seg > kShort || off + n_seg > a.cap) continue;
    for (uint32_t m = 0; m < kMeasures; ++m) {
      const unsigned long long *seg = a.seg + m * a.cap + off;
      const uint32_t first = (svc * kMeasures + m) * block;  // below 2^32: ISIM_SVS_MAX_WORDS
      for (uint32_t base = 0; base < n_seg; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t key = i < n_seg ? first + (i >= n200 ? bins : 0u) + sk::bucket(a.sub_bits, seg[i]) : kNone;
        wave_inc<unsigned long long, unsigned long long>(a.out, key, lane);
      }
    }
  }
}

}  // namespace

int launch(uint32_t n_services, uint32_t sub_bits, const uint64_t *d_off, const isim_des_span *d_spans,
           uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_table, void *d_workspace, void *stream) {
  if (cap_spans == 0) return ISIM_OK;  // no span: nothing is touched
  const hipStream_t s = (hipStream_t)stream;
  const Layout l = layout(n_services, cap_spans);
  char *ws = (char *)d_workspace;
  svq::SK k{};
  k.off = d_off;
  k.info = d_info;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.n_services = n_services;
  k.cnt = (uint32_t *)(ws + l.cnt);
  k.cur = (uint32_t *)(ws + l.cur);
  k.seg = (unsigned long long *)(ws + l.seg);
  k.hdr = (unsigned long long *)d_table + (table_words(n_services, sub_bits) - ISIM_SVQ_HEADER_WORDS);
  FillArgs a{};
  a.cnt = k.cnt;
  a.off = (const uint32_t *)(ws + l.off);
  a.seg = k.seg;
  a.cap = cap_spans;
  a.head = (const Head *)ws;
  a.slots = (const Slot *)(ws + l.slots);
  a.out = (unsigned long long *)d_table;
  a.n_services = n_services;
  a.sub_bits = sub_bits;
  a.bins = sk::bins(sub_bits);

  // the head and the counts, contiguous from the workspace's start (every clear is a kernel)
  const uint64_t clear_words = l.cnt / 4 + l.counters;
  hipLaunchKernelGGL(svq::k_svq_clear, dim3(rs::grid_for(clear_words, svq::kThreads * 4, svq::kMaxGrid)),
                     dim3(svq::kThreads), 0, s, (uint32_t *)ws, clear_words, (uint32_t *)nullptr, (uint64_t)0);
  const uint32_t grid = rs::grid_for(cap_spans, svq::kThreads * svq::kUnroll, svq::kMaxGrid);
  hipLaunchKernelGGL(svq::k_svq_count<svq::ServiceKey>, dim3(grid), dim3(svq::kThreads), 0, s, k, svq::ServiceKey{});
  hipLaunchKernelGGL(svq::k_svq_scan<kShort>, dim3(1), dim3(svq::kScanThreads), 0, s, (const uint32_t *)k.cnt,
                     (uint32_t *)(ws + l.off), k.cur, n_services, (Slot *)(ws + l.slots), (uint32_t)l.n_slots,
                     (Head *)ws);
  hipLaunchKernelGGL(svq::k_svq_scatter<svq::ServiceKey>, dim3(grid), dim3(svq::kThreads), 0, s, k, svq::ServiceKey{});
  // as many workgroups as the most (chunk, measure) pairs cap_spans spans can form, or as the services ask waves for
  const uint64_t max_items = (cap_spans / kChunk + l.n_slots) * kMeasures;
  const uint64_t want = std::max<uint64_t>(max_items, (n_services + kFillWaves - 1) / kFillWaves);
  hipLaunchKernelGGL(k_svs_fill, dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), kFillMaxGrid)),
                     dim3(kFillThreads), 0, s, a);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace svs
}  // namespace isim

namespace {
namespace svs = isim::svs;
int kfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service sketch: " + msg); }

}  // namespace

extern "C" {

int isim_service_sketch_device(const isim_handler *h, uint32_t sub_bits, const uint64_t *d_off,
                               const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
                               uint64_t *d_table, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, cap_spans, ns)) return rc;
  if (!d_off || !d_info || !d_table) return kfail("null offsets, info or table");
  if (cap_spans && !d_spans) return kfail("null spans with cap_spans > 0");
  if ((((uintptr_t)d_off | (uintptr_t)d_info | (uintptr_t)d_table | (uintptr_t)d_workspace) & 7u) ||
      ((uintptr_t)d_spans & 15u))
    return kfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (cap_spans && (!d_workspace || workspace_bytes < svs::layout(ns, cap_spans).total))
    return kfail("the workspace is smaller than isim_service_sketch_workspace_bytes()");
  return svs::launch((uint32_t)ns, sub_bits, d_off, d_spans, cap_spans, d_info, d_table, d_workspace, hip_stream);
}

int isim_service_sketch(int device, const isim_handler *h, uint32_t sub_bits, const isim_des_span *h_spans,
                        uint64_t n_spans, uint64_t *h_table) {
  uint64_t ns = 0;
  if (const int rc = svs::check_sizes(h, sub_bits, n_spans, ns)) return rc;
  if (!h_table) return kfail("null table");
  if (n_spans && !h_spans) return kfail("null spans");
  if (n_spans == 0) return ISIM_OK;
  // the tap's offsets and info of one list entry that holds every span
  const uint64_t off[2] = {0, n_spans};
  const uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {n_spans, 1, 1, 1, 1};
  const uint64_t bytes = svs::table_words(ns, sub_bits) * 8, ws_bytes = svs::layout(ns, n_spans).total;
  isim::HostStage stage(device);
  void *d_table = stage.upload(h_table, bytes);  // h_table is accumulated into like d_table: it goes up first
  void *d_off = stage.upload(off, sizeof off), *d_info = stage.upload(info, sizeof info);
  void *d_spans = stage.upload(h_spans, n_spans * sizeof(isim_des_span)), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_service_sketch_device(h, sub_bits, (const uint64_t *)d_off, (const isim_des_span *)d_spans,
                                                n_spans, (const uint64_t *)d_info, (uint64_t *)d_table, d_ws, ws_bytes,
                                                stage.stream()))
    return rc;
  return stage.download(h_table, d_table, bytes);
}

}  // extern "C"
