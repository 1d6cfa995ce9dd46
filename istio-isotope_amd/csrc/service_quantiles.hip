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
// The select itself, in LDS and as launches, is segmented_select.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hip_check.h"
#include "host_stage.h"
#include "segmented_select.h"
#include "service_quantiles.h"

namespace isim {
namespace svq {
namespace {

namespace rs = isim::rs;
using rs::kBins;
using rs::kHistThreads;
using rs::kMaxQ;
using rs::kResolveThreads;
using rs::kSelThreads;
using rs::kUnroll;
static_assert(rs::kStage == kStage, "the stage is segmented_select.h's");
static_assert(rs::kClasses == kClasses, "the classes are radix_select.h's");

constexpr uint32_t kThreads = 256;   // clear, count, scatter, or, setup
constexpr uint32_t kMaxGrid = 2048;  // count and scatter stride past it
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kSelMaxGrid = 512;  // two workgroups per CU by LDS: 48 KB of bins + 28 KB of stage + 1.2 KB of state
constexpr uint32_t kHistWaves = kHistThreads / 64;
constexpr uint32_t kHistMaxGrid = 1024;  // per measure
static_assert(kChunk % (kHistThreads * kUnroll) == 0 && kChunk % kThreads == 0, "a chunk is whole steps of a workgroup");

struct Head {
  uint32_t ticket;    // k_svq_short: the next service
  uint32_t n_long;    // long segments
  uint32_t n_chunks;  // their chunks
};
static_assert(sizeof(Head) <= kHeadBytes, "the head fits its bytes");

// a long segment; the select's top byte of measure m is st[m].owner_word (as int; -1: every value is 0)
struct Slot {
  uint32_t svc, chunk0, n200, n500;
  uint64_t off;  // the segment's first element
  unsigned long long any[kMeasures];
  rs::State<uint32_t> st[kMeasures];
  unsigned char pad[kSlotBytes - 48 - kMeasures * sizeof(rs::State<uint32_t>)];
};
static_assert(sizeof(Slot) == kSlotBytes, "isim_service_quantiles_workspace_bytes is pinned");

struct SK {
  const uint64_t *off, *info;
  const isim_des_span *spans;
  uint64_t cap;
  uint32_t n_services;
  uint32_t *cnt;            // count: [n_services][2], added to
  uint32_t *cur;            // scatter: [n_services][2] cursors
  unsigned long long *seg;  // scatter: [kMeasures][cap]
  unsigned long long *hdr;  // the table's header
};

__device__ __forceinline__ uint64_t span_count(const SK &k) {
  const uint64_t end = k.off[k.info[ISIM_SPAN_WRITTEN]];
  return end < k.cap ? end : k.cap;
}

__global__ __launch_bounds__(kThreads) void k_svq_clear(uint32_t *a, uint64_t na, uint32_t *b, uint64_t nb) {
  rs::clear_words<kThreads>(a, na);
  rs::clear_words<kThreads>(b, nb);
}

// a wave's kUnroll * 64 consecutive spans from `base`: per span the key 2 * service + code (kNone past n or
// refused) and the three measures
__device__ __forceinline__ void load_keys(const SK &k, uint64_t n, uint64_t base, uint32_t lane, uint32_t (&key)[kUnroll],
                                          uint64_t (&val)[kUnroll][kMeasures], uint32_t &refused) {
  uint64_t a[kUnroll], s[kUnroll], f[kUnroll];
  uint32_t svc[kUnroll], st[kUnroll];
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    const uint64_t i = base + u * 64 + lane;
    a[u] = s[u] = f[u] = 0;
    svc[u] = kNone;
    st[u] = 0;
    if (i < n) {
      const isim_des_span &x = k.spans[i];
      a[u] = x.arrival_ns;
      s[u] = x.start_ns;
      f[u] = x.finish_ns;
      svc[u] = x.service;
      st[u] = x.status;
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    const bool live = base + u * 64 + lane < n;
    const bool bad = span_refused(k.n_services, a[u], s[u], f[u], svc[u]);
    refused += live && bad ? 1u : 0u;
    key[u] = live && !bad ? svc[u] * 2u + (st[u] & 1u) : kNone;
#pragma unroll
    for (uint32_t m = 0; m < kMeasures; ++m) val[u][m] = measure(m, a[u], s[u], f[u]);
  }
}

// Pass 1: spans per (service, code), and the header.
__global__ __launch_bounds__(kThreads) void k_svq_count(SK k) {
  const uint64_t n = span_count(k);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  uint32_t refused = 0, folded = 0;
  // a wave takes 64 * kUnroll consecutive spans per step; the loop bound is wave-uniform
  for (uint64_t base = wave * (64 * kUnroll); base < n; base += step) {
    uint32_t key[kUnroll];
    uint64_t val[kUnroll][kMeasures];
    load_keys(k, n, base, lane, key, val, refused);
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      folded += key[u] != kNone ? 1u : 0u;
      rs::wave_add(k.cnt, (int)key[u], lane);  // kNone: no bin
    }
  }
  const uint64_t fo = dev::wave_reduce<dev::OpAdd>(folded), re = dev::wave_reduce<dev::OpAdd>(refused);
  if (lane == 0) {
    if (fo) atomicAdd(k.hdr + ISIM_SVQ_H_FOLDED, (unsigned long long)fo);
    if (re) atomicAdd(k.hdr + ISIM_SVQ_H_REFUSED, (unsigned long long)re);
  }
}

// One workgroup, a service per thread and tile: the exclusive scan of the counts into the segment offsets and
// the scatter cursors; the long segments get a slot each, in service order, and the first of their chunks.
// The counts are of at most cap spans, so no more than n_slots segments are long.
__global__ __launch_bounds__(kScanThreads) void k_svq_scan(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off,
                                                          uint32_t *__restrict__ cur, uint32_t n_services, Slot *slots,
                                                          uint32_t n_slots, Head *head) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t c_elem = 0, c_long = 0, c_chunk = 0;
  for (uint32_t tile = 0; tile < n_services; tile += kScanThreads) {
    const uint32_t s = tile + t;
    const bool live = s < n_services;
    const uint32_t n200 = live ? cnt[2 * s] : 0u, n500 = live ? cnt[2 * s + 1] : 0u;
    const uint32_t n = n200 + n500;
    const bool is_long = n > kStage;
    uint32_t t_elem, t_long, t_chunk;
    const uint32_t e = c_elem + rs::block_scan<kScanThreads>(n, s_wave, lane, wave, t_elem);
    const uint32_t l = c_long + rs::block_scan<kScanThreads>(is_long ? 1u : 0u, s_wave, lane, wave, t_long);
    const uint32_t c =
        c_chunk + rs::block_scan<kScanThreads>(is_long ? (n - 1) / kChunk + 1 : 0u, s_wave, lane, wave, t_chunk);
    if (live) {
      off[2 * s] = cur[2 * s] = e;
      off[2 * s + 1] = cur[2 * s + 1] = e + n200;
      if (is_long && l < n_slots) {
        Slot &x = slots[l];
        x.svc = s;
        x.chunk0 = c;
        x.n200 = n200;
        x.n500 = n500;
        x.off = e;
        for (uint32_t m = 0; m < kMeasures; ++m) x.any[m] = 0;
      }
    }
    c_elem += t_elem;
    c_long += t_long;
    c_chunk += t_chunk;
  }
  if (t == 0) {
    const bool fits = c_long <= n_slots;  // always, for counts of at most cap spans
    head->n_long = fits ? c_long : 0u;
    head->n_chunks = fits ? c_chunk : 0u;
  }
}

// Pass 2: the three measures of each span to its service's segment (its 200s, then its 500s).  A position
// past cap cannot come from counts and cursors of the same spans; were the spans changed under the call,
// nothing is written outside the segment arrays.
__global__ __launch_bounds__(kThreads) void k_svq_scatter(SK k) {
  const uint64_t n = span_count(k);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  uint32_t refused = 0;
  for (uint64_t base = wave * (64 * kUnroll); base < n; base += step) {
    uint32_t key[kUnroll];
    uint64_t val[kUnroll][kMeasures];
    load_keys(k, n, base, lane, key, val, refused);
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t pos = dev::wave_claim(k.cur, key[u], kNone, lane);
      if (key[u] != kNone && pos < k.cap) {
#pragma unroll
        for (uint32_t m = 0; m < kMeasures; ++m) k.seg[m * k.cap + pos] = val[u][m];
      }
    }
  }
}

struct SelArgs {
  const uint32_t *cnt;            // [n_services][2]
  const uint32_t *off;            // [n_services][2]
  const unsigned long long *seg;  // [kMeasures][cap]
  uint64_t cap;
  Head *head;
  Slot *slots;
  uint32_t *bins;           // [n_slots][kMeasures][kClasses][n_q][kBins]
  unsigned long long *out;  // [n_services][kMeasures][kClasses][1 + n_q]
  uint32_t n_services, n_q, n_slots;
  rs::Ppm ppm;
};

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

// the long segment that holds chunk (< n_chunks, so n_long >= 1): the last slot whose first chunk is at or before it
__device__ __forceinline__ uint32_t find_slot(const Slot *slots, uint32_t n_long, uint32_t chunk) {
  uint32_t lo = 0, hi = n_long;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (slots[mid].chunk0 <= chunk) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the elements [begin, end) of the slot's segment that are the chunk's; false: none (counts not of these spans)
__device__ __forceinline__ bool chunk_range(const Slot &x, uint32_t chunk, uint64_t cap, uint32_t &begin, uint32_t &end) {
  const uint32_t n_seg = x.n200 + x.n500;
  const uint64_t b = (uint64_t)(chunk - x.chunk0) * kChunk;
  if (b >= n_seg || x.off + n_seg > cap) return false;
  begin = (uint32_t)b;
  end = n_seg - begin > kChunk ? begin + kChunk : n_seg;
  return true;
}

// The OR of every long segment's values, per measure (blockIdx.y): the bytes above its top bit are zero.
__global__ __launch_bounds__(kThreads) void k_svq_long_or(SelArgs a) {
  __shared__ unsigned long long s_any[kThreads / 64];
  const uint32_t t = threadIdx.x, m = blockIdx.y;
  const uint32_t n_long = a.head->n_long, n_chunks = a.head->n_chunks;
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // workgroup-uniform
    const uint32_t slot = find_slot(a.slots, n_long, chunk);
    Slot &x = a.slots[slot];
    uint32_t begin, end;
    if (!chunk_range(x, chunk, a.cap, begin, end)) continue;
    const unsigned long long *seg = a.seg + m * a.cap + x.off;
    unsigned long long any = 0;
    for (uint32_t i = begin + t; i < end; i += kThreads) any |= seg[i];
    for (int d = 32; d; d >>= 1) any |= __shfl_xor(any, d, 64);
    __syncthreads();  // the previous chunk's s_any has been read
    if ((t & 63u) == 0) s_any[t >> 6] = any;
    __syncthreads();
    if (t == 0) {
      any = 0;
      for (uint32_t w = 0; w < kThreads / 64; ++w) any |= s_any[w];
      if (any) atomicOr(&x.any[m], any);
    }
  }
}

// One workgroup per (long segment, measure): the ranks from the counts, one group per non-empty class, the
// top byte, the counts into the table, and the segment's bins cleared.
__global__ __launch_bounds__(kThreads) void k_svq_long_setup(SelArgs a) {
  const uint32_t t = threadIdx.x, slot = blockIdx.x, m = blockIdx.y;
  if (slot >= a.head->n_long) return;  // workgroup-uniform
  Slot &x = a.slots[slot];
  const uint32_t n_q = a.n_q, ow = 1u + n_q;
  unsigned long long *om = a.out + ((uint64_t)x.svc * kMeasures + m) * kClasses * ow;
  rs::setup(x.st[m], t, n_q, x.n200 + x.n500, x.n200, x.n500, a.ppm, om);
  if (t == 0) x.st[m].owner_word = (uint32_t)rs::top_byte(x.any[m]);
  const uint32_t words = kClasses * n_q * kBins;
  uint32_t *bins = a.bins + ((uint64_t)slot * kMeasures + m) * words;
  for (uint32_t i = t; i < words; i += kThreads) bins[i] = 0;
}

// Digit pass `byte` of measure blockIdx.y over the long segments: a workgroup takes chunks, each a
// rs::hist_pass into its segment's bins.
__global__ __launch_bounds__(kHistThreads) void k_svq_long_hist(SelArgs a, int byte) {
  __shared__ rs::HistLds lds;
  const uint32_t wave = threadIdx.x >> 6, m = blockIdx.y;
  const uint32_t n_long = a.head->n_long, n_chunks = a.head->n_chunks;
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // workgroup-uniform
    const uint32_t slot = find_slot(a.slots, n_long, chunk);
    const Slot &x = a.slots[slot];
    if (byte > (int)x.st[m].owner_word) continue;  // every value is zero in this byte: the prefixes keep a zero digit
    uint32_t begin, end;
    if (!chunk_range(x, chunk, a.cap, begin, end)) continue;
    __syncthreads();  // the previous chunk's flush has read the bins
    const auto keys = [&] {
      const unsigned long long *seg = a.seg + m * a.cap + x.off;
      const uint32_t n200 = x.n200;
      return [=](uint32_t i, bool live) { return rs::Key{live ? seg[i] : 0, rs::seg_class(i, n200)}; };
    };
    // a wave takes 64 * kUnroll consecutive elements per step
    rs::hist_pass(lds, x.st[m], a.n_q, byte, begin + wave * (64 * kUnroll), end, kHistWaves * (64 * kUnroll), keys,
                  a.bins + ((uint64_t)slot * kMeasures + m) * kClasses * a.n_q * kBins);
  }
}

// After digit pass `byte`, one workgroup per (long segment, measure): rs::resolve_pass.
__global__ __launch_bounds__(kResolveThreads) void k_svq_long_resolve(SelArgs a, int byte) {
  const uint32_t slot = blockIdx.x, m = blockIdx.y;
  if (slot >= a.head->n_long) return;  // workgroup-uniform
  Slot &x = a.slots[slot];
  rs::State<uint32_t> &st = x.st[m];
  rs::resolve_pass(st, a.bins + ((uint64_t)slot * kMeasures + m) * kClasses * a.n_q * kBins, a.n_q, byte,
                   (int)st.owner_word, a.out + ((uint64_t)x.svc * kMeasures + m) * kClasses * (1u + a.n_q));
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
  hipLaunchKernelGGL(k_svq_count, dim3(grid), dim3(kThreads), 0, s, k);
  hipLaunchKernelGGL(k_svq_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)k.cnt, (uint32_t *)(ws + l.off),
                     k.cur, n_services, a.slots, a.n_slots, a.head);
  hipLaunchKernelGGL(k_svq_scatter, dim3(grid), dim3(kThreads), 0, s, k);
  hipLaunchKernelGGL(k_svq_short, dim3(std::min(n_services, kSelMaxGrid)), dim3(kSelThreads), 0, s, a);
  if (a.n_slots) {  // cap_spans allows a long segment: the passes are issued whatever the spans are
    const uint64_t max_chunks = cap_spans / kChunk + a.n_slots;
    const dim3 chunks(rs::grid_for(max_chunks, 1, kHistMaxGrid), kMeasures), segs(a.n_slots, kMeasures);
    hipLaunchKernelGGL(k_svq_long_or, chunks, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_svq_long_setup, segs, dim3(kThreads), 0, s, a);
    for (int byte = 7; byte >= 0; --byte) {
      hipLaunchKernelGGL(k_svq_long_hist, chunks, dim3(kHistThreads), 0, s, a, byte);
      hipLaunchKernelGGL(k_svq_long_resolve, segs, dim3(kResolveThreads), 0, s, a, byte);
    }
  }
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
