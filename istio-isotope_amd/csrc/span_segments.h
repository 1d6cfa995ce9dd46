// The spans of a tapped batch as segments of u64 keys, device only: what
// service_quantiles.hip (a segment per service) and
// service_window_quantiles.hip (§29, a segment per (service, timeline row))
// share.  The span load with the refusal rule and the three measures, the
// count per (segment, code) and the scatter of the measures to the segments
// (both take the caller's key of a span), and the long segments (more than
// kStage spans): their slots and the chunked launches over them, which are
// segmented_select.h's hist_pass / resolve_pass.  The callers own the scan that
// numbers the segments, the select of the shorter ones and the order of the
// launches.  A segment's cells are out[segment][kMeasures][kClasses][1 + n_q].
#pragma once

#include <hip/hip_runtime.h>

#include "segmented_select.h"
#include "service_quantiles.h"

namespace isim {
namespace svq {

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
constexpr uint32_t kSelMaxGrid = 512;  // two workgroups per CU by LDS: 48 KB of bins + 28 KB of stage + 1.2 KB of state
constexpr uint32_t kHistWaves = kHistThreads / 64;
constexpr uint32_t kHistMaxGrid = 1024;  // per measure
static_assert(kChunk % (kHistThreads * kUnroll) == 0 && kChunk % kThreads == 0, "a chunk is whole steps of a workgroup");

struct Head {
  uint32_t ticket;    // the LDS select: the next segment
  uint32_t n_long;    // long segments
  uint32_t n_chunks;  // their chunks
};
static_assert(sizeof(Head) <= kHeadBytes, "the head fits its bytes");

// a long segment; the select's top byte of measure m is st[m].owner_word (as int; -1: every value is 0)
struct Slot {
  uint32_t svc, chunk0, n200, n500;  // svc: the segment
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
  uint32_t *cnt;            // count: [segments][2], added to
  uint32_t *cur;            // scatter: [segments][2] cursors
  unsigned long long *seg;  // scatter: [kMeasures][cap]
  unsigned long long *hdr;  // the table's header
};

// the key of a span that is not refused: 2 * segment + code; §28's segment is the service
struct ServiceKey {
  __device__ __forceinline__ uint32_t operator()(uint32_t svc, uint32_t status, uint64_t) const {
    return svc * 2u + (status & 1u);
  }
};

__device__ __forceinline__ uint64_t span_count(const SK &k) {
  const uint64_t end = k.off[k.info[ISIM_SPAN_WRITTEN]];
  return end < k.cap ? end : k.cap;
}

static __global__ __launch_bounds__(kThreads) void k_svq_clear(uint32_t *a, uint64_t na, uint32_t *b, uint64_t nb) {
  rs::clear_words<kThreads>(a, na);
  rs::clear_words<kThreads>(b, nb);
}

// a wave's kUnroll * 64 consecutive spans from `base`: per span the key key_of(service, status, finish) (kNone
// past n or refused) and the three measures
template <typename KeyOf>
__device__ __forceinline__ void load_keys(const SK &k, const KeyOf &key_of, uint64_t n, uint64_t base, uint32_t lane,
                                          uint32_t (&key)[kUnroll], uint64_t (&val)[kUnroll][kMeasures],
                                          uint32_t &refused) {
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
    key[u] = live && !bad ? key_of(svc[u], st[u], f[u]) : kNone;
#pragma unroll
    for (uint32_t m = 0; m < kMeasures; ++m) val[u][m] = measure(m, a[u], s[u], f[u]);
  }
}

// Pass 1: spans per (segment, code), and the header.
template <typename KeyOf>
static __global__ __launch_bounds__(kThreads) void k_svq_count(SK k, KeyOf key_of) {
  const uint64_t n = span_count(k);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  uint32_t refused = 0, folded = 0;
  // a wave takes 64 * kUnroll consecutive spans per step; the loop bound is wave-uniform
  for (uint64_t base = wave * (64 * kUnroll); base < n; base += step) {
    uint32_t key[kUnroll];
    uint64_t val[kUnroll][kMeasures];
    load_keys(k, key_of, n, base, lane, key, val, refused);
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

// Pass 2: the three measures of each span to its segment (its 200s, then its 500s).  A position past cap
// cannot come from counts and cursors of the same spans; were the spans changed under the call, nothing is
// written outside the segment arrays.
template <typename KeyOf>
static __global__ __launch_bounds__(kThreads) void k_svq_scatter(SK k, KeyOf key_of) {
  const uint64_t n = span_count(k);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  uint32_t refused = 0;
  for (uint64_t base = wave * (64 * kUnroll); base < n; base += step) {
    uint32_t key[kUnroll];
    uint64_t val[kUnroll][kMeasures];
    load_keys(k, key_of, n, base, lane, key, val, refused);
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
  const uint32_t *cnt;            // [segments][2]
  const uint32_t *off;            // [segments][2]
  const unsigned long long *seg;  // [kMeasures][cap]
  uint64_t cap;
  Head *head;
  Slot *slots;
  uint32_t *bins;           // [n_slots][kMeasures][kClasses][n_q][kBins]
  unsigned long long *out;  // [segments][kMeasures][kClasses][1 + n_q]
  uint32_t n_services, n_q, n_slots;  // n_services: the segments
  rs::Ppm ppm;
};

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
static __global__ __launch_bounds__(kThreads) void k_svq_long_or(SelArgs a) {
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
static __global__ __launch_bounds__(kThreads) void k_svq_long_setup(SelArgs a) {
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
static __global__ __launch_bounds__(kHistThreads) void k_svq_long_hist(SelArgs a, int byte) {
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
static __global__ __launch_bounds__(kResolveThreads) void k_svq_long_resolve(SelArgs a, int byte) {
  const uint32_t slot = blockIdx.x, m = blockIdx.y;
  if (slot >= a.head->n_long) return;  // workgroup-uniform
  Slot &x = a.slots[slot];
  rs::State<uint32_t> &st = x.st[m];
  rs::resolve_pass(st, a.bins + ((uint64_t)slot * kMeasures + m) * kClasses * a.n_q * kBins, a.n_q, byte,
                   (int)st.owner_word, a.out + ((uint64_t)x.svc * kMeasures + m) * kClasses * (1u + a.n_q));
}

// The launches over the long segments, issued whatever the spans are when cap_spans allows one (a.n_slots):
// every kernel reads the long segments' count on the device and leaves when there is nothing for it.
inline void launch_long(const SelArgs &a, uint64_t cap_spans, hipStream_t s) {
  if (!a.n_slots) return;
  const uint64_t max_chunks = cap_spans / kChunk + a.n_slots;
  const dim3 chunks(rs::grid_for(max_chunks, 1, kHistMaxGrid), kMeasures), segs(a.n_slots, kMeasures);
  hipLaunchKernelGGL(k_svq_long_or, chunks, dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_svq_long_setup, segs, dim3(kThreads), 0, s, a);
  for (int byte = 7; byte >= 0; --byte) {
    hipLaunchKernelGGL(k_svq_long_hist, chunks, dim3(kHistThreads), 0, s, a, byte);
    hipLaunchKernelGGL(k_svq_long_resolve, segs, dim3(kResolveThreads), 0, s, a, byte);
  }
}

}  // namespace svq
}  // namespace isim
