// The mergeable latency sketch on the device (include/isim.h isim_latency_sketch*,
// isim_timeline_sketch*): a log-linear histogram of latency_ns
// per response code, for a whole batch or per row of the timeline (§14, §15:
// by completion).  One pass over the records (16 B per trace, 24 B with the
// arrivals), accumulated into the caller's table: one launch on the caller's
// stream, no workspace, no host synchronisation, no workgroup waits for
// another.
//
// A workgroup keeps a u32 table in LDS and flushes its nonzero words with
// global u64 atomics at the end.  The whole-batch kernel keeps the whole table
// [2][BINS] there and strides over the batch.  The per-window kernel takes a
// tile of consecutive traces (a DES batch's arrivals ascend with the trace id,
// so a tile completes in a few adjacent rows) and keeps as many consecutive
// rows as the same LDS holds, anchored at the lowest row a completion of the
// tile's first step falls in (taken from the data, not assumed); updates
// outside that run go to the table as global atomics.  Before either kind of
// update the lanes of a wave that hit the same word add once (wave_peel.h): the
// build turns the compiler's atomic optimizer off, and a constant batch puts
// all 64 lanes on one word.  A tile whose times scatter is as exact, only slower.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "host_stage.h"
#include "sketch_bucket.h"
#include "timeline_row.h"
#include "trace_rec_dev.h"
#include "wave_peel.h"

namespace {

namespace sk = isim::sk;
using isim::dev::rec4;

constexpr uint32_t kThreads = 512;
constexpr uint32_t kUnroll = 4;                          // records per lane in flight
constexpr uint32_t kStep = kThreads * kUnroll;           // records per workgroup step
constexpr uint32_t kLdsWords = 2 * ISIM_SK_BINS(7);      // 59,392 B of u32: two workgroups share a CU
constexpr uint32_t kMaxGrid = 512;                       // whole batch: two per CU; a workgroup's u32 LDS words hold 2^40 / 512 < 2^32 records
constexpr uint32_t kTileSteps = 4;
constexpr uint32_t kTile = kStep * kTileSteps;           // per window: consecutive records per workgroup
constexpr uint64_t kMaxRecords = 1ull << 40;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(ISIM_SK_BINS(7) == 7424 && ISIM_SK_BINS(3) == 496 && ISIM_SK_BINS(0) == 65, "the bucket rule's bin counts");
static_assert(ISIM_TLS_OUT_WORDS(ISIM_TL_MAX_WINDOWS, ISIM_SK_MAX_SUB_BITS) < (1ull << 32) - 1, "keys fit 32 bits below kNone");

int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

struct SkArgs {
  const uint64_t *arr;       // per window only
  const rec4 *rec;
  unsigned long long *out;
  uint64_t n, t0, window;
  uint64_t recip;            // floor((2^64 - 1) / window)
  uint32_t n_windows;
  uint32_t shift;            // window = 2^shift (pow2), else unused
  uint32_t pow2;
  uint32_t sub_bits;
  uint32_t bins;             // ISIM_SK_BINS(sub_bits)
  uint32_t lds_words;        // words of the table kept in LDS: whole rows of 2 * bins
};

// The LDS run of table words [first, first + words) and the table behind it.
struct Tile {
  uint32_t *lds;
  unsigned long long *out;
  uint32_t first, words;
};

// word[key] += v.  WINDOWED false: the whole table is in LDS.
template <bool WINDOWED>
__device__ __forceinline__ void sk_add(const Tile &t, uint32_t key, uint32_t v) {
  const uint32_t d = key - t.first;  // a key below the run wraps to a large value
  if (!WINDOWED || d < t.words) atomicAdd(&t.lds[d], v);
  else atomicAdd(&t.out[key], (unsigned long long)v);
}

// word[key] += 1 per lane (kNone: no update): the peel of wave_peel.h
template <bool WINDOWED>
__device__ __forceinline__ void wave_inc(const Tile &t, uint32_t key, uint32_t lane) {
  isim::dev::wave_peel<isim::dev::kPeelAll>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        if ((int)lane == lead) sk_add<WINDOWED>(t, k0, (uint32_t)__popcll(m));
      },
      [&](uint32_t k) { sk_add<WINDOWED>(t, k, 1u); });
}

// A wave's kUnroll * 64 consecutive records from `base`, each read once as one
// 16-byte load, all loads issued before the first use: per record its table
// word (row * 2 + code) * bins + bin (kNone past n), row 0 for a whole batch.
template <bool WINDOWED>
__device__ __forceinline__ void load_keys(const SkArgs &a, uint64_t base, uint32_t lane, uint32_t (&key)[kUnroll]) {
  rec4 r[kUnroll];
  uint64_t arr[kUnroll];
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    const uint64_t i = base + u * 64 + lane;
    const bool live = i < a.n;
    arr[u] = WINDOWED && live ? a.arr[i] : 0;
    r[u] = isim::dev::load_rec(a.rec, i, live);
  }
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    const uint64_t lat = isim::dev::latency(r[u]);
    const uint32_t row = WINDOWED ? isim::tl::row_of(a, isim::dev::completion(arr[u], lat)) : 0u;
    const uint32_t word = (row * 2u + isim::dev::code(r[u])) * a.bins + sk::bucket(a.sub_bits, lat);
    key[u] = base + u * 64 + lane < a.n ? word : kNone;
  }
}

// nonzero LDS words to the table; `limit`: the table's words (a run anchored near the last row ends past it)
__device__ __forceinline__ void flush(const Tile &t, uint32_t limit) {
  for (uint32_t i = threadIdx.x; i < t.words; i += kThreads) {
    const uint32_t v = t.lds[i];
    const uint32_t w = t.first + i;
    if (v && w < limit) atomicAdd(&t.out[w], (unsigned long long)v);
  }
}

// Whole batch: the table [2][bins] in LDS, one flush per workgroup.
__global__ __launch_bounds__(kThreads) void k_sketch(SkArgs a) {
  __shared__ uint32_t s_tab[kLdsWords];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const Tile tile{s_tab, a.out, 0u, a.lds_words};
  for (uint32_t i = t; i < tile.words; i += kThreads) s_tab[i] = 0;
  __syncthreads();
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (t >> 6);
  const uint64_t step = (uint64_t)gridDim.x * kStep;
  // a wave takes 64 * kUnroll consecutive records per step; the loop bound is wave-uniform
  for (uint64_t base = wave * (64 * kUnroll); base < a.n; base += step) {
    uint32_t key[kUnroll];
    load_keys<false>(a, base, lane, key);
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) wave_inc<false>(tile, key[u], lane);
  }
  __syncthreads();
  flush(tile, tile.words);
}

// Per window: a tile of kTile consecutive records, lds_words / (2 * bins) consecutive rows in LDS.
__global__ __launch_bounds__(kThreads) void k_timeline_sketch(SkArgs a) {
  __shared__ uint32_t s_tab[kLdsWords];
  __shared__ uint32_t s_not_anchor;  // ~(lowest completion row of the first step)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  Tile tile{s_tab, a.out, 0u, a.lds_words};
  for (uint32_t i = t; i < tile.words; i += kThreads) s_tab[i] = 0;
  if (t == 0) s_not_anchor = 0;
  __syncthreads();
  const uint32_t row_words = 2u * a.bins;
  const uint64_t tile_base = (uint64_t)blockIdx.x * kTile;
  for (uint32_t step = 0; step < kTileSteps; ++step) {
    if (tile_base + (uint64_t)step * kStep >= a.n) break;  // workgroup-uniform
    // a wave takes 64 * kUnroll consecutive records per step
    const uint64_t base = tile_base + (uint64_t)step * kStep + (uint64_t)wave * (64 * kUnroll);
    uint32_t key[kUnroll];
    load_keys<true>(a, base, lane, key);
    if (step == 0) {
      uint32_t lowest = 0;  // max of ~row over the live lanes
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u)
        if (key[u] != kNone) lowest = max(lowest, ~(key[u] / row_words));
      for (int d = 32; d; d >>= 1) lowest = max(lowest, (uint32_t)__shfl_xor((int)lowest, d, 64));
      if (lane == 0) atomicMax(&s_not_anchor, lowest);
      __syncthreads();  // the tile's first record exists, so some lane of the workgroup is live
      tile.first = ~s_not_anchor * row_words;
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) wave_inc<true>(tile, key[u], lane);
  }
  __syncthreads();
  flush(tile, (a.n_windows + 2u) * row_words);
}

// what both whole-batch entry points reject alike
int check_batch(uint32_t sub_bits, const void *records, uint64_t n, const void *table) {
  if (sub_bits > sk::kMaxSubBits) return sfail("sub_bits must be 0..7");
  if (!table) return sfail("null table");
  if (n && !records) return sfail("null records");
  if (n > kMaxRecords) return sfail("n is above 2^40");
  return ISIM_OK;
}

// and both per-window ones; the parameters come first, as in isim_timeline*
int check_windowed(const isim_timeline_params *p, uint32_t sub_bits, const void *arrivals, const void *records,
                   uint64_t n, const void *out) {
  if (const char *m = isim::tl::params_error(p)) return sfail(m);
  if (sub_bits > sk::kMaxSubBits) return sfail("sub_bits must be 0..7");
  if (!out) return sfail("null out");
  if (n && (!arrivals || !records)) return sfail("null arrivals or records");
  if (n > kMaxRecords) return sfail("n is above 2^40");
  return ISIM_OK;
}

}  // namespace

extern "C" {

int isim_latency_sketch_device(const isim_trace_rec *d_records, uint64_t n, uint32_t sub_bits, uint64_t *d_table,
                               void *hip_stream) {
  if (const int rc = check_batch(sub_bits, d_records, n, d_table)) return rc;
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_table & 7u))
    return sfail("d_records must be 16-byte aligned, d_table 8-byte aligned");
  if (n == 0) return ISIM_OK;
  SkArgs a{};
  a.rec = (const rec4 *)d_records;
  a.out = (unsigned long long *)d_table;
  a.n = n;
  a.sub_bits = sub_bits;
  a.bins = sk::bins(sub_bits);
  a.lds_words = 2 * a.bins;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kStep - 1) / kStep, kMaxGrid);
  hipLaunchKernelGGL(k_sketch, dim3(grid), dim3(kThreads), 0, (hipStream_t)hip_stream, a);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int isim_latency_sketch(int device, const isim_trace_rec *h_records, uint64_t n, uint32_t sub_bits, uint64_t *h_table) {
  if (const int rc = check_batch(sub_bits, h_records, n, h_table)) return rc;
  if (n == 0) return ISIM_OK;
  const uint64_t bytes = ISIM_SK_WORDS(sub_bits) * 8;
  isim::HostStage stage(device);
  void *d_table = stage.upload(h_table, bytes);  // h_table is accumulated into like d_table: it goes up first
  void *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_latency_sketch_device((const isim_trace_rec *)d_rec, n, sub_bits, (uint64_t *)d_table,
                                                stage.stream()))
    return rc;
  return stage.download(h_table, d_table, bytes);
}

int isim_timeline_sketch_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                                const isim_timeline_params *p, uint32_t sub_bits, uint64_t *d_out, void *hip_stream) {
  if (const int rc = check_windowed(p, sub_bits, d_arrivals, d_records, n, d_out)) return rc;
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_arrivals & 7u) || ((uintptr_t)d_out & 7u))
    return sfail("d_records must be 16-byte aligned, d_arrivals and d_out 8-byte aligned");
  if (n == 0) return ISIM_OK;
  SkArgs a{};
  a.arr = d_arrivals;
  a.rec = (const rec4 *)d_records;
  a.out = (unsigned long long *)d_out;
  a.n = n;
  isim::tl::set_row_args(a, *p);
  a.sub_bits = sub_bits;
  a.bins = sk::bins(sub_bits);
  const uint32_t lds_rows = std::min<uint32_t>(kLdsWords / (2 * a.bins), p->n_windows + 2);
  a.lds_words = lds_rows * 2 * a.bins;
  const uint64_t grid = (n + kTile - 1) / kTile;  // n <= 2^40: at most 2^27 workgroups
  hipLaunchKernelGGL(k_timeline_sketch, dim3((uint32_t)grid), dim3(kThreads), 0, (hipStream_t)hip_stream, a);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int isim_timeline_sketch(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records, uint64_t n,
                         const isim_timeline_params *p, uint32_t sub_bits, uint64_t *h_out) {
  if (const int rc = check_windowed(p, sub_bits, h_arrivals, h_records, n, h_out)) return rc;
  if (n == 0) return ISIM_OK;
  const uint64_t bytes = ISIM_TLS_OUT_WORDS(p->n_windows, sub_bits) * 8;
  isim::HostStage stage(device);
  void *d_out = stage.upload(h_out, bytes);  // accumulated into: it goes up first
  void *d_arr = stage.upload(h_arrivals, n * 8), *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_timeline_sketch_device((const uint64_t *)d_arr, (const isim_trace_rec *)d_rec, n, p, sub_bits,
                                                 (uint64_t *)d_out, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, bytes);
}

}  // extern "C"
