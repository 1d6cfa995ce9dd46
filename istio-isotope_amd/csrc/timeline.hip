// The load-test timeline (include/isim.h isim_timeline*): per
// window of simulated time the requests that arrived, and of those that
// completed in it, by response code, their count, latency sum, latency
// maximum and Prometheus histogram.  One pass over 24 B per trace (arrival +
// record), accumulated into the caller's table: one launch on the caller's
// stream, no workspace, no host synchronisation, no workgroup waits for
// another.
//
// A workgroup takes a tile of consecutive traces.  A DES batch's arrivals
// ascend with the trace id, so the tile arrives in a few adjacent windows and
// mostly completes in those or the next ones: the workgroup keeps kRows
// consecutive table rows in LDS, anchored at the lowest row an arrival of the
// tile's first 1024 traces falls in (taken from the data, not assumed), and
// updates outside that run go to the table as global atomics.  Before either
// kind of update the lanes of a wave that hit the same word add up among
// themselves (ballots; DPP reductions for the latency sum and maximum).  A
// tile whose times scatter is as exact, only slower.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "des_bucket.h"
#include "host_stage.h"
#include "timeline_row.h"
#include "trace_rec_dev.h"
#include "wave_peel.h"

namespace {

using isim::dev::rec4;

constexpr uint32_t kW = ISIM_TL_ROW_WORDS;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kUnroll = 4;                       // records per lane in flight
constexpr uint32_t kStep = kThreads * kUnroll;        // records per workgroup step
constexpr uint32_t kSteps = 4;
constexpr uint32_t kTile = kStep * kSteps;            // consecutive records per workgroup
constexpr uint32_t kRows = 64;                        // table rows cached in LDS (36.5 KB)
constexpr uint32_t kPeel = 4;                         // shared words a wave adds up per update before the rest go singly
constexpr uint64_t kMaxRecords = 1ull << 40;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kW == 7 + 2 * ISIM_N_PROM, "row layout");
static_assert((uint64_t)(ISIM_TL_MAX_WINDOWS + 2) * kW < (1ull << 31), "word indices fit 32 bits");

int tfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

struct TlArgs {
  const uint64_t *arr;
  const rec4 *rec;
  unsigned long long *out;
  uint64_t n, t0, window;
  uint64_t recip;      // floor((2^64 - 1) / window)
  uint32_t n_windows;
  uint32_t shift;      // window = 2^shift (pow2), else unused
  uint32_t pow2;
};

// the table row of time x (timeline_row.h)
__device__ __forceinline__ uint32_t tl_row(const TlArgs &a, uint64_t x) { return isim::tl::row_of(a, x); }

// the wave reductions of wave_peel.h
using isim::dev::OpAdd;
using isim::dev::OpMax;
using isim::dev::wave_reduce;

// ---- one update of word `off` of table row `row`: the LDS run or the table
struct Tile {
  unsigned long long *lds;  // [kRows][kW]
  unsigned long long *out;
  uint32_t anchor;
};
__device__ __forceinline__ void tl_add(const Tile &t, uint32_t row, uint32_t off, uint64_t v) {
  const uint32_t d = row - t.anchor;  // a row below the anchor wraps to a large value
  if (d < kRows) atomicAdd(&t.lds[d * kW + off], (unsigned long long)v);
  else atomicAdd(&t.out[(uint64_t)row * kW + off], (unsigned long long)v);
}
__device__ __forceinline__ void tl_max(const Tile &t, uint32_t row, uint32_t off, uint64_t v) {
  const uint32_t d = row - t.anchor;
  if (d < kRows) atomicMax(&t.lds[d * kW + off], (unsigned long long)v);
  else atomicMax(&t.out[(uint64_t)row * kW + off], (unsigned long long)v);
}

// word[key] += 1 per lane (key = row * kW + offset; kNone: no update): the
// peel of wave_peel.h, at most kPeel shared keys before the rest add one each
__device__ __forceinline__ void wave_count(const Tile &t, uint32_t key) {
  isim::dev::wave_peel<kPeel>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        if ((int)(threadIdx.x & 63u) == lead) tl_add(t, k0 / kW, k0 % kW, (uint64_t)__popcll(m));
      },
      [&](uint32_t k) { tl_add(t, k / kW, k % kW, 1); });
}

// the completion words of (row, code) = key >> 1, key & 1: count, latency sum
// and latency maximum, added up the same way
__device__ __forceinline__ void wave_done(const Tile &t, uint32_t key, uint64_t lat) {
  isim::dev::wave_peel<kPeel>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        const bool mine = key == k0;
        const uint64_t sum = wave_reduce<OpAdd>(mine ? lat : 0);
        const uint64_t mx = wave_reduce<OpMax>(mine ? lat : 0);
        if ((int)(threadIdx.x & 63u) == lead) {
          const uint32_t row = k0 >> 1, code = k0 & 1u;
          tl_add(t, row, ISIM_TL_DONE + code, (uint64_t)__popcll(m));
          if (sum) tl_add(t, row, ISIM_TL_SUM_LAT + code, sum);
          if (mx) tl_max(t, row, ISIM_TL_MAX_LAT + code, mx);
        }
      },
      [&](uint32_t k) {
        const uint32_t row = k >> 1, code = k & 1u;
        tl_add(t, row, ISIM_TL_DONE + code, 1);
        if (lat) {
          tl_add(t, row, ISIM_TL_SUM_LAT + code, lat);
          tl_max(t, row, ISIM_TL_MAX_LAT + code, lat);
        }
      });
}

__global__ __launch_bounds__(kThreads) void k_timeline(TlArgs a) {
  __shared__ unsigned long long s_rows[kRows * kW];
  __shared__ uint32_t s_lut[isim::dev::kBucketLutWords];
  __shared__ uint32_t s_not_anchor;  // ~(lowest arrival row of the first step)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  isim::dev::des_bucket_lut_init(reinterpret_cast<uint8_t *>(s_lut));
  for (uint32_t i = t; i < kRows * kW; i += kThreads) s_rows[i] = 0;
  if (t == 0) s_not_anchor = 0;
  __syncthreads();
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut);
  Tile tile{s_rows, a.out, 0};
  const uint64_t tile_base = (uint64_t)blockIdx.x * kTile;
  for (uint32_t step = 0; step < kSteps; ++step) {
    // a wave takes 64 * kUnroll consecutive records per step
    const uint64_t base = tile_base + (uint64_t)step * kStep + (uint64_t)wave * (64 * kUnroll);
    if (tile_base + (uint64_t)step * kStep >= a.n) break;  // workgroup-uniform
    rec4 r[kUnroll];
    uint64_t arr[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint64_t i = base + u * 64 + lane;
      const bool live = i < a.n;
      arr[u] = live ? a.arr[i] : 0;
      r[u] = isim::dev::load_rec(a.rec, i, live);
    }
    uint32_t ra[kUnroll], kc[kUnroll], kp[kUnroll];
    uint64_t lat[kUnroll];
    uint32_t lowest = 0;  // max of ~row over the live lanes
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const bool live = base + u * 64 + lane < a.n;
      lat[u] = isim::dev::latency(r[u]);
      const uint64_t c = isim::dev::completion(arr[u], lat[u]);
      const uint32_t code = isim::dev::code(r[u]);
      const uint32_t row_a = tl_row(a, arr[u]), row_c = tl_row(a, c);
      ra[u] = live ? row_a * kW + ISIM_TL_ARRIVED : kNone;
      kc[u] = live ? row_c * 2u + code : kNone;
      kp[u] = live ? row_c * kW + ISIM_TL_PROM + code * ISIM_N_PROM + isim::dev::des_prom_bucket(lut, lat[u]) : kNone;
      if (live) lowest = max(lowest, ~row_a);
    }
    if (step == 0) {
      const uint32_t w = (uint32_t)wave_reduce<OpMax>(lowest);
      if (lane == 0) atomicMax(&s_not_anchor, w);
      __syncthreads();
      tile.anchor = ~s_not_anchor;
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      wave_count(tile, ra[u]);
      wave_done(tile, kc[u], lat[u]);
      wave_count(tile, kp[u]);
    }
  }
  __syncthreads();
  // the flush: nonzero words of the rows that exist
  const uint32_t rows = a.n_windows + 2u;
  for (uint32_t i = t; i < kRows * kW; i += kThreads) {
    const unsigned long long v = s_rows[i];
    const uint32_t row = tile.anchor + i / kW, off = i % kW;
    if (!v || row >= rows) continue;
    unsigned long long *p = &a.out[(uint64_t)row * kW + off];
    if (off == ISIM_TL_MAX_LAT || off == ISIM_TL_MAX_LAT + 1) atomicMax(p, v);
    else atomicAdd(p, v);
  }
}

int check_params(const isim_timeline_params *p, uint64_t n) {
  if (const char *m = isim::tl::params_error(p)) return tfail(m);
  if (n > kMaxRecords) return tfail("n is above 2^40");
  return ISIM_OK;
}

uint64_t out_words(uint32_t n_windows) { return ((uint64_t)n_windows + 2) * kW; }

}  // namespace

extern "C" {

int isim_timeline_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                         const isim_timeline_params *p, uint64_t *d_out, void *hip_stream) {
  if (const int rc = check_params(p, n)) return rc;
  if (!d_out) return tfail("null d_out");
  if (n && (!d_arrivals || !d_records)) return tfail("null d_arrivals or d_records");
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_arrivals & 7u) || ((uintptr_t)d_out & 7u))
    return tfail("d_records must be 16-byte aligned, d_arrivals and d_out 8-byte aligned");
  if (n == 0) return ISIM_OK;
  TlArgs a{};
  a.arr = d_arrivals;
  a.rec = (const rec4 *)d_records;
  a.out = (unsigned long long *)d_out;
  a.n = n;
  isim::tl::set_row_args(a, *p);
  const uint64_t grid = (n + kTile - 1) / kTile;  // n <= 2^40: at most 2^28 workgroups
  hipLaunchKernelGGL(k_timeline, dim3((uint32_t)grid), dim3(kThreads), 0, (hipStream_t)hip_stream, a);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int isim_timeline(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records, uint64_t n,
                  const isim_timeline_params *p, uint64_t *h_out) {
  if (const int rc = check_params(p, n)) return rc;
  if (!h_out) return tfail("null h_out");
  if (n && (!h_arrivals || !h_records)) return tfail("null h_arrivals or h_records");
  if (n == 0) return ISIM_OK;
  const uint64_t out_bytes = out_words(p->n_windows) * 8;
  isim::HostStage stage(device);
  void *d_out = stage.upload(h_out, out_bytes);  // h_out is accumulated into like d_out: it goes up first
  void *d_arr = stage.upload(h_arrivals, n * 8), *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_timeline_device((const uint64_t *)d_arr, (const isim_trace_rec *)d_rec, n, p,
                                          (uint64_t *)d_out, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, out_bytes);
}

int isim_timeline_merge(uint32_t n_windows, uint64_t *dst, const uint64_t *src) {
  if (!dst || !src) return tfail("null argument");
  if (n_windows == 0 || n_windows > ISIM_TL_MAX_WINDOWS)
    return tfail("n_windows must be 1.." + std::to_string(ISIM_TL_MAX_WINDOWS));
  const uint64_t rows = (uint64_t)n_windows + 2;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint32_t w = 0; w < kW; ++w) {
      const uint64_t i = r * kW + w;
      if (w == ISIM_TL_MAX_LAT || w == ISIM_TL_MAX_LAT + 1) dst[i] = std::max(dst[i], src[i]);
      else dst[i] += src[i];
    }
  return ISIM_OK;
}

}  // extern "C"
