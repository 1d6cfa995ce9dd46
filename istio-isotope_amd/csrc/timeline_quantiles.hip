// Per-window exact latency percentiles (include/isim.h isim_timeline_quantiles*,
// DESIGN.md §15): for every row of the timeline (§14) the order statistics of
// the latencies that COMPLETE in it, per class (all / 200 / 500).  Five
// launches on the caller's stream: clear, count per (row, code), one-workgroup
// exclusive scan, scatter of the latencies into one segment per row (its 200s,
// then its 500s), and a select in which a workgroup owns a row and runs §13's
// MSD radix select over it as a loop.  No host synchronisation, no
// allocation, no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "host_stage.h"
#include "quantile_rank.h"
#include "segmented_select.h"
#include "timeline_row.h"
#include "trace_rec_dev.h"

namespace {

namespace rs = isim::rs;
using isim::dev::rec4;
using rs::kBins;
using rs::kClasses;
using rs::kMaxQ;
using rs::kSelThreads;
using rs::kStage;
using rs::kUnroll;
using rs::u32x4;

constexpr uint32_t kThreads = 256;        // count, scatter, clear
constexpr uint32_t kMaxGrid = 2048;       // count and scatter stride past it
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanTile = kScanThreads * 4;
constexpr uint32_t kSelMaxGrid = 512;     // two workgroups per CU by LDS
constexpr uint64_t kMaxRecords = 0xFFFFFFFFull;  // u32 counters, offsets and ranks
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kHeadBytes = 256;      // the row ticket

int tfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

// The workspace: the ticket, then three u32 arrays of one word per (row, code)
// (counts, segment offsets, scatter cursors), then the n latencies by row.
struct Layout {
  uint64_t counters;  // 2 * (n_windows + 2)
  uint64_t cnt, off, cur, seg, total;
};
Layout layout(uint64_t n, uint32_t n_windows) {
  Layout l{};
  l.counters = 2 * ((uint64_t)n_windows + 2);
  const uint64_t cbytes = (l.counters * 4 + 255) & ~255ull;
  l.cnt = kHeadBytes;
  l.off = l.cnt + cbytes;
  l.cur = l.off + cbytes;
  l.seg = l.cur + cbytes;
  l.total = l.seg + n * 8;
  return l;
}

struct TqArgs {
  const uint64_t *arr;
  const rec4 *rec;
  uint32_t *cnt;             // count: [rows][2], added to
  uint32_t *cur;             // scatter: [rows][2] cursors
  unsigned long long *seg;   // scatter: [n]
  uint64_t n, t0, window;
  uint64_t recip;      // floor((2^64 - 1) / window)
  uint32_t n_windows;
  uint32_t shift;      // window = 2^shift (pow2), else unused
  uint32_t pow2;
};

__global__ __launch_bounds__(kThreads) void k_tlq_clear(uint32_t *words, uint64_t n_words) {
  rs::clear_words<kThreads>(words, n_words);
}

// a wave's kUnroll * 64 consecutive records from `base`: per record the key
// 2 * (row of its completion) + code (kNone past n) and the latency
__device__ __forceinline__ void load_keys(const TqArgs &a, uint64_t base, uint32_t lane, uint32_t (&key)[kUnroll],
                                          uint64_t (&lat)[kUnroll]) {
  rec4 r[kUnroll];
  uint64_t arr[kUnroll];
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    const uint64_t i = base + u * 64 + lane;
    const bool live = i < a.n;
    arr[u] = live ? a.arr[i] : 0;
    r[u] = isim::dev::load_rec(a.rec, i, live);
  }
#pragma unroll
  for (uint32_t u = 0; u < kUnroll; ++u) {
    lat[u] = isim::dev::latency(r[u]);
    const uint64_t c = isim::dev::completion(arr[u], lat[u]);
    key[u] = base + u * 64 + lane < a.n ? isim::tl::row_of(a, c) * 2u + isim::dev::code(r[u]) : kNone;
  }
}

// Pass 1: records per (row, code).
__global__ __launch_bounds__(kThreads) void k_tlq_count(TqArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  // a wave takes 64 * kUnroll consecutive records per step; the loop bound is wave-uniform
  for (uint64_t base = wave * (64 * kUnroll); base < a.n; base += step) {
    uint32_t key[kUnroll];
    uint64_t lat[kUnroll];
    load_keys(a, base, lane, key, lat);
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) rs::wave_add(a.cnt, (int)key[u], lane);  // kNone: no bin
  }
}

// Exclusive scan of the counters into the segment offsets and the scatter
// cursors: one workgroup, tiles of 4096 counters (a 16-byte load per thread, a
// shuffle scan per wave, the 16 wave totals through LDS) with a running carry.
// The arrays are padded to 256 B, so the last load stays inside them; words
// past n_counters are not used and not written.
__global__ __launch_bounds__(kScanThreads) void k_tlq_scan(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off,
                                                          uint32_t *__restrict__ cur, uint32_t n_counters) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t carry = 0;
  for (uint32_t tile = 0; tile < n_counters; tile += kScanTile) {
    const uint32_t i = tile + 4 * t;
    u32x4 v{0, 0, 0, 0};
    if (i < n_counters) v = *reinterpret_cast<const u32x4 *>(cnt + i);
    if (i + 1 >= n_counters) v.y = 0;
    if (i + 2 >= n_counters) v.z = 0;
    if (i + 3 >= n_counters) v.w = 0;
    uint32_t total;
    const uint32_t e0 = carry + rs::block_scan<kScanThreads>(v.x + v.y + v.z + v.w, s_wave, lane, wave, total);
    const u32x4 e{e0, e0 + v.x, e0 + v.x + v.y, e0 + v.x + v.y + v.z};
    if (i + 3 < n_counters) {
      *reinterpret_cast<u32x4 *>(off + i) = e;
      *reinterpret_cast<u32x4 *>(cur + i) = e;
    } else {
      if (i < n_counters) off[i] = cur[i] = e.x;
      if (i + 1 < n_counters) off[i + 1] = cur[i + 1] = e.y;
      if (i + 2 < n_counters) off[i + 2] = cur[i + 2] = e.z;
    }
    carry += total;
  }
}

// Pass 2: each latency to its row's segment.  A position past n cannot come
// from counts and cursors of the same records; were the records changed under
// the call, nothing is written outside the segment array.
__global__ __launch_bounds__(kThreads) void k_tlq_scatter(TqArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kThreads / 64) * (64 * kUnroll);
  for (uint64_t base = wave * (64 * kUnroll); base < a.n; base += step) {
    uint32_t key[kUnroll];
    uint64_t lat[kUnroll];
    load_keys(a, base, lane, key, lat);
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t pos = isim::dev::wave_claim(a.cur, key[u], kNone, lane);
      if (key[u] != kNone && pos < a.n) a.seg[pos] = lat[u];
    }
  }
}

struct SelArgs {
  const uint32_t *cnt;             // [rows][2]
  const uint32_t *off;             // [rows][2]
  const unsigned long long *seg;   // [n]
  uint32_t *ticket;
  unsigned long long *out;         // [rows][3][1 + n_q]
  uint32_t rows, n_q;
  rs::Ppm ppm;
};

// The select.  A workgroup claims rows through the ticket until none is left.
// An empty row gets its zeros, any other the select of segmented_select.h,
// staged in LDS while it fits; the ticket is s.sel.owner_word.
__global__ __launch_bounds__(kSelThreads) void k_tlq_select(SelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[kClasses * kMaxQ * kBins];
  __shared__ unsigned long long s_stage[kStage];
  __shared__ rs::SelState s;
  const uint32_t t = threadIdx.x, ow = 1u + a.n_q;
  for (;;) {
    __syncthreads();  // the previous row's state has been read
    if (t == 0) s.sel.owner_word = atomicAdd(a.ticket, 1u);
    __syncthreads();
    const uint32_t row = s.sel.owner_word;
    if (row >= a.rows) return;  // workgroup-uniform
    const uint32_t n200 = a.cnt[2 * row], n500 = a.cnt[2 * row + 1];
    const uint32_t n_row = n200 + n500;  // at most n < 2^32
    unsigned long long *out = a.out + (uint64_t)row * kClasses * ow;
    if (n_row == 0) {
      for (uint32_t i = t; i < kClasses * ow; i += kSelThreads) out[i] = 0;
      continue;
    }
    rs::select_segment<false>(hist, s_stage, s, a.seg + a.off[2 * row], n_row, n200, n_row <= kStage, a.n_q, a.ppm, out);
  }
}

// everything the three entry points reject alike; the quantile list comes after the parameters
int check_common(const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q, uint64_t n) {
  if (const char *m = isim::tl::params_error(p)) return tfail(m);
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return tfail(m);
  if (n > kMaxRecords) return tfail("n is above 2^32 - 1");
  return ISIM_OK;
}

}  // namespace

extern "C" {

int isim_timeline_quantiles_workspace_bytes(uint64_t n, uint32_t n_windows, uint32_t n_q, uint64_t *bytes) {
  if (!bytes) return tfail("null argument");
  if (n_windows == 0 || n_windows > ISIM_TL_MAX_WINDOWS) return tfail("n_windows must be 1..65536");
  if (n_q == 0 || n_q > kMaxQ) return tfail("n_q must be 1.." + std::to_string(kMaxQ));
  if (n > kMaxRecords) return tfail("n is above 2^32 - 1");
  *bytes = layout(n, n_windows).total;
  return ISIM_OK;
}

int isim_timeline_quantiles_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                                   const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q,
                                   uint64_t *d_out, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  if (const int rc = check_common(p, q_ppm, n_q, n)) return rc;
  if (!d_out || !d_workspace) return tfail("null d_out or d_workspace");
  if (n && (!d_arrivals || !d_records)) return tfail("null d_arrivals or d_records");
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_arrivals & 7u) || ((uintptr_t)d_out & 7u) ||
      ((uintptr_t)d_workspace & 7u))
    return tfail("d_records must be 16-byte aligned, d_arrivals, d_out and d_workspace 8-byte aligned");
  const Layout l = layout(n, p->n_windows);
  if (workspace_bytes < l.total)
    return tfail("workspace too small: " + std::to_string(workspace_bytes) + " bytes, need " +
                 std::to_string(l.total) + " (isim_timeline_quantiles_workspace_bytes)");
  const hipStream_t s = (hipStream_t)hip_stream;
  const uint32_t rows = p->n_windows + 2;
  if (n == 0) {
    const uint64_t words = 2 * ISIM_TLQ_OUT_WORDS(p->n_windows, n_q);  // u32
    hipLaunchKernelGGL(k_tlq_clear, dim3(rs::grid_for(words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
                       (uint32_t *)d_out, words);
    ISIM_HIPCHK(hipGetLastError());
    return ISIM_OK;
  }
  char *ws = (char *)d_workspace;
  TqArgs a{};
  a.arr = d_arrivals;
  a.rec = (const rec4 *)d_records;
  a.cnt = (uint32_t *)(ws + l.cnt);
  a.cur = (uint32_t *)(ws + l.cur);
  a.seg = (unsigned long long *)(ws + l.seg);
  a.n = n;
  isim::tl::set_row_args(a, *p);
  SelArgs sel{};
  sel.cnt = a.cnt;
  sel.off = (const uint32_t *)(ws + l.off);
  sel.seg = a.seg;
  sel.ticket = (uint32_t *)ws;
  sel.out = (unsigned long long *)d_out;
  sel.rows = rows;
  sel.n_q = n_q;
  sel.ppm = rs::ppm_of(q_ppm, n_q);

  // the ticket and the counts, contiguous from the workspace's start (every clear is a kernel: §13)
  const uint64_t clear_words = l.cnt / 4 + l.counters;
  hipLaunchKernelGGL(k_tlq_clear, dim3(rs::grid_for(clear_words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
                     (uint32_t *)ws, clear_words);
  const uint32_t grid = rs::grid_for(n, kThreads * kUnroll, kMaxGrid);
  hipLaunchKernelGGL(k_tlq_count, dim3(grid), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_tlq_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)a.cnt, (uint32_t *)(ws + l.off),
                     a.cur, (uint32_t)l.counters);
  hipLaunchKernelGGL(k_tlq_scatter, dim3(grid), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(k_tlq_select, dim3(std::min(rows, kSelMaxGrid)), dim3(kSelThreads), 0, s, sel);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int isim_timeline_quantiles(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records, uint64_t n,
                            const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q, uint64_t *h_out) {
  if (const int rc = check_common(p, q_ppm, n_q, n)) return rc;
  if (!h_out) return tfail("null h_out");
  if (n && (!h_arrivals || !h_records)) return tfail("null h_arrivals or h_records");
  const uint64_t out_bytes = ISIM_TLQ_OUT_WORDS(p->n_windows, n_q) * 8, wsb = layout(n, p->n_windows).total;
  isim::HostStage stage(device);
  void *d_out = stage.alloc(out_bytes), *d_ws = stage.alloc(wsb);
  void *d_arr = stage.upload(h_arrivals, n * 8), *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_timeline_quantiles_device((const uint64_t *)d_arr, (const isim_trace_rec *)d_rec, n, p, q_ppm,
                                                    n_q, (uint64_t *)d_out, d_ws, wsb, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, out_bytes);
}

}  // extern "C"
