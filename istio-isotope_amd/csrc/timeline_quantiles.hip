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
#include "radix_select.h"
#include "timeline_row.h"
#include "trace_rec_dev.h"
#include "wave_peel.h"

namespace {

namespace rs = isim::rs;
using isim::dev::rec4;
using rs::kBins;
using rs::kClasses;
using rs::kMaxQ;

constexpr uint32_t kThreads = 256;        // count, scatter, clear
constexpr uint32_t kUnroll = 4;           // records per lane in flight
constexpr uint32_t kMaxGrid = 2048;       // count and scatter stride past it
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanTile = kScanThreads * 4;
constexpr uint32_t kSelThreads = 512;
constexpr uint32_t kSelWaves = kSelThreads / 64;
constexpr uint32_t kSelMaxGrid = 512;     // two workgroups per CU by LDS
constexpr uint32_t kStage = 3584;         // latencies of a row kept in LDS (28 KB): with the 48 KB of bins two workgroups share a CU
constexpr uint64_t kMaxRecords = 0xFFFFFFFFull;  // u32 counters, offsets and ranks
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kHeadBytes = 256;      // the row ticket

int tfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

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
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += stride) words[i] = 0;
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

// The peel of the counts (rs::wave_add) for the cursors: the leader claims a run of positions
// for the lanes that share its key and each takes the one of its rank among them.
__device__ __forceinline__ uint32_t wave_claim(uint32_t *cur, uint32_t key, uint32_t lane) {
  uint32_t pos = 0;
  isim::dev::wave_peel<isim::dev::kPeelAll>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        uint32_t first = 0;
        if ((int)lane == lead) first = atomicAdd(&cur[k0], (uint32_t)__popcll(m));
        first = (uint32_t)__builtin_amdgcn_readlane((int)first, lead);
        if (key == k0) pos = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      },
      [&](uint32_t k) { pos = atomicAdd(&cur[k], 1u); });
  return pos;
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
    const uint32_t sum = v.x + v.y + v.z + v.w;
    uint32_t incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if ((int)lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
      const uint32_t x = s_wave[w];
      before += w < wave ? x : 0u;
      total += x;
    }
    const uint32_t e0 = carry + before + incl - sum;
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
    __syncthreads();  // s_wave is rewritten by the next tile
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
      const uint32_t pos = wave_claim(a.cur, key[u], lane);
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
  uint32_t ppm[kMaxQ];
};

// The select's state of a workgroup's row (radix_select.h); the row's ticket is sel.owner_word,
// which keeps the struct, and with it the kernel's LDS, at its size.
struct SelState {
  rs::State<uint32_t> sel;
  unsigned long long any[kSelWaves];  // per wave: OR of the row's latencies
};

// One digit of a row: per (class, group) the 256-bin histogram of byte `byte`
// over the latencies whose higher bytes equal the group's prefix.  Element i of
// the segment is a 200 below n200, else a 500.
template <bool STAGED>
__device__ __forceinline__ void digit_pass(uint32_t *hist, const SelState &s, const unsigned long long *stage,
                                           const unsigned long long *seg, uint32_t n_row, uint32_t n200, int byte,
                                           uint32_t ng_all, uint32_t ng_200, uint32_t ng_500, uint32_t lane,
                                           uint32_t wave) {
  // a wave takes 64 * kUnroll consecutive latencies per step; the loop bound is wave-uniform
  for (uint64_t base = (uint64_t)wave * (64 * kUnroll); base < n_row; base += (uint64_t)kSelWaves * (64 * kUnroll)) {
    unsigned long long key[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint64_t i = base + u * 64 + lane;
      key[u] = i < n_row ? (STAGED ? stage[i] : seg[i]) : 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint64_t i = base + u * 64 + lane;
      rs::count_key(hist, key[u], i < n_row, byte, i < n200 ? ISIM_Q_200 : ISIM_Q_500, s.sel.gprefix, ng_all, ng_200,
                    ng_500, lane);
    }
  }
}

// The select.  A workgroup claims rows through the ticket until none is left.
// An empty row gets its zeros; otherwise the row's OR gives the top byte and
// from there down each digit is a histogram pass, a resolve (a wave per
// (class, quantile)) and a regroup (radix_select.h).  After byte 0 the
// prefixes are the values.
__global__ __launch_bounds__(kSelThreads) void k_tlq_select(SelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[kClasses * kMaxQ * kBins];
  __shared__ unsigned long long s_stage[kStage];
  __shared__ SelState s;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t n_q = a.n_q, ow = 1u + n_q;
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
    const unsigned long long *seg = a.seg + a.off[2 * row];
    const bool staged = n_row <= kStage;

    unsigned long long any = 0;
    if (staged) {
      for (uint32_t i = t; i < n_row; i += kSelThreads) {
        const unsigned long long v = seg[i];
        s_stage[i] = v;
        any |= v;
      }
    } else {
      for (uint64_t i = t; i < n_row; i += kSelThreads) any |= seg[i];
    }
    for (int d = 32; d; d >>= 1) any |= __shfl_xor(any, d, 64);
    if (lane == 0) s.any[wave] = any;
    if (t < kClasses * kMaxQ) {
      const uint32_t c = t / kMaxQ, i = t % kMaxQ;
      const uint32_t n_c = c == ISIM_Q_ALL ? n_row : c == ISIM_Q_200 ? n200 : n500;
      rs::init(s.sel, c, i, n_q, n_c, a.ppm);
      if (i == 0) out[c * ow] = n_c;
    }
    __syncthreads();
    any = 0;
    for (uint32_t w = 0; w < kSelWaves; ++w) any |= s.any[w];

    for (int byte = rs::top_byte(any); byte >= 0; --byte) {
      const uint32_t ng_all = min(s.sel.ngrp[ISIM_Q_ALL], n_q), ng_200 = min(s.sel.ngrp[ISIM_Q_200], n_q),
                     ng_500 = min(s.sel.ngrp[ISIM_Q_500], n_q);
      for (uint32_t i = t; i < ng_all * kBins; i += kSelThreads) hist[i] = 0;
      for (uint32_t i = t; i < ng_200 * kBins; i += kSelThreads) hist[ISIM_Q_200 * kMaxQ * kBins + i] = 0;
      for (uint32_t i = t; i < ng_500 * kBins; i += kSelThreads) hist[ISIM_Q_500 * kMaxQ * kBins + i] = 0;
      __syncthreads();
      if (staged) digit_pass<true>(hist, s, s_stage, seg, n_row, n200, byte, ng_all, ng_200, ng_500, lane, wave);
      else digit_pass<false>(hist, s, s_stage, seg, n_row, n200, byte, ng_all, ng_200, ng_500, lane, wave);
      __syncthreads();
      for (uint32_t task = wave; task < kClasses * n_q; task += kSelWaves) {  // wave-uniform
        const uint32_t c = task / n_q, i = task % n_q;
        const uint32_t k = s.sel.k[c][i];
        if (!k) continue;  // empty class
        const uint32_t g = min(s.sel.grp[c][i], n_q - 1);
        const u32x4 b = *reinterpret_cast<const u32x4 *>(hist + (c * kMaxQ + g) * kBins + lane * 4);  // they sum to at most n_row
        uint32_t digit, below;
        if (rs::resolve<uint32_t>(b.x, b.y, b.z, b.w, k, lane, digit, below)) rs::take_digit(s.sel, c, i, digit, k, below);
      }
      __syncthreads();
      if (t < kClasses) rs::regroup(s.sel, t, n_q);
      __syncthreads();
    }
    if (t < kClasses * kMaxQ && t % kMaxQ < n_q) {
      const uint32_t c = t / kMaxQ, i = t % kMaxQ;
      out[c * ow + 1 + i] = s.sel.k[c][i] ? s.sel.prefix[c][i] : 0;
    }
  }
}

// everything the three entry points reject alike; the quantile list comes after the parameters
int check_common(const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q, uint64_t n) {
  if (const char *m = isim::tl::params_error(p)) return tfail(m);
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return tfail(m);
  if (n > kMaxRecords) return tfail("n is above 2^32 - 1");
  return ISIM_OK;
}

uint32_t grid_for(uint64_t items, uint64_t per_workgroup, uint32_t cap) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_workgroup - 1) / per_workgroup, 1), cap);
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
    hipLaunchKernelGGL(k_tlq_clear, dim3(grid_for(words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
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
  for (uint32_t i = 0; i < n_q; ++i) sel.ppm[i] = q_ppm[i];

  // the ticket and the counts, contiguous from the workspace's start (every clear is a kernel: §13)
  const uint64_t clear_words = l.cnt / 4 + l.counters;
  hipLaunchKernelGGL(k_tlq_clear, dim3(grid_for(clear_words, kThreads * 4, kMaxGrid)), dim3(kThreads), 0, s,
                     (uint32_t *)ws, clear_words);
  const uint32_t grid = grid_for(n, kThreads * kUnroll, kMaxGrid);
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
