// Per-replica worker-pool DES on gfx950: exact,
// level-synchronous over a batch of N traces.
//
//   arrivals   A[t] = sum of exponential inter-arrival times (Philox draw,
//              integer inverse CDF) — a block scan + a scan of block sums
//   down pass  per queue round: the replica queue of a position's service is
//              FIFO over its arrivals a(v,t) = S(parent,t) + off(v), which are
//              in trace order, so the start times are one
//              max-plus scan over t:  fin_t = max(fin_{t-1}, a_t) + hold,
//              S_t = fin_t - hold (per replica for replicated services).
//              Wide groups: one workgroup per position; narrow groups: chunks
//              of a position chained by a decoupled look-back.  Leaves finish
//              here (F = S + script time, status, duration).
//   up pass    finish groups from the deepest, (position, trace-range)
//              blocks: F = max(S + floor, max_c F(c)) + post, status (own
//              Philox draw; mode B ORs the children's), duration F - a(v,t)
//              into the per-service histogram.
//   finalize   latency F(entry), records and the stats header.
//
// Rows W[position][trace] (and the step-begin rows BK) hold times RELATIVE to
// the arrival of the trace's GROUP, G_t = A[t & ~63] (64 consecutive traces,
// round 3): every value of trace t lies in [A_t - G_t, A_t - G_t + latency_t].
// A queue scan then needs no per-trace arrival time (its keys are G + row +
// off - t hold, the wave's groups' bases are 4 scalars), and within one wave
// the keys relative to the wave's first key fit 32 bits (down1_chunk_n32).
// Narrow rows are u32 (status in bit 31), so a batch whose latencies plus 63
// inter-arrival gaps stay below 2^31 ns (2.1 s) moves 4 B per value; a value that does not fit sets
// the overflow flag, the batch's statistics (staged in the workspace) are
// then dropped and ISIM_ST_DES_RETRY counts it, to be rerun with u64 rows
// (ISIM_DES_FLAG_WIDE; isim_serve_des does that itself).  Bytes per
// (position, trace), narrow: queue pass 4 R + 4 W, up pass 4 R (S) + 4 R
// (arrival row) + 4 R per child + 4 W.
//
// One translation unit in pieces, each included inside namespace isim::dev:
// des_rows.h (row access, change tracking), des_scan.h (wave and block
// scans), des_queue.h (queue pass), des_up.h (up pass, finalize), des_sort.h
// (sort path).  This file keeps the tunables, DesK, the arrivals, status,
// step-begin, zero-hold and commit kernels, the statistics flushes the passes
// share, and the host driver.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>

#include "des_layout.h"
#include "kernel_abi.h"
#include "des_bucket.h"
#include "load_profile.h"

// ---- tunables (tools/build_variant.sh builds a library with one overridden)
#ifndef ISIM_DES_DOWN_THREADS
#define ISIM_DES_DOWN_THREADS 256  // round 3: 512 -> 256 threads per queue-pass workgroup, 36.9 -> 36.4 ms per c5 step
#endif
#ifndef ISIM_DES_DOWN_WAVES
#define ISIM_DES_DOWN_WAVES 6  // waves per SIMD the one-workgroup-per-position pass is compiled for
#endif
#ifndef ISIM_DES_PIPE32_WAVES
#define ISIM_DES_PIPE32_WAVES 6  // waves per SIMD of the 32-bit-key pipelined pass
#endif
#ifndef ISIM_DES_CHAIN_BELOW
#define ISIM_DES_CHAIN_BELOW 256  // positions per launch below which the chained scan is used
#endif
#ifndef ISIM_DES_UP_CB
#define ISIM_DES_UP_CB 2  // round 3: 3 -> 2 (with the 256-thread queue pass: 36.4 -> 36.1 ms per c5 step)
#endif
#ifndef ISIM_DES_UP_WAVES
#define ISIM_DES_UP_WAVES 6  // waves per SIMD the up pass is compiled for (80 VGPRs: no spills)
#endif
#ifndef ISIM_DES_UP32_WAVES
#define ISIM_DES_UP32_WAVES 7  // 69 VGPRs: no spills at 7 (35.6 -> 35.4 ms per c5 step), 8 spill
#endif
#ifndef ISIM_DES_SPLIT_TARGET
#define ISIM_DES_SPLIT_TARGET 8192  // (position x trace-range) blocks per up / step-begin launch
#endif
#ifndef ISIM_DES_MAX_SPLITS
#define ISIM_DES_MAX_SPLITS 256u  // (position x trace-range) blocks per position (uncapped -> 256: 35.5 -> 34.8 ms per c5 step)
#endif
#ifndef ISIM_DES_FIN_BLOCKS
#define ISIM_DES_FIN_BLOCKS 512  // des_finalize workgroups (each flushes the stats header by atomics; 2048 -> 512: -0.05 ms)
#endif

namespace isim {
void *stream_calls_kernel();
namespace dev {

constexpr uint32_t kDesPer = 8;                   // traces per thread in the arrivals
constexpr uint32_t kDesThreads = 1024;
constexpr uint32_t kDesOvfFault = 4u;  // ovf bit: a look-back gave up (the batch fails)
constexpr uint32_t kDesChunk = kDesPer * kDesThreads;  // 8192 traces per arrivals chunk
constexpr uint32_t kPer = 4;                           // consecutive traces per thread in the row passes
constexpr uint32_t kDownChunk = kPer * kDesThreads;    // traces per down-pass chunk
constexpr uint32_t kDesUpThreads = 256;
constexpr uint32_t kDownThreads = ISIM_DES_DOWN_THREADS;  // one-workgroup-per-position queue pass

// the arrival draw (Philox) and the Q24 exponential, shared with load_profile.hip
#include "des_draw.h"

struct ChainState;

struct DesK {
  const DesPos *pos;
  const DesPosExt *ext;
  const DesStep *steps;
  const uint32_t *child;
  const uint32_t *level_pos;  // the positions of the launch (fast queue or finish group)
  const uint32_t *arr_ops;    // BK rows of the launch (step begins)
  void *BK;                   // [steps][ld] row type T
  void *W;                    // [n_pos][ld] row type T: starts S
  void *WF;                   // [n_pos][ld] row type T: finishes F | status (separate rows, so a
                              // fixed-point pass reads last pass's F while S is being rewritten)
  uint64_t *A;                // [N] absolute arrival times
  uint32_t *E;                // [N] per-trace 500 count
  uint64_t *blk;
  uint64_t *stats;            // narrow rows: the staging copy (des_commit)
  uint64_t *table;            // [rows][ISIM_DES_ROW_WORDS] (staged likewise)
  isim_trace_rec *records;
  uint32_t *ovf;              // bit 0: a 32-bit row value reached 2^31; bit 1: no fixed point;
                              // kDesOvfFault: a look-back gave up (the batch is dropped as a fault)
  uint32_t spin_limit;        // look-back polls before that fault (des_spin_limit)
  uint32_t *changed;          // fixed-point passes: set when a stored row value changes (null: no tracking)
  uint32_t quiet;             // fixed-point passes before the last: no statistics
  const uint32_t *stbits;     // own error status of (position, trace): bit t%32 of word [v][t/32]
  uint32_t st_wpr;            // words per status row
  uint64_t N, trace_begin, mean_ns;
  uint64_t ld;                // row stride in traces: N rounded up to 16 (64-B aligned rows)
  uint32_t k0, k1;
  uint32_t n_pos, n_slots;
  uint32_t level_begin, splits;
  uint32_t modeb, n_blk;
  // sort path: the service being queued and its sorted arrivals
  const uint32_t *sort_pos;
  DesSortSvc svc;
  const uint64_t *skeys;
  const uint32_t *svals;
  uint64_t *keys;
  uint32_t *vals;
  // chained down pass
  ChainState *chain;
  uint32_t *chain_ticket;     // this launch's ticket counter
  uint32_t n_chunks;
  // pipelined down pass
  const uint32_t *pipe_dep;   // per level_pos entry: the position it waits on (kDesNone: none)
  uint32_t *prog;             // [n_pos] chunks of a position's start row published (zeroed per pass)
};

#include "des_rows.h"
#include "des_scan.h"

// ---- arrivals: per chunk inclusive prefix of the inter-arrival times
__global__ void __launch_bounds__(kDesThreads) des_arrivals(DesK k) {
  __shared__ uint64_t wtot[kDesThreads / 64];
  const uint64_t base = (uint64_t)blockIdx.x * kDesChunk + (uint64_t)threadIdx.x * kDesPer;
  uint64_t x[kDesPer], s = 0;
#pragma unroll
  for (uint32_t i = 0; i < kDesPer; ++i) {
    const uint64_t t = base + i;
    x[i] = 0;
    if (t < k.N) {
      const uint32_t u = des_draw(k.trace_begin + t, 0u, 0x80000001u, 0, k.k0, k.k1);
      x[i] = (k.mean_ns * des_exp_q24(u)) >> 24;
    }
    s += x[i];
  }
  uint64_t total;
  uint64_t run = block_scan_add(s, wtot, total) - s;
#pragma unroll
  for (uint32_t i = 0; i < kDesPer; ++i) {
    run += x[i];
    if (base + i < k.N) k.A[base + i] = run;
  }
  if (threadIdx.x == 0) k.blk[blockIdx.x] = total;
}

// exclusive scan of the chunk totals (one workgroup)
__global__ void __launch_bounds__(kDesThreads) des_scan_blocks(DesK k) {
  __shared__ uint64_t wtot[kDesThreads / 64];
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < k.n_blk; b0 += kDesThreads) {
    const uint32_t b = b0 + threadIdx.x;
    const uint64_t v = b < k.n_blk ? k.blk[b] : 0;
    uint64_t total;
    const uint64_t inc = block_scan_add(v, wtot, total);
    if (b < k.n_blk) k.blk[b] = carry + inc - v;
    carry += total;
  }
}

__global__ void __launch_bounds__(kDesThreads) des_add_blocks(DesK k) {
  const uint64_t off = k.blk[blockIdx.x];
  const uint64_t base = (uint64_t)blockIdx.x * kDesChunk;
  for (uint32_t i = threadIdx.x; i < kDesChunk; i += kDesThreads)
    if (base + i < k.N) k.A[base + i] += off;
}

// hist[bin[i]] += 1 for the (up to) 4 bins of every lane (kNoBin: none).
// The durations of one position mostly share a bin: the wave counts the bins
// equal to its first lane's first bin with ballots and adds them with one LDS
// atomic; the rest go one atomic each.  Call with the wave converged.
constexpr uint32_t kNoBin = 0xFFFFFFFFu;
// FULL: every bin is set (whole quads of traces below N)
template <bool FULL = false>
__device__ __forceinline__ void hist_add4(uint32_t *hist, const uint32_t (&bin)[4]) {
  const uint32_t first =
      FULL ? bin[0] : bin[0] != kNoBin ? bin[0] : bin[1] != kNoBin ? bin[1] : bin[2] != kNoBin ? bin[2] : bin[3];
  const uint64_t any = __ballot(first != kNoBin);
  if (!any) return;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)__builtin_ctzll(any));
  uint32_t n = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    n += (uint32_t)__builtin_popcountll(__ballot(bin[i] == b0));
    if ((FULL || bin[i] != kNoBin) && bin[i] != b0) atomicAdd(&hist[bin[i]], 1u);
  }
  if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(any)) atomicAdd(&hist[b0], n);
}

// m = 2 m + (this lane in mask): one v_addc_co_u32 with the mask as carry-in
__device__ __forceinline__ void des_shift_in(uint32_t &m, uint64_t mask) {
  uint64_t co;
  asm("v_addc_co_u32 %0, %1, %0, %0, %2" : "+v"(m), "=s"(co) : "s"(mask));
}

// own error statuses of traces [base, base+4) of position v (base % 4 == 0),
// bit i.  The status pass zeroes the bits past N inside a row, but a partial
// last chunk also asks for quads far past N — up to a chunk beyond the row's
// 16-word padding, i.e. into the NEXT position's row.  Those quads read
// nothing (round 3: this was the cause of the "hoisted 500-count atomics gave
// wrong batches" variant of round 2 — without the per-trace N guard its
// atomics counted the next row's bits into E[t >= N], past the end of E).
__device__ __forceinline__ uint32_t des_status4(const DesK &k, uint32_t v, uint64_t base) {
  if (base >= k.N) return 0u;
  return (k.stbits[(uint64_t)v * k.st_wpr + (base >> 5)] >> (base & 31u)) & 0xFu;
}

// ---- status pass: the own error status of every (position, trace).  The
// four positions 4g..4g+3 share Philox block (t, g, 0, 0) (word j for
// position 4g+j, as in the walks), so one block per (group, trace) instead of
// one per (position, trace).  One thread: a group x 32 consecutive traces.
__global__ void __launch_bounds__(256) des_status(DesK k) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t ng = (k.n_pos + 3) / 4;
  const uint64_t g = tid / k.st_wpr, w = tid - g * k.st_wpr;
  if (g >= ng) return;
  uint32_t thr[4], always[4], live[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t v = (uint32_t)g * 4 + j;
    live[j] = v < k.n_pos;
    const DesPos &P = k.pos[live[j] ? v : 0];
    thr[j] = live[j] ? P.thr : 0u;
    always[j] = live[j] && (P.flags & kDesFlagAlways);
  }
  uint32_t bits[4] = {0, 0, 0, 0};
  const uint32_t any = thr[0] | thr[1] | thr[2] | thr[3];
  auto put = [&](const uint32_t (&c)[4], uint32_t b) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) bits[j] |= (uint32_t)(always[j] || (thr[j] && c[j] < thr[j])) << b;
  };
  // whole waves of one group and one trace-id high word (the usual case):
  // counter words 1-3 are wave-uniform, so rounds 1-2 fold into scalar math
  // (as walk.hip philox_lockstep), and each trace's bit is shifted in from
  // the compare's lane mask (one v_addc_co_u32)
  const uint64_t t0 = k.trace_begin + w * 32;
  const uint32_t gu = __builtin_amdgcn_readfirstlane((uint32_t)g);
  const uint32_t hiu = __builtin_amdgcn_readfirstlane((uint32_t)(t0 >> 32));
  const bool lane_ok = any && w * 32 + 32 <= k.N && (uint32_t)g == gu && (uint32_t)(t0 >> 32) == hiu &&
                       (uint32_t)((t0 + 31) >> 32) == hiu;
  if (__ballot(!lane_ok) == 0) {
    uint32_t lim[4], en[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {  // wave-uniform: bit = en && c <= lim
      const uint32_t a = __builtin_amdgcn_readfirstlane(always[j]), t = __builtin_amdgcn_readfirstlane(thr[j]);
      en[j] = a | (t != 0u);
      lim[j] = a ? 0xFFFFFFFFu : t - 1u;
    }
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    const uint64_t q1 = (uint64_t)M1 * gu;                           // scalar
    const uint32_t u0 = (uint32_t)(q1 >> 32) ^ hiu ^ k.k0;           // uniform
    const uint64_t q0 = (uint64_t)M0 * u0;                           // scalar (round 2)
    uint32_t uk0 = (uint32_t)q1 ^ (k.k0 + W0), uk1 = (uint32_t)(q0 >> 32) ^ (k.k1 + W1);
    asm volatile("" : "+s"(uk0), "+s"(uk1));
    uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    for (int b = 15; b >= 0; --b) {  // traces b and b + 16, shifted in from the top bit down
      uint32_t c[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t tl = (uint32_t)t0 + (uint32_t)b + 16u * u;
        const uint64_t p0 = (uint64_t)M0 * tl;
        const uint64_t p1 = (uint64_t)M1 * ((uint32_t)(p0 >> 32) ^ k.k1);
        c[u][0] = (uint32_t)(p1 >> 32) ^ uk0;
        c[u][1] = (uint32_t)p1;
        c[u][2] = (uint32_t)p0 ^ uk1;
        c[u][3] = (uint32_t)q0;
      }
      uint32_t k0 = k.k0 + 2u * W0, k1 = k.k1 + 2u * W1;
#pragma unroll
      for (int r = 2; r < 10; ++r) {
        asm volatile("" : "+s"(k0), "+s"(k1));
        des_round(c[0], k0, k1);
        des_round(c[1], k0, k1);
        k0 += W0;
        k1 += W1;
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        des_shift_in(lo[j], en[j] ? __ballot(c[0][j] <= lim[j]) : 0ull);
        des_shift_in(hi[j], en[j] ? __ballot(c[1][j] <= lim[j]) : 0ull);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) bits[j] = lo[j] | (hi[j] << 16);
  } else if (any && w * 32 + 32 <= k.N) {
    // two independent Philox chains per step (ILP)
    for (uint32_t b = 0; b < 16; ++b) {
      const uint64_t t0 = k.trace_begin + w * 32 + b, t1 = t0 + 16;
      uint32_t c0[4] = {(uint32_t)t0, (uint32_t)(t0 >> 32), (uint32_t)g, 0u};
      uint32_t c1[4] = {(uint32_t)t1, (uint32_t)(t1 >> 32), (uint32_t)g, 0u};
      uint32_t k0 = k.k0, k1 = k.k1;
#pragma unroll
      for (int r = 0; r < 10; ++r) {
        des_round(c0, k0, k1);
        des_round(c1, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
      }
      put(c0, b);
      put(c1, b + 16);
    }
  } else {
    for (uint32_t b = 0; b < 32; ++b) {
      const uint64_t t = w * 32 + b;
      if (t >= k.N) break;
      if (any) {
        uint32_t c[4] = {(uint32_t)(k.trace_begin + t), (uint32_t)((k.trace_begin + t) >> 32), (uint32_t)g, 0u};
        des_philox(c, k.k0, k.k1);
        put(c, b);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) bits[j] |= always[j] << b;
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (live[j]) const_cast<uint32_t *>(k.stbits)[(g * 4 + j) * k.st_wpr + w] = bits[j];
}

// per-service duration statistics of a workgroup: LDS histogram + sums -> the
// service's table row, 500s -> the call site's callee-500 counter
template <uint32_t NT>
__device__ __forceinline__ void des_flush_durations(const DesK &k, const DesPos &P, const uint32_t *hist,
                                                    uint64_t d0, uint64_t d1, uint64_t n5, uint64_t *red) {
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) {
    d0 += __shfl_xor(d0, d, 64);
    d1 += __shfl_xor(d1, d, 64);
    n5 += __shfl_xor(n5, d, 64);
  }
  constexpr uint32_t W = NT / 64;
  if ((threadIdx.x & 63u) == 0) {
    red[threadIdx.x >> 6] = d0;
    red[W + (threadIdx.x >> 6)] = d1;
    red[2 * W + (threadIdx.x >> 6)] = n5;
  }
  __syncthreads();
  unsigned long long *trow = (unsigned long long *)(k.table + (uint64_t)P.row * ISIM_DES_ROW_WORDS);
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += NT)
    if (hist[i]) atomicAdd(trow + i, (unsigned long long)hist[i]);
  if (threadIdx.x == 0) {
    uint64_t s0 = 0, s1 = 0, e = 0;
#pragma unroll 2
    for (uint32_t i = 0; i < W; ++i) {
      s0 += red[i];
      s1 += red[W + i];
      e += red[2 * W + i];
    }
    if (s0) atomicAdd(trow + 2 * ISIM_N_PROM, (unsigned long long)s0);
    if (s1) atomicAdd(trow + 2 * ISIM_N_PROM + 1, (unsigned long long)s1);
    if (e && P.slot != kSlotRoot)
      atomicAdd((unsigned long long *)(k.stats + ISIM_ST_SITES + k.n_slots + P.slot), (unsigned long long)e);
  }
}

// queue statistics of a workgroup -> the service's table row
template <uint32_t NT>
__device__ __forceinline__ void des_flush_waits(const DesK &k, uint32_t trow_idx, uint64_t wsum, uint64_t wmax,
                                                uint64_t count, uint64_t hold_sum, uint64_t *red) {
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) {
    wsum += __shfl_xor(wsum, d, 64);
    const uint64_t o = __shfl_xor(wmax, d, 64);
    wmax = o > wmax ? o : wmax;
  }
  if ((threadIdx.x & 63u) == 0) {
    red[threadIdx.x >> 6] = wsum;
    red[NT / 64 + (threadIdx.x >> 6)] = wmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0, m = 0;
#pragma unroll 2
    for (uint32_t i = 0; i < NT / 64; ++i) {
      s += red[i];
      m = red[NT / 64 + i] > m ? red[NT / 64 + i] : m;
    }
    unsigned long long *trow = (unsigned long long *)(k.table + (uint64_t)trow_idx * ISIM_DES_ROW_WORDS);
    if (count) atomicAdd(trow + ISIM_DES_COUNT, (unsigned long long)count);
    if (hold_sum) atomicAdd(trow + ISIM_DES_SUM_HOLD, (unsigned long long)hold_sum);
    if (s) atomicAdd(trow + ISIM_DES_SUM_WAIT, (unsigned long long)s);
    if (m) atomicMax(trow + ISIM_DES_MAX_WAIT, (unsigned long long)m);
  }
}

#include "des_queue.h"
#include "des_up.h"
#include "des_sort.h"

// ---- step begins (calls after calls): BK rows of one round
template <typename T>
__global__ void __launch_bounds__(kDesUpThreads) des_arrive(DesK k) {
  const uint32_t b = k.arr_ops[k.level_begin + blockIdx.y];
  const DesStep st = k.steps[b];
  const uint64_t N = k.N;
  const uint64_t tb = N * blockIdx.x / k.splits, te = N * (blockIdx.x + 1) / k.splits;
  T *out = row<T>(k.BK, k.ld, b);
  bool bad = false;
  for (uint64_t t = tb + threadIdx.x; t < te; t += kDesUpThreads) {
    uint64_t v;
    if (st.prev == kDesNone) {
      v = row<T>(k.W, k.ld, st.pos)[t];  // the position's start
    } else {
      v = (uint64_t)row<T>(k.BK, k.ld, st.prev)[t] + st.smax;
      for (uint32_t j = 0; j < st.child_cnt; ++j) {
        const uint64_t f = row<T>(k.WF, k.ld, k.child[st.child_off + j])[t] & Row<T>::kMask;
        v = f > v ? f : v;
      }
    }
    v += st.add;
    bad |= !Row<T>::fits(v);
    track1<T>(k, out + t, (T)v);
    out[t] = (T)v;
  }
  flag_overflow(k, bad);
}

// ---- zero-hold services: no queue, start = arrival (relative), per
// (position, trace-range) block; the queue statistics: N invocations, no wait
template <typename T>
__global__ void __launch_bounds__(kDesUpThreads) des_zero(DesK k) {
  const uint32_t v = k.level_pos[k.level_begin + blockIdx.y];
  const DesPos P = k.pos[v];
  const uint64_t N = k.N;
  const uint64_t tb = N * blockIdx.x / k.splits, te = N * (blockIdx.x + 1) / k.splits;
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  T *out = row<T>(k.W, k.ld, v);
  bool bad = false;
  for (uint64_t t = tb + threadIdx.x; t < te; t += kDesUpThreads) {
    const uint64_t a = par ? (uint64_t)par[t] + off : k.A[t] - des_gbase(k, t);
    bad |= !Row<T>::fits(a);
    out[t] = (T)a;
  }
  flag_overflow(k, bad);
  if (threadIdx.x == 0 && te > tb && !k.quiet)
    atomicAdd((unsigned long long *)(k.table + (uint64_t)P.row * ISIM_DES_ROW_WORDS + ISIM_DES_COUNT),
              (unsigned long long)(te - tb));
}

// ---- narrow rows: merge the staged statistics into the caller's buffers,
// or count the batch in ISIM_ST_DES_RETRY when a value overflowed
__global__ void __launch_bounds__(256) des_commit(const uint64_t *__restrict__ stage, uint64_t *stats,
                                                  uint64_t *table, uint64_t stats_words, uint64_t table_words,
                                                  const uint32_t *ovf) {
  if (const uint32_t o = *ovf) {
    // dropped: a retry (narrow rows overflowed, no fixed point) or a fault
    // (a look-back gave up: counted in the word's high half, an error)
    if (blockIdx.x == 0 && threadIdx.x == 0)
      atomicAdd((unsigned long long *)(stats + ISIM_ST_DES_RETRY),
                (unsigned long long)((o & kDesOvfFault) ? kDesFaultUnit : 1ull));
    return;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < stats_words + table_words;
       i += (uint64_t)gridDim.x * 256) {
    const uint64_t x = stage[i];
    if (!x) continue;
    if (i < stats_words) {
      unsigned long long *p = (unsigned long long *)(stats + i);
      if (i == ISIM_ST_NOT_MIN_LATENCY || i == ISIM_ST_MAX_LATENCY) atomicMax(p, (unsigned long long)x);
      else atomicAdd(p, (unsigned long long)x);
    } else {
      const uint64_t j = i - stats_words;
      unsigned long long *p = (unsigned long long *)(table + j);
      if (j % ISIM_DES_ROW_WORDS == ISIM_DES_MAX_WAIT) atomicMax(p, (unsigned long long)x);
      else atomicAdd(p, (unsigned long long)x);
    }
  }
}

}  // namespace dev

static size_t sort_temp_bytes(uint64_t m) {
  size_t bytes = 0;
  if (m == 0) return 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                  (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, 0, 64);
  return bytes;
}

static_assert(kDesArrChunk == dev::kDesChunk && kDesDownChunk == dev::kDownChunk, "des_layout.h chunk sizes");

uint64_t des_workspace_bytes(const DesPlan &plan, uint64_t n, uint64_t stats_words, uint64_t table_rows) {
  Arena sizing;
  DesBufs b;
  des_layout(sizing, b, plan, n, stats_words, table_rows, sort_temp_bytes((uint64_t)plan.max_sort_pos * n));
  return sizing.bytes();
}

void des_carve(DesLaunch &L, void *workspace) {
  Arena carving(workspace);
  des_layout(carving, L.ws, *L.plan, L.n_traces, L.stats_words, L.table_rows,
             sort_temp_bytes((uint64_t)L.plan->max_sort_pos * L.n_traces));
}

// The rounds of one batch with row type T: step begins,
// queues (fast: in place; sort path: radix sort first), finishes.
template <typename T>
static int des_rounds(const DesLaunch &L, dev::DesK k, hipStream_t stream) {
  using namespace dev;
  const DesPlan &pl = *L.plan;
  const DesBufs &B = L.ws;
  const size_t sort_tmp_bytes = sort_temp_bytes((uint64_t)pl.max_sort_pos * L.n_traces);
  k.sort_pos = L.d_sort_pos;
  // (position or row) x trace-range blocks: enough to fill the chip, >= 256 traces each
  // and at most ISIM_DES_MAX_SPLITS per position: every block flushes its
  // histogram and sums into the position's one table row by memory-side
  // atomics, which serialise per address (a one-position level in 4,096
  // blocks: ~90 us of atomics for 25 MB of rows)
  auto splits_for = [&](uint32_t width) {
    uint64_t sp = (ISIM_DES_SPLIT_TARGET + width - 1) / width;
    const uint64_t cap = (L.n_traces + 255) / 256;
    sp = sp < cap ? sp : cap;
    sp = sp < ISIM_DES_MAX_SPLITS ? sp : ISIM_DES_MAX_SPLITS;
    return (uint32_t)(sp ? sp : 1);
  };
  size_t seg = 0;
  uint32_t piped_to = 0;  // rounds below this one had their queues in a pipelined launch
  for (uint32_t r = 0; r < pl.rounds(); ++r) {
    if (seg < pl.pipe.size() && pl.pipe[seg].r0 == r) {
      // the single-replica queues of rounds [r0, r1] in one launch (no step
      // begins, zero-hold, sort-path or replicated queues in them; finishes
      // only in r1)
      const DesPlan::PipeSeg &sg = pl.pipe[seg++];
      DesK kp = k;
      kp.level_pos = L.d_pipe;
      kp.pipe_dep = L.d_pipe + pl.pipe_pos.size();
      kp.level_begin = sg.off;
      kp.chain_ticket = B.tickets + 4 * r + 2;
      bool n32 = false;
      if constexpr (sizeof(T) == 4) {
        n32 = pl.pipe_n32;
        if (n32) hipLaunchKernelGGL((des_down_pipe<T, true>), dim3(sg.cnt), dim3(kDownThreads), 0, stream, kp);
      }
      if (!n32) hipLaunchKernelGGL((des_down_pipe<T, false>), dim3(sg.cnt), dim3(kDownThreads), 0, stream, kp);
      piped_to = sg.r1 + 1;
    }
    if (r >= piped_to) {
      // 1. step begins (calls after calls)
      const uint32_t na = pl.arr_off[r + 1] - pl.arr_off[r];
      if (na) {
        k.level_begin = pl.arr_off[r];
        k.splits = splits_for(na);
        hipLaunchKernelGGL(des_arrive<T>, dim3(k.splits, na), dim3(kDesUpThreads), 0, stream, k);
      }
      // 2. queues.  Zero-hold services: start = arrival.
      const uint32_t nz = pl.zero_off[r + 1] - pl.zero_off[r];
      if (nz) {
        k.level_pos = L.d_zero_pos;
        k.level_begin = pl.zero_off[r];
        k.splits = splits_for(nz);
        hipLaunchKernelGGL(des_zero<T>, dim3(k.splits, nz), dim3(kDesUpThreads), 0, stream, k);
      }
      //    Fast positions, in the plan's variant order (des_plan.cpp):
      //    [single fused | single | replicated fused | replicated].
      //    Single-replica positions (fused leaves or not) share one launch:
      //    groups narrower than the chip take the chained scan (many
      //    workgroups per position), wide groups one workgroup per position.
      k.level_pos = L.d_fast_pos;
      const uint32_t *fs = &pl.fast_split[5 * r];
      if (fs[2] > fs[0]) {
        k.level_begin = fs[0];
        if (fs[2] - fs[0] < ISIM_DES_CHAIN_BELOW) {
          k.chain_ticket = B.tickets + 4 * r;
          hipLaunchKernelGGL(des_down_chain_mix<T>, dim3((fs[2] - fs[0]) * k.n_chunks), dim3(kDesThreads), 0, stream,
                             k);
        } else {
          hipLaunchKernelGGL(des_down_mix<T>, dim3(fs[2] - fs[0]), dim3(kDownThreads), 0, stream, k);
        }
      }
      //    Replicated services: one workgroup per position, fused leaves and others apart.
      if (fs[3] > fs[2]) {
        k.level_begin = fs[2];
        hipLaunchKernelGGL((des_down<T, true>), dim3(fs[3] - fs[2]), dim3(kDownThreads), 0, stream, k);
      }
      if (fs[4] > fs[3]) {
        k.level_begin = fs[3];
        hipLaunchKernelGGL((des_down<T, false>), dim3(fs[4] - fs[3]), dim3(kDownThreads), 0, stream, k);
      }
      for (uint32_t si = pl.sorted_off[r]; si < pl.sorted_off[r + 1]; ++si) {
        k.svc = pl.sorted[si];
        const uint64_t m = (uint64_t)k.svc.pos_cnt * L.n_traces;
        k.keys = B.keys_a;
        k.vals = B.vals_a;
        uint64_t g = (m + kDesUpThreads - 1) / kDesUpThreads;
        g = g < 4096 ? g : 4096;
        hipLaunchKernelGGL(des_sort_keys<T>, dim3((uint32_t)g), dim3(kDesUpThreads), 0, stream, k);
        size_t tb = sort_tmp_bytes;
        if (rocprim::radix_sort_pairs(B.sort_tmp, tb, B.keys_a, B.keys_b, B.vals_a, B.vals_b, (size_t)m, 0, 64,
                                      stream) != hipSuccess)
          return 1;
        k.skeys = B.keys_b;
        k.svals = B.vals_b;
        hipLaunchKernelGGL(des_down_sorted<T>, dim3(1), dim3(kDesThreads), 0, stream, k);
      }
    }
    // 3. finishes, deepest group first
    k.level_pos = L.d_fin_pos;
    for (uint32_t gi = pl.fin_round_off[r]; gi < pl.fin_round_off[r + 1]; ++gi) {
      const uint32_t width = pl.fin_off[gi + 1] - pl.fin_off[gi];
      k.level_begin = pl.fin_off[gi];
      k.splits = splits_for(width);
      bool n32 = false;
      if constexpr (sizeof(T) == 4) {
        n32 = pl.up_n32;
        if (n32) hipLaunchKernelGGL((des_up<T, true>), dim3(k.splits, width), dim3(kDesUpThreads), 0, stream, k);
      }
      if (!n32) hipLaunchKernelGGL((des_up<T, false>), dim3(k.splits, width), dim3(kDesUpThreads), 0, stream, k);
    }
  }
  return 0;
}

// Host launcher: the whole DES of one batch on `stream` (no allocation; no
// host synchronisation unless the schedule is cyclic: its fixed-point passes
// read one flag per pass).
static std::atomic<uint32_t> g_spin_limit{kDesSpinLimit};
uint32_t des_spin_limit() { return g_spin_limit.load(std::memory_order_relaxed); }
void des_set_spin_limit(uint32_t polls) { g_spin_limit.store(polls, std::memory_order_relaxed); }

// A[t] of the batch k describes (N, trace_begin, mean_ns, k0, k1, A, blk,
// n_blk): the chunk prefixes, the scan of the chunk sums, the offsets added
static void launch_arrivals(const dev::DesK &k, hipStream_t stream) {
  using namespace dev;
  hipLaunchKernelGGL(des_arrivals, dim3(k.n_blk), dim3(kDesThreads), 0, stream, k);
  hipLaunchKernelGGL(des_scan_blocks, dim3(1), dim3(kDesThreads), 0, stream, k);
  hipLaunchKernelGGL(des_add_blocks, dim3(k.n_blk), dim3(kDesThreads), 0, stream, k);
}

uint64_t des_arrivals_blocks(uint64_t n) { return (n + dev::kDesChunk - 1) / dev::kDesChunk; }

int des_arrivals_launch(uint64_t seed, uint64_t mean_ns, uint64_t trace_begin, uint64_t n, uint64_t *d_arrivals,
                        uint64_t *d_blk, void *stream) {
  dev::DesK k{};
  k.A = d_arrivals;
  k.blk = d_blk;
  k.N = n;
  k.trace_begin = trace_begin;
  k.mean_ns = mean_ns;
  k.k0 = (uint32_t)seed;
  k.k1 = (uint32_t)(seed >> 32);
  k.n_blk = (uint32_t)des_arrivals_blocks(n);
  launch_arrivals(k, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int des_launch(const DesLaunch &L, void *stream_) {
  using namespace dev;
  hipStream_t stream = (hipStream_t)stream_;
  const bool narrow = !L.wide;
  const uint64_t table_words = (uint64_t)L.table_rows * ISIM_DES_ROW_WORDS;
  DesK k{};
  k.pos = (const DesPos *)L.d_pos;
  k.ext = (const DesPosExt *)L.d_ext;
  k.steps = (const DesStep *)L.d_steps;
  k.child = L.d_child;
  k.arr_ops = L.d_arr_ops;
  const DesBufs &B = L.ws;
  k.W = B.W;
  k.WF = B.WF;
  k.BK = B.BK;
  k.A = B.A;
  k.E = B.E;
  k.blk = B.blk;
  k.ovf = B.ovf;
  k.spin_limit = des_spin_limit();
  k.stbits = B.stbits;
  k.st_wpr = (uint32_t)des_status_wpr(L.n_traces);
  // statistics go to the staging copy, merged by des_commit unless the batch
  // is dropped (a 32-bit row overflowed, or no fixed point)
  k.stats = B.stage;
  k.table = B.stage + L.stats_words;
  k.records = L.d_records;
  k.N = L.n_traces;
  k.ld = des_row_ld(L.n_traces);
  k.trace_begin = L.trace_begin;
  k.mean_ns = L.mean_ns;
  k.k0 = (uint32_t)L.seed;
  k.k1 = (uint32_t)(L.seed >> 32);
  k.n_pos = L.n_pos;
  k.n_slots = L.n_slots;
  k.modeb = L.modeb;
  k.n_blk = (uint32_t)((L.n_traces + kDesChunk - 1) / kDesChunk);
  k.n_chunks = (uint32_t)((L.n_traces + kDownChunk - 1) / kDownChunk);
  k.prog = B.prog;
  k.chain = B.chain;
  if (hipMemsetAsync(B.E, 0, L.n_traces * sizeof(uint32_t), stream) != hipSuccess) return 1;
  if (hipMemsetAsync(B.ovf, 0, 8, stream) != hipSuccess) return 1;  // overflow flag + changed flag
  if (hipMemsetAsync(B.stage, 0, (L.stats_words + table_words) * 8, stream) != hipSuccess) return 1;
  if (L.profile) {
    if (lp::arrivals_launch(L.seed, *L.profile, L.trace_begin, L.n_traces, B.A, B.blk, stream)) return 1;
  } else {
    launch_arrivals(k, stream);
  }
  {
    const uint64_t threads = (uint64_t)((L.n_pos + 3) / 4) * k.st_wpr;
    hipLaunchKernelGGL(des_status, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, k);
  }
  auto pass = [&](const DesK &kk) -> int {
    if (hipMemsetAsync(B.tickets, 0, B.pass_zero_bytes, stream) != hipSuccess) return 1;
    return narrow ? des_rounds<uint32_t>(L, kk, stream) : des_rounds<uint64_t>(L, kk, stream);
  };
  if (L.plan->cyclic) {
    // fixed point: back-edge rows start at 0 (a lower bound of every
    // relative time); quiet passes until no stored value changes, then the
    // pass that records the statistics
    const uint64_t rb = narrow ? 4 : 8;
    if (hipMemsetAsync(B.W, 0, (uint64_t)L.n_pos * k.ld * rb, stream) != hipSuccess ||
        hipMemsetAsync(B.WF, 0, (uint64_t)L.n_pos * k.ld * rb, stream) != hipSuccess ||
        hipMemsetAsync(B.BK, 0, (uint64_t)L.plan->steps.size() * k.ld * rb, stream) != hipSuccess)
      return 1;
    DesK kq = k;
    kq.quiet = 1;
    kq.changed = B.changed;
    uint32_t p = 0;
    for (; p < kMaxPasses; ++p) {
      if (hipMemsetAsync(kq.changed, 0, 4, stream) != hipSuccess) return 1;
      if (pass(kq)) return 1;
      // the overflow word and, behind it, the changed flag (des_layout.h): a batch
      // that is dropped anyway (a 32-bit row value reached 2^31, a look-back
      // fault) has no fixed point to wait for — its rows may never settle
      uint32_t flags[2] = {0, 1};
      if (hipMemcpyAsync(flags, B.ovf, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess)
        return 1;
      if (flags[0] || !flags[1]) break;
    }
    if (p == kMaxPasses) {
      static const uint32_t no_fixed_point = 2;
      if (hipMemcpyAsync(B.ovf, &no_fixed_point, 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess)
        return 1;
    }
  }
  if (pass(k)) return 1;
  uint64_t fin_blocks = (L.n_traces + kDesUpThreads - 1) / kDesUpThreads;
  fin_blocks = fin_blocks < ISIM_DES_FIN_BLOCKS ? fin_blocks : ISIM_DES_FIN_BLOCKS;
  if (narrow) hipLaunchKernelGGL(des_finalize<uint32_t>, dim3((uint32_t)fin_blocks), dim3(kDesUpThreads), 0, stream, k);
  else hipLaunchKernelGGL(des_finalize<uint64_t>, dim3((uint32_t)fin_blocks), dim3(kDesUpThreads), 0, stream, k);
  if (L.n_slots > 0) {  // executed calls: every trace makes mult[slot] calls through each site
    uint32_t n_slots = L.n_slots;
    uint64_t n = L.n_traces;
    const uint32_t *mult = L.d_mult;
    uint64_t *st = k.stats;
    uint32_t *stage = nullptr;  // the DES counts its 500s itself (no staged walk flush)
    void *args[] = {&mult, &n_slots, &n, &st, &stage};
    if (hipLaunchKernel(stream_calls_kernel(), dim3((n_slots + 255) / 256), dim3(256), args, 0, stream) !=
        hipSuccess)
      return 1;
  }
  uint64_t g = (L.stats_words + table_words + 255) / 256;
  g = g < 1024 ? g : 1024;
  hipLaunchKernelGGL(des_commit, dim3((uint32_t)(g ? g : 1)), dim3(256), 0, stream, B.stage, L.d_stats, L.d_table,
                     L.stats_words, table_words, (const uint32_t *)B.ovf);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace isim
