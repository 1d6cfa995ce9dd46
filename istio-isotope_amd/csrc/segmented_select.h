// The drivers of the MSD radix select, device only: the loops
// that run radix_select.h's steps over a segment of u64 keys whose first n200
// elements are 200s and the rest 500s (quantile.hip's batch takes the class
// from the record).  Two forms.  select_segment: one workgroup, u32 bins in
// LDS, every digit in a loop (a timeline row, a short service).  setup,
// hist_pass and resolve_pass: a launch each, bins in global memory (the batch
// with u64 counts, a long service's chunks with u32).  The callers own the
// kernels, the tickets and the early exits; every barrier in here is reached by
// the whole workgroup or by none of it.
#pragma once

#include <algorithm>

#include "radix_select.h"

namespace isim {
namespace rs {

constexpr uint32_t kUnroll = 4;  // keys per lane in flight
constexpr uint32_t kSelThreads = 512;
constexpr uint32_t kSelWaves = kSelThreads / 64;
constexpr uint32_t kHistThreads = 512;  // three workgroups of 48 KB LDS per CU: 24 waves
constexpr uint32_t kResolveThreads = 64 * kMaxQ;
// keys of a segment kept in LDS (28 KB): with the 48 KB of bins two workgroups share a CU
constexpr uint32_t kStage = 3584;
static_assert(kStage == ISIM_SVQ_STAGE, "include/isim.h states the same number");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the quantile list, by value in the kernel arguments
struct Ppm {
  uint32_t v[kMaxQ];
};
inline Ppm ppm_of(const uint32_t *q_ppm, uint32_t n_q) {
  Ppm p{};
  for (uint32_t i = 0; i < n_q; ++i) p.v[i] = q_ppm[i];
  return p;
}

inline uint32_t grid_for(uint64_t items, uint64_t per_workgroup, uint32_t cap) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + per_workgroup - 1) / per_workgroup, 1), cap);
}

// Every clear is a kernel, so a captured call is a chain of kernel nodes only; this is their body.
template <uint32_t THREADS, typename W>
__device__ __forceinline__ void clear_words(W *words, uint64_t n_words) {
  const uint64_t stride = (uint64_t)gridDim.x * THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n_words; i += stride) words[i] = 0;
}

// Exclusive scan of v over a workgroup of THREADS (a shuffle scan per wave, the wave totals through
// s_wave[THREADS / 64]); total: the sum.
template <uint32_t THREADS>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *s_wave, uint32_t lane, uint32_t wave, uint32_t &total) {
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if ((int)lane >= d) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t w = 0; w < THREADS / 64; ++w) {
    const uint32_t x = s_wave[w];
    before += w < wave ? x : 0u;
    total += x;
  }
  __syncthreads();  // s_wave is rewritten by the next scan
  return before + incl - v;
}

// ---- the steps both forms share

// the first threads of the workgroup: ranks and groups from the three class counts (of the ranks' width), and
// the counts into the cell
template <typename Rank>
__device__ __forceinline__ void setup(State<Rank> &st, uint32_t t, uint32_t n_q, Rank n_all, Rank n_200, Rank n_500,
                                      const Ppm &ppm, unsigned long long *cell) {
  if (t < kClasses * kMaxQ) {
    const uint32_t c = t / kMaxQ, i = t % kMaxQ;
    const Rank n_c = c == ISIM_Q_ALL ? n_all : c == ISIM_Q_200 ? n_200 : n_500;
    init(st, c, i, n_q, n_c, ppm.v);
    if (i == 0) cell[c * (1 + n_q)] = n_c;
  }
}

// after byte 0 the prefixes are the values
template <typename Rank>
__device__ __forceinline__ void write_values(const State<Rank> &st, uint32_t t, uint32_t n_q, unsigned long long *cell) {
  if (t < kClasses * kMaxQ && t % kMaxQ < n_q) {
    const uint32_t c = t / kMaxQ, i = t % kMaxQ;
    cell[c * (1 + n_q) + 1 + i] = st.k[c][i] ? st.prefix[c][i] : 0;
  }
}

// the live bins of hist[kClasses][kMaxQ][kBins]
template <uint32_t THREADS>
__device__ __forceinline__ void zero_bins(uint32_t *hist, const uint32_t (&ng)[kClasses], uint32_t t) {
  for (uint32_t c = 0; c < kClasses; ++c)
    for (uint32_t i = t; i < ng[c] * kBins; i += THREADS) hist[c * kMaxQ * kBins + i] = 0;
}

struct Key {
  uint64_t key;
  uint32_t cls;  // ISIM_Q_200 or ISIM_Q_500
};
// element i of a segment: a 200 below n200, else a 500
__device__ __forceinline__ uint32_t seg_class(uint64_t i, uint32_t n200) { return i < n200 ? ISIM_Q_200 : ISIM_Q_500; }

// One wave's share of a digit pass: 64 * kUnroll consecutive elements from `first`, then every `step`, below
// `end` (wave-uniform, as is the loop bound).  key_at(i, live) gives element i's Key (live: i < end).  AHEAD:
// all kUnroll loads are issued before the first count (keys in global memory); else a key is read where it is
// counted (keys in LDS).
template <typename Idx, bool AHEAD, typename KeyAt>
__device__ __forceinline__ void count_range(uint32_t *hist, const uint64_t (&gprefix)[kClasses][kMaxQ],
                                            const uint32_t (&ng)[kClasses], int byte, Idx first, Idx end, Idx step,
                                            uint32_t lane, KeyAt key_at) {
  for (Idx base = first; base < end; base += step) {
    Key k[kUnroll];
    if (AHEAD) {
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u) {
        const Idx i = base + u * 64 + lane;
        k[u] = key_at(i, i < end);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const Idx i = base + u * 64 + lane;
      if (!AHEAD) k[u] = key_at(i, i < end);
      count_key(hist, k[u].key, i < end, byte, k[u].cls, gprefix, ng[ISIM_Q_ALL], ng[ISIM_Q_200], ng[ISIM_Q_500], lane);
    }
  }
}

// ---- one segment by one workgroup of kSelThreads, in LDS

// The select's state of a workgroup's segment; sel.owner_word is the embedding kernel's ticket, which keeps
// the struct, and with it the kernel's LDS, at its size.
struct SelState {
  State<uint32_t> sel;
  unsigned long long any[kSelWaves];  // per wave: OR of the segment's keys
};

// Idx: u32 is enough for a staged segment, a longer one may end within a step of 2^32
template <bool STAGED, bool AHEAD, typename Idx>
__device__ __forceinline__ void digit_pass(uint32_t *hist, const SelState &s, const unsigned long long *stage,
                                           const unsigned long long *seg, uint32_t n_seg, uint32_t n200, int byte,
                                           const uint32_t (&ng)[kClasses], uint32_t lane, uint32_t wave) {
  count_range<Idx, AHEAD>(hist, s.sel.gprefix, ng, byte, (Idx)wave * (64 * kUnroll), (Idx)n_seg,
                          (Idx)kSelWaves * (64 * kUnroll), lane, [&](Idx i, bool live) {
                            return Key{live ? (STAGED ? stage[i] : seg[i]) : 0, seg_class(i, n200)};
                          });
}

// Everything between "the segment is not empty" and "its cell is written": the keys' OR gives the top byte
// and from there down each digit is a histogram pass, a resolve (a wave per (class, quantile)) and a regroup.
// staged (workgroup-uniform, n_seg <= kStage): the keys are read from global memory once, into stage[kStage],
// else once per digit and once for the OR.  ONLY_STAGED: the caller has no other segments, and the staged
// digit pass reads each key where it counts it.  hist[kClasses * kMaxQ * kBins] is 16-byte aligned.  The
// caller puts a barrier between two calls: the first lines rewrite what the last ones read.
template <bool ONLY_STAGED>
__device__ __forceinline__ void select_segment(uint32_t *hist, unsigned long long *stage, SelState &s,
                                               const unsigned long long *seg, uint32_t n_seg, uint32_t n200, bool staged,
                                               uint32_t n_q, const Ppm &ppm, unsigned long long *cell) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  unsigned long long any = 0;
  if (staged) {
    for (uint32_t i = t; i < n_seg; i += kSelThreads) {
      const unsigned long long v = seg[i];
      stage[i] = v;
      any |= v;
    }
  } else {
    for (uint64_t i = t; i < n_seg; i += kSelThreads) any |= seg[i];
  }
  for (int d = 32; d; d >>= 1) any |= __shfl_xor(any, d, 64);
  if (lane == 0) s.any[wave] = any;
  setup(s.sel, t, n_q, n_seg, n200, n_seg - n200, ppm, cell);
  __syncthreads();
  any = 0;
  for (uint32_t w = 0; w < kSelWaves; ++w) any |= s.any[w];

  for (int byte = top_byte(any); byte >= 0; --byte) {
    const uint32_t ng[kClasses] = {min(s.sel.ngrp[ISIM_Q_ALL], n_q), min(s.sel.ngrp[ISIM_Q_200], n_q),
                                   min(s.sel.ngrp[ISIM_Q_500], n_q)};
    zero_bins<kSelThreads>(hist, ng, t);
    __syncthreads();
    if (ONLY_STAGED) digit_pass<true, false, uint32_t>(hist, s, stage, seg, n_seg, n200, byte, ng, lane, wave);
    else if (staged) digit_pass<true, true, uint64_t>(hist, s, stage, seg, n_seg, n200, byte, ng, lane, wave);
    else digit_pass<false, true, uint64_t>(hist, s, stage, seg, n_seg, n200, byte, ng, lane, wave);
    __syncthreads();
    for (uint32_t task = wave; task < kClasses * n_q; task += kSelWaves) {  // wave-uniform
      const uint32_t c = task / n_q, i = task % n_q;
      const uint32_t k = s.sel.k[c][i];
      if (!k) continue;  // empty class
      const uint32_t g = min(s.sel.grp[c][i], n_q - 1);
      // the four bins sum to at most n_seg
      const u32x4 b = *reinterpret_cast<const u32x4 *>(hist + (c * kMaxQ + g) * kBins + lane * 4);
      uint32_t digit, below;
      if (resolve<uint32_t>(b.x, b.y, b.z, b.w, k, lane, digit, below)) take_digit(s.sel, c, i, digit, k, below);
    }
    __syncthreads();
    if (t < kClasses) regroup(s.sel, t, n_q);
    __syncthreads();
  }
  write_values(s.sel, t, n_q, cell);
}

// ---- one launch per step, bins in global memory

// the LDS of a workgroup of hist_pass
struct alignas(16) HistLds {
  uint32_t hist[kClasses * kMaxQ * kBins];
  uint64_t gprefix[kClasses][kMaxQ];
  uint32_t ngrp[kClasses];
};

// Digit pass `byte` of a workgroup of kHistThreads over its part of a segment: per (class, group) of st a
// 256-bin histogram of that byte over the keys whose higher bytes equal the group's prefix, in LDS, then one
// flush into gbins[kClasses][n_q][kBins].  first, end and step: count_range's; keys() gives its key_at, and
// is called after the barriers, so that what it loads is not held over them.  ngrp is clamped to n_q, so a
// corrupted state stays inside the arrays.
template <typename Idx, typename Rank, typename Cnt, typename Keys>
__device__ __forceinline__ void hist_pass(HistLds &l, const State<Rank> &st, uint32_t n_q, int byte, Idx first, Idx end,
                                          Idx step, Keys keys, Cnt *gbins) {
  const uint32_t t = threadIdx.x;
  if (t < kClasses) l.ngrp[t] = min(st.ngrp[t], n_q);
  if (t < kClasses * kMaxQ) l.gprefix[t / kMaxQ][t % kMaxQ] = st.gprefix[t / kMaxQ][t % kMaxQ];
  __syncthreads();
  const uint32_t ng[kClasses] = {l.ngrp[ISIM_Q_ALL], l.ngrp[ISIM_Q_200], l.ngrp[ISIM_Q_500]};
  zero_bins<kHistThreads>(l.hist, ng, t);
  __syncthreads();
  count_range<Idx, true>(l.hist, l.gprefix, ng, byte, first, end, step, t & 63u, keys());
  __syncthreads();
  for (uint32_t c = 0; c < kClasses; ++c)
    for (uint32_t i = t; i < ng[c] * kBins; i += kHistThreads) {
      const uint32_t v = l.hist[c * kMaxQ * kBins + i];
      if (v) atomicAdd(&gbins[c * n_q * kBins + i], (Cnt)v);
    }
}

// After digit pass `byte`, one workgroup of kResolveThreads: the resolve per (class, quantile), wave i taking
// quantile i of every class, then the regroup, and the bins are cleared.  A byte above `top` holds zeros in
// every key: the prefixes keep a zero digit.  After byte 0 the values go to the cell.  grp is clamped to
// n_q - 1 like ngrp above.
template <typename Cnt, typename Rank>
__device__ __forceinline__ void resolve_pass(State<Rank> &st, Cnt *bins, uint32_t n_q, int byte, int top,
                                             unsigned long long *cell) {
  const uint32_t t = threadIdx.x, lane = t & 63u, i = t >> 6;
  if (byte <= top) {
    if (i < n_q) {
      for (uint32_t c = 0; c < kClasses; ++c) {
        const Cnt k = st.k[c][i];
        if (!k) continue;  // empty class
        const uint32_t g = min(st.grp[c][i], n_q - 1);
        const Cnt *b = bins + (c * n_q + g) * kBins + lane * 4;  // they sum to at most the number of keys
        uint32_t digit;
        Cnt below;
        if (resolve<Cnt>(b[0], b[1], b[2], b[3], k, lane, digit, below)) take_digit(st, c, i, digit, (Rank)k, (Rank)below);
      }
    }
    __syncthreads();  // every wave has read its bins and written its prefix
    if (t < kClasses) regroup(st, t, n_q);
    for (uint32_t w = t; w < kClasses * n_q * kBins; w += kResolveThreads) bins[w] = 0;
  }
  if (byte == 0) {
    __syncthreads();
    write_values(st, t, n_q, cell);
  }
}

}  // namespace rs
}  // namespace isim
