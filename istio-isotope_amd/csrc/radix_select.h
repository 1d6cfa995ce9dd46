// The steps of the MSD radix select, device only: from the
// most significant byte down, per (class, group) a 256-bin histogram of the
// byte over the keys whose higher bytes equal the group's prefix, then per
// (class, quantile) the digit at which the running count reaches its rank.
// The loops that run the steps are segmented_select.h's: as launches with the
// counts in global memory (quantile.hip's batch, u64; service_quantiles.hip's
// long segments, u32) or as a loop of one workgroup with u32 counts in LDS
// (a row of timeline_quantiles.hip, a short segment of service_quantiles.hip).
// A group is one still-distinct prefix of a class: quantiles that share a
// prefix share a histogram.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/isim.h"
#include "quantile_rank.h"
#include "wave_peel.h"

namespace isim {
namespace rs {

constexpr uint32_t kMaxQ = ISIM_MAX_QUANTILES;
constexpr uint32_t kClasses = 3;  // ISIM_Q_ALL, ISIM_Q_200, ISIM_Q_500
constexpr uint32_t kBins = 256;

// Rank: wide enough for the number of keys (u64 for a batch, u32 for a row).
template <typename Rank>
struct State {
  uint64_t prefix[kClasses][kMaxQ];   // per quantile: the digits chosen so far
  uint64_t gprefix[kClasses][kMaxQ];  // per group: the digits chosen so far
  Rank k[kClasses][kMaxQ];            // per quantile: 1-based rank among the keys under its prefix (0: the class is empty)
  uint32_t grp[kClasses][kMaxQ];      // per quantile: its group
  uint32_t ngrp[kClasses];            // groups per class (0: the class is empty)
  uint32_t owner_word;                // fills the struct's last 8 bytes: the embedding kernel's, not the select's
};

// ---- init: thread (c, i) of kClasses * kMaxQ, for a class of n_c keys
template <typename Rank>
__device__ __forceinline__ void init(State<Rank> &s, uint32_t c, uint32_t i, uint32_t n_q, uint64_t n_c,
                                     const uint32_t *ppm) {
  if (i < n_q) {
    s.prefix[c][i] = 0;
    s.k[c][i] = n_c ? (Rank)isim::q::nearest_rank(n_c, ppm[i]) : (Rank)0;
    s.grp[c][i] = 0;
  }
  if (i == 0) {
    s.ngrp[c] = n_c ? 1u : 0u;
    s.gprefix[c][0] = 0;
  }
}

// the most significant byte with a set bit in the OR of the keys (the digits above it are zero); -1: every key is 0
__device__ __forceinline__ int top_byte(uint64_t any) { return any ? (63 - __clzll((long long)any)) >> 3 : -1; }

// ---- histogram: one LDS bin per lane (bin < 0: none); lanes of a wave that
// hit the same bin add once (wave_peel.h)
__device__ __forceinline__ void wave_add(uint32_t *hist, int bin, uint32_t lane) {
  isim::dev::wave_peel<isim::dev::kPeelAll>(
      (uint32_t)bin, ~0u,
      [&](uint32_t b0, unsigned long long m, int lead) {
        if ((int)lane == lead) atomicAdd(&hist[b0], (uint32_t)__popcll(m));
      },
      [&](uint32_t b) { atomicAdd(&hist[b], 1u); });
}

// One key of class cls (ISIM_Q_200 or ISIM_Q_500) in digit pass `byte` into
// hist[kClasses][kMaxQ][kBins] (live: the lane holds a key): its bin among the
// groups of ISIM_Q_ALL and among its class's, none where no group's prefix
// equals the key's higher bytes.  ng_*: the classes' group counts, wave-uniform.
__device__ __forceinline__ void count_key(uint32_t *hist, uint64_t key, bool live, int byte, uint32_t cls,
                                          const uint64_t (&gprefix)[kClasses][kMaxQ], uint32_t ng_all, uint32_t ng_200,
                                          uint32_t ng_500, uint32_t lane) {
  const uint32_t shift = 8u * (uint32_t)byte;
  const uint32_t digit = (uint32_t)(key >> shift) & 255u;
  const uint64_t hi = byte == 7 ? 0 : key >> (shift + 8);
  const uint32_t ng_max = max(ng_200, ng_500);
  int bin_all = -1, bin_cls = -1;
  for (uint32_t g = 0; g < ng_all; ++g)
    if (gprefix[0][g] == hi) bin_all = (int)(g * kBins + digit);
  const uint32_t ng = cls == ISIM_Q_200 ? ng_200 : ng_500;
  for (uint32_t g = 0; g < ng_max; ++g)  // a wave-uniform trip count
    if (g < ng && gprefix[cls][g] == hi) bin_cls = (int)((cls * kMaxQ + g) * kBins + digit);
  wave_add(hist, live ? bin_all : -1, lane);
  wave_add(hist, live ? bin_cls : -1, lane);
}

// ---- resolve: a wave over the 256 bins of one (class, quantile)'s group,
// lane l holding bins 4 l .. 4 l + 3.  The digit is the bin at which the
// running count reaches k (1-based).  True in the one lane that holds it, with
// the digit and the count of the bins below it.  If no bin reaches k (the keys
// changed under the select) the last lane takes it, so the digit stays a byte.
template <typename Cnt>
__device__ __forceinline__ bool resolve(Cnt b0, Cnt b1, Cnt b2, Cnt b3, Cnt k, uint32_t lane, uint32_t &digit,
                                        Cnt &below) {
  const Cnt sum = b0 + b1 + b2 + b3;
  Cnt incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const Cnt up = __shfl_up(incl, d, 64);
    if ((int)lane >= d) incl += up;
  }
  const unsigned long long reach = __ballot(incl >= k);
  const uint32_t owner = reach ? (uint32_t)__ffsll((long long)reach) - 1u : 63u;
  if (lane != owner) return false;
  below = incl - sum;
  uint32_t d = 0;
  if (below + b0 < k) {
    below += b0;
    d = 1;
    if (below + b1 < k) {
      below += b1;
      d = 2;
      if (below + b2 < k) {
        below += b2;
        d = 3;
      }
    }
  }
  digit = lane * 4 + d;
  return true;
}

// the owner lane: the digit joins quantile i's prefix and the bins below it leave its rank k
template <typename Rank>
__device__ __forceinline__ void take_digit(State<Rank> &s, uint32_t c, uint32_t i, uint32_t digit, Rank k, Rank below) {
  s.prefix[c][i] = (s.prefix[c][i] << 8) | digit;
  s.k[c][i] = k - below;
}

// ---- regroup: one thread per class; the distinct prefixes become the next pass's groups
template <typename Rank>
__device__ __forceinline__ void regroup(State<Rank> &s, uint32_t c, uint32_t n_q) {
  if (!s.ngrp[c]) return;
  uint32_t ng = 0;
  for (uint32_t q = 0; q < n_q; ++q) {
    const uint64_t p = s.prefix[c][q];
    uint32_t g = 0;
    while (g < ng && s.gprefix[c][g] != p) ++g;
    if (g == ng) s.gprefix[c][ng++] = p;
    s.grp[c][q] = g;
  }
  s.ngrp[c] = ng;
}

}  // namespace rs
}  // namespace isim
