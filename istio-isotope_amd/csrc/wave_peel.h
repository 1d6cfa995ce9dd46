// The ballot peel: lanes of a wave that update the same
// word act once.  Shared by the three quantile selects (radix_select.h's
// wave_add for their counts, wave_claim for their scatter cursors), and by
// timeline.hip and service_timeline.hip, which also share the DPP reductions
// below for their SUM and MAX words.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace isim {
namespace dev {

constexpr uint32_t kPeelAll = ~0u;  // ROUNDS: no cap

// Every lane of the wave calls this with its key (`none`: nothing to do).
// The first pending lane's key is broadcast and the lanes that hold it are
// found by a ballot: shared(k0, m, lead) then runs in every lane, once for
// all of them (m: their mask, lead: the first of them).  The peel ends after
// ROUNDS shared keys or at the first key held by fewer than four lanes, and
// each lane that still holds a key calls alone(key).  A wave on one key (a
// constant batch) takes one round; a wave whose keys are spread takes none.
//
// The tail's condition is `key != none` alone.  A lane leaves `rem` only in a
// round that also sets its key to none, so rem == 0 after the loop means no
// lane holds a key: testing rem as well adds nothing, and under a cap rem may
// be nonzero with this lane's key already taken.
template <uint32_t ROUNDS, typename Shared, typename Alone>
__device__ __forceinline__ void wave_peel(uint32_t key, uint32_t none, Shared shared, Alone alone) {
  unsigned long long rem = __ballot(key != none);
  for (uint32_t it = 0; (ROUNDS == kPeelAll || it < ROUNDS) && rem; ++it) {
    const int lead = __ffsll((long long)rem) - 1;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const unsigned long long m = __ballot(key == k0);
    if (__popcll(m) < 4) break;
    shared(k0, m, lead);
    if (key == k0) key = none;
    rem &= ~m;
  }
  if (key != none) alone(key);
}

// The peel for cursors: every lane with a key (`none`: no key) gets a position
// of its own from cur[key]; the leader claims a run of positions for the lanes
// that share its key and each takes the one of its rank among them.
__device__ __forceinline__ uint32_t wave_claim(uint32_t *cur, uint32_t key, uint32_t none, uint32_t lane) {
  uint32_t pos = 0;
  wave_peel<kPeelAll>(
      key, none,
      [&](uint32_t k0, unsigned long long m, int lead) {
        uint32_t first = 0;
        if ((int)lane == lead) first = atomicAdd(&cur[k0], (uint32_t)__popcll(m));
        first = (uint32_t)__builtin_amdgcn_readlane((int)first, lead);
        if (key == k0) pos = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      },
      [&](uint32_t k) { pos = atomicAdd(&cur[k], 1u); });
  return pos;
}

// ---- wave reductions (all 64 lanes active): row shifts, then the row totals
// broadcast into the later rows; lane 63 holds the result, which every lane
// gets.  0 is the identity of both operations, so lanes without a source read 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t lane63(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}
struct OpAdd {
  __device__ static uint64_t f(uint64_t a, uint64_t b) { return a + b; }
};
struct OpMax {
  __device__ static uint64_t f(uint64_t a, uint64_t b) { return a > b ? a : b; }
};
template <typename Op>
__device__ __forceinline__ uint64_t wave_reduce(uint64_t v) {
  v = Op::f(v, dpp_u64<0x111, 0xF>(v));  // row_shr:1
  v = Op::f(v, dpp_u64<0x112, 0xF>(v));  // row_shr:2
  v = Op::f(v, dpp_u64<0x114, 0xF>(v));  // row_shr:4
  v = Op::f(v, dpp_u64<0x118, 0xF>(v));  // row_shr:8
  v = Op::f(v, dpp_u64<0x142, 0xA>(v));  // row_bcast:15 into rows 1, 3
  v = Op::f(v, dpp_u64<0x143, 0xC>(v));  // row_bcast:31 into rows 2, 3
  return lane63(v);
}

}  // namespace dev
}  // namespace isim
