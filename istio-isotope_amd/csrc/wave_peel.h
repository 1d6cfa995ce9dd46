// The ballot peel: lanes of a wave that update the same
// word act once.  Shared by quantile.hip and timeline_quantiles.hip (through
// radix_select.h's wave_add), and by timeline.hip.
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

}  // namespace dev
}  // namespace isim
