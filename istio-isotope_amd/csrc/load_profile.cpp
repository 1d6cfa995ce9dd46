// Load profiles on the host (load_profile.h): the checks of a
// caller's isim_load_profile, its compilation into the segment table, and the
// map evaluated for one work value (isim_load_profile_time).
#include "load_profile.h"

namespace isim {
namespace lp {

int compile(const isim_load_profile *lp, Compiled &out, std::string &err) {
  auto bad = [&](const std::string &why) {
    err = "load profile: " + why;
    return (int)ISIM_EINVAL;
  };
  if (!lp) return bad("null profile");
  if (!lp->segments) return bad("null segments");
  if (lp->n_segments == 0 || lp->n_segments > kMaxSegments) return bad("n_segments must be in [1, 1024]");
  if (lp->flags & ~ISIM_LP_PACED) return bad("flags must be 0 or ISIM_LP_PACED");
  const uint32_t K = lp->n_segments;
  out.flags = lp->flags;
  out.seg.assign(K, Seg{0, 0, 0});
  uint64_t T = 0, C = 0;
  for (uint32_t j = 0; j < K; ++j) {
    const uint64_t D = lp->segments[j].duration_ns, m = lp->segments[j].mean_interarrival_ns;
    const std::string at = "segment " + std::to_string(j) + ": ";
    if (m > kMaxMean) return bad(at + "mean_interarrival_ns above 2^34");
    if (j + 1 < K) {
      if (D == 0 || D > kMaxDuration) return bad(at + "duration_ns must be in [1, 2^48]");
    } else {
      if (D != 0) return bad(at + "the last segment runs forever: its duration_ns must be 0");
      if (m == 0) return bad(at + "the last segment cannot be a pause (mean_interarrival_ns 0)");
    }
    out.seg[j] = Seg{T, C, m};
    if (j + 1 < K) {
      unsigned __int128 W = m ? (((unsigned __int128)D) << 24) / m : 0;
      const unsigned __int128 next = (unsigned __int128)C + W;
      C = next < kWorkEnd ? (uint64_t)next : kWorkEnd;
      T += D;
    }
  }
  return ISIM_OK;
}

int time_of(const Compiled &c, uint64_t u, uint64_t &t) {
  if (u >= kWorkEnd) return ISIM_ERANGE;
  const Seg &s = c.seg[find_seg(c.seg.data(), (uint32_t)c.seg.size(), u)];
  return seg_time(s, u, t) ? ISIM_OK : ISIM_ERANGE;
}

uint64_t max_work(const Compiled &c, uint64_t n) { return n * (c.paced() ? (1ull << 24) : kMaxWorkPerTrace); }

bool horizon(const Compiled &c, uint64_t n, uint64_t &t) {
  return time_of(c, max_work(c, n), t) == ISIM_OK && t < kHorizonEnd;
}

}  // namespace lp
}  // namespace isim
