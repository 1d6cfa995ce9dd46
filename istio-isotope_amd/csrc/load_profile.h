// The load-profile rule (include/isim.h isim_load_profile*),
// one header for load_profile.cpp (host compiler) and load_profile.hip (host
// and device): a profile compiled into a table of segments, and the map from
// work u (Q24, a unit-rate stream) to time t (ns), in exact integer arithmetic.
//
//   compile  T_0 = C_0 = 0, W_j = floor(D_j 2^24 / m_j) (0 for a pause),
//            T_{j+1} = T_j + D_j, C_{j+1} = min(C_j + W_j, 2^63)
//   map      j = the largest index with C_j <= u,
//            t(u) = T_j + floor((u - C_j) m_j / 2^24)
//
// A segment without work (a pause, or D_j 2^24 < m_j) has C_{j+1} = C_j and is
// never the largest index, so the map skips it and only its duration counts.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/isim.h"
#include "host_device.h"

namespace isim {
namespace lp {

constexpr uint32_t kMaxSegments = ISIM_LP_MAX_SEGMENTS;
constexpr uint64_t kMaxDuration = 1ull << 48;
constexpr uint64_t kMaxMean = 1ull << 34;
constexpr uint64_t kWorkEnd = 1ull << 63;   // work and time stay below this
constexpr uint64_t kHorizonEnd = 1ull << 62;  // a device batch's last possible arrival stays below this
constexpr uint64_t kMaxTraces = 1ull << 32;   // per arrivals call: u < 2^32 x 24 ln 2 x 2^24 < 2^61
// the largest work of one trace: E(draw) <= 24 ln 2 in Q24 (des.h kLn2Q24)
constexpr uint64_t kMaxWorkPerTrace = 24ull * 11629080ull;

// One compiled segment (device layout, 24 bytes): it starts at time T with
// the work C done, and from there a unit of work (2^24) takes m ns.
struct Seg {
  uint64_t T, C, m;
};

// floor(a m / 2^24) of the 128-bit product; false when it does not fit 64 bits
__host__ __device__ inline bool mul_shr24(uint64_t a, uint64_t m, uint64_t &out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t hi = __umul64hi(a, m), lo = a * m;
#else
  const unsigned __int128 p = (unsigned __int128)a * m;
  const uint64_t hi = (uint64_t)(p >> 64), lo = (uint64_t)p;
#endif
  out = (hi << 40) | (lo >> 24);
  return (hi >> 24) == 0;
}

// the largest j in [0, n) with seg[j].C <= u (seg[0].C is 0)
__host__ __device__ inline uint32_t find_seg(const Seg *seg, uint32_t n, uint64_t u) {
  uint32_t lo = 0, hi = n;  // seg[lo].C <= u, and seg[hi].C > u where hi < n
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg[mid].C <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

// t(u) inside segment s (s.C <= u); false when t reaches 2^63
__host__ __device__ inline bool seg_time(const Seg &s, uint64_t u, uint64_t &t) {
  uint64_t d;
  const bool fits = mul_shr24(u - s.C, s.m, d);
  t = s.T + d;
  return fits && d < kWorkEnd && t < kWorkEnd;
}

// ---- host side (load_profile.cpp)
struct Compiled {
  std::vector<Seg> seg;
  uint32_t flags = 0;
  bool paced() const { return (flags & ISIM_LP_PACED) != 0; }
};

// ISIM_OK, or ISIM_EINVAL with the reason in `err`
int compile(const isim_load_profile *lp, Compiled &out, std::string &err);
// t(u): ISIM_OK, or ISIM_ERANGE (u or t at or above 2^63)
int time_of(const Compiled &c, uint64_t u, uint64_t &t);
// the largest work n traces can reach: n x 24 ln 2 (Poisson) or n (paced), in Q24; n <= 2^32
uint64_t max_work(const Compiled &c, uint64_t n);
// t(max_work): the time no arrival of an n-trace batch passes; false when it
// is at or above 2^62 (the device's 64-bit products and sums need it below)
bool horizon(const Compiled &c, uint64_t n, uint64_t &t);

// ---- device side (load_profile.hip).  A profile on the device: the table
// uploaded by `upload` into device memory of table_bytes(n_seg).
struct DeviceProfile {
  const Seg *d_seg;
  uint32_t n_seg;
  uint32_t paced;
};
inline uint64_t table_bytes(uint32_t n_seg) { return (uint64_t)n_seg * sizeof(Seg); }
uint64_t arrival_blocks(uint64_t n);
// Writes c's table to d_seg by kernels that carry it in their arguments, so
// the host copy is free at return and a captured graph holds the values.
int upload(const Compiled &c, Seg *d_seg, void *stream);
// A[i] = t(u_i) for the n traces from trace_begin (the chunk sums in d_blk,
// arrival_blocks(n) + 1 words, dirty or not).  0, or 1 (HIP error).
int arrivals_launch(uint64_t seed, const DeviceProfile &p, uint64_t trace_begin, uint64_t n, uint64_t *d_arrivals,
                    uint64_t *d_blk, void *stream);
// The item engine's two steps around its own scan: work[i] = the work of
// trace trace_begin + i alone, and A[i] = t(A[i]) in place.
int work_launch(uint64_t seed, const DeviceProfile &p, uint64_t trace_begin, uint64_t n, uint64_t *d_work,
                void *stream);
int map_launch(const DeviceProfile &p, uint64_t n, uint64_t *d_arrivals, void *stream);

}  // namespace lp
}  // namespace isim
