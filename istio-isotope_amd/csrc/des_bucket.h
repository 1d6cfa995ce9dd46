// The Prometheus duration bucket of a latency (ISIM_ST_PROM's edges), stated
// once for every kernel that fills such a histogram: the DES engine (des.hip)
// and the timeline (timeline.hip).  Device code; include from a .hip file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace isim {
namespace dev {

// Prometheus duration bucket (prometheus/handler.go:26-35): the first edge
// >= t.  The edges are whole milliseconds in six arithmetic runs (7..12 by 1,
// 14..20 by 2, 25..50 by 5, 60..100 by 10, 120..200 by 20, 250..500 by 50), so
// with m = ceil(t / 1 ms) (t <= e ms  <=>  m <= e) the bucket is the run's
// base + ceil((m - run start) / step).  The kernels look m up in a 501-byte
// LDS table built from this formula (des_bucket_lut: 7 VALU per duration
// instead of 57).
__host__ __device__ constexpr uint32_t des_prom_bucket_m(uint32_t m) {
  const uint32_t lo = m <= 12 ? 7 : m <= 20 ? 12 : m <= 50 ? 20 : m <= 100 ? 50 : m <= 200 ? 100 : 200;
  const uint32_t base = m <= 12 ? 0 : m <= 20 ? 5 : m <= 50 ? 9 : m <= 100 ? 15 : m <= 200 ? 20 : 25;
  const uint32_t d = m <= 12 ? 1 : m <= 20 ? 2 : m <= 50 ? 5 : m <= 100 ? 10 : m <= 200 ? 20 : 50;
  // ceil(65536 / d): exact quotients for numerators below 2^9
  const uint32_t M = m <= 12 ? 65536 : m <= 20 ? 32768 : m <= 50 ? 13108 : m <= 100 ? 6554 : m <= 200 ? 3277 : 1311;
  const uint32_t n = m > lo ? m - lo : 0;
  return base + (((n + d - 1) * M) >> 16);
}
constexpr uint32_t kBucketLut = 502;  // m = ceil(t / 1 ms) in 0..500; 501: above 500 ms (+Inf)
constexpr uint32_t kBucketLutWords = 128;
struct DesBucketLut {
  uint32_t w[kBucketLutWords];  // byte m of the table: the bucket of m (m <= 501), little-endian
  constexpr DesBucketLut() : w() {
    for (uint32_t m = 0; m < 4 * kBucketLutWords; ++m)
      w[m / 4] |= (m < kBucketLut ? des_prom_bucket_m(m) : 32u) << (8 * (m % 4));
  }
};
__device__ constexpr DesBucketLut kDesBucketLut{};
// copies the table into the workgroup's LDS (the caller's barrier publishes
// it): one 4-byte word per thread instead of computing 502 entries
__device__ __forceinline__ void des_bucket_lut_init(uint8_t *lut) {
  for (uint32_t i = threadIdx.x; i < kBucketLutWords; i += blockDim.x)
    reinterpret_cast<uint32_t *>(lut)[i] = kDesBucketLut.w[i];
}
__device__ __forceinline__ uint32_t des_prom_bucket32(const uint8_t *lut, uint32_t t) {
  const uint32_t c = t < 500000001u ? t : 500000001u;  // v_min_u32
  return lut[(c + 999999u) / 1000000u];
}
__device__ __forceinline__ uint32_t des_prom_bucket(const uint8_t *lut, uint64_t t) {
  const uint32_t c = (uint32_t)(t < 500000001ull ? t : 500000001ull);  // branch-free: entry 501 is the +Inf bucket
  return lut[(c + 999999u) / 1000000u];
}

}  // namespace dev
}  // namespace isim
