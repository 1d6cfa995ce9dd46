// The DES's arrival draw and its Q24 exponential on the device (DESIGN.md
// §10.1, §10.2), shared by des.hip and load_profile.hip.
//
// Include it INSIDE the including file's device namespace, below namespace
// isim (des.h: kLn2Q24), after <hip/hip_runtime.h>: every translation unit
// gets its own c_ln table in constant memory and its own inlined functions
// (the code objects are linked separately), and the names keep the
// namespace they had in des.hip.  One inclusion per translation unit: a
// second one is an error, not a silent second table.
#ifdef ISIM_DES_DRAW_H_INCLUDED
#error "des_draw.h is included once per translation unit, inside its device namespace"
#endif
#define ISIM_DES_DRAW_H_INCLUDED

__constant__ int32_t c_ln[257] = {
#include "des_ln_table.inc"
};

__device__ __forceinline__ uint32_t des_xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Philox4x32-10 (Random123), counter (t_lo, t_hi, w2, w3), key (k0, k1)
__device__ __forceinline__ void des_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = des_xor3((uint32_t)(p1 >> 32), c[1], k0);
  const uint32_t n2 = des_xor3((uint32_t)(p0 >> 32), c[3], k1);
  c[0] = n0;
  c[1] = (uint32_t)p1;
  c[2] = n2;
  c[3] = (uint32_t)p0;
}
__device__ __forceinline__ void des_philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    des_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ uint32_t des_draw(uint64_t t, uint32_t w2, uint32_t w3, uint32_t word, uint32_t k0,
                                             uint32_t k1) {
  uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), w2, w3};
  des_philox(c, k0, k1);
  return word == 0 ? c[0] : word == 1 ? c[1] : word == 2 ? c[2] : c[3];
}

// -ln(w / 2^24) in Q24, w = (u >> 8) + 1 (des.h / DESIGN §10.2)
__device__ __forceinline__ uint64_t des_exp_q24(uint32_t u) {
  const uint32_t w = (u >> 8) + 1u;
  const int e = 31 - __builtin_clz(w);
  const uint32_t f = (w << (24 - e)) & 0xFFFFFFu;
  const uint32_t idx = f >> 16, rem = f & 0xFFFFu;
  const int64_t lnm = c_ln[idx] + ((((int64_t)c_ln[idx + 1] - c_ln[idx]) * (int64_t)rem) >> 16);
  return (uint64_t)(24 * kLn2Q24 - ((int64_t)e * kLn2Q24 + lnm));
}
