// DES item engine, what every stage shares: the block
// size, the Q24 log and histogram-edge tables, the draws, the kernel
// argument K and the per-item helpers.  A part of des_items.hip, included
// inside namespace isim::dit.
#pragma once

constexpr uint32_t kT = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__constant__ int32_t c_ln[257] = {
#include "des_ln_table.inc"
};
// service_request_duration_seconds edges (prometheus/handler.go:26-31), ns
__constant__ uint64_t c_edges[32] = {
    7000000ull,   8000000ull,   9000000ull,   10000000ull,  11000000ull,  12000000ull,  14000000ull,
    16000000ull,  18000000ull,  20000000ull,  25000000ull,  30000000ull,  35000000ull,  40000000ull,
    45000000ull,  50000000ull,  60000000ull,  70000000ull,  80000000ull,  90000000ull,  100000000ull,
    120000000ull, 140000000ull, 160000000ull, 180000000ull, 200000000ull, 250000000ull, 300000000ull,
    350000000ull, 400000000ull, 450000000ull, 500000000ull};

// The same bucket from a workgroup's LDS table by ceil(t / 1 ms) (every edge
// is a whole number of milliseconds; entry 501 is +Inf): one ds_read_u8
// instead of five dependent constant loads per item.
constexpr uint32_t kLutEntries = 502;
__device__ __forceinline__ void lut_init(uint8_t *lut) {
  for (uint32_t i = threadIdx.x; i < kLutEntries; i += blockDim.x) {
    uint32_t b = 0;
    while (b < 32 && (uint64_t)i * 1000000ull > c_edges[b]) ++b;
    lut[i] = (uint8_t)b;
  }
  __syncthreads();
}
__device__ __forceinline__ uint32_t lut_bucket(const uint8_t *lut, uint64_t t) {
  const uint64_t c = t < 500000001ull ? t : 500000001ull;
  return lut[(uint32_t)((c + 999999ull) / 1000000ull)];
}

__device__ __forceinline__ uint32_t prom_bucket(uint64_t t) {
  uint32_t lo = 0, hi = 32;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (t <= c_edges[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// word 0 of Philox4x32-10 (t, w2, w3) under the handler's seed
__device__ __forceinline__ uint32_t draw0(uint64_t t, uint32_t w2, uint32_t w3, uint32_t k0, uint32_t k1) {
  uint32_t a = (uint32_t)t, b = (uint32_t)(t >> 32), c = w2, d = w3;
  tw::philox10(a, b, c, d, k0, k1);
  return a;
}

// -ln(w / 2^24) in Q24, w = (u >> 8) + 1 (des.h des_exp_q24_host)
__device__ __forceinline__ uint64_t exp_q24(uint32_t u) {
  const uint32_t w = (u >> 8) + 1u;
  const int e = 31 - __builtin_clz(w);
  const uint32_t f = (w << (24 - e)) & 0xFFFFFFu;
  const uint32_t idx = f >> 16, rem = f & 0xFFFFu;
  const int64_t lnm = c_ln[idx] + ((((int64_t)c_ln[idx + 1] - c_ln[idx]) * (int64_t)rem) >> 16);
  return (uint64_t)(24 * kLn2Q24 - ((int64_t)e * kLn2Q24 + lnm));
}

struct K {
  // plan
  const DesPos *pos;
  const DesItemPos *ip;
  const DesStep *steps;
  const uint32_t *step_round;
  // tree (pre-walk)
  const unsigned long long *nodes;
  uint32_t n_nodes;
  const TreeExt *ext;
  const TreeStep *tstep;
  uint32_t *spill;
  // per trace
  uint64_t *gap, *A, *cnt, *tend;  // cnt: hops; tend: inclusive item offsets
  uint32_t *terr;                  // status_err
  // per item
  uint32_t *ipos, *ipar, *itr, *ihop;
  uint8_t *iown;
  uint32_t *troot;                 // per trace: its entry item (items are renumbered position-major)
  // the pre-walk's items in trace order, before the renumbering: one 16-byte
  // record each (one line touched per item, not one per field) — x: position
  // (k_own replaces it with the hop), y: duration without contention
  // (saturated), z: caller hop (k_own: the caller's new index; kNone: the
  // entry), w: trace | status << 31
  uint4 *erec;
  uint64_t *IA, *IS, *IF, *acc, *bk;
  const uint64_t *acc_prev;        // cyclic schedules: the previous pass's callee maxima
  const uint64_t *row_hold;        // per duration-table row: the service's worker hold
  uint32_t aw, bw;                 // acc / bk slots per item
  uint64_t M;
  // outputs
  unsigned long long *stats, *table;
  isim_trace_rec *records;
  uint64_t n, trace_begin, mean_ns;
  uint32_t k0, k1, n_slots;
  // cyclic schedules (des_plan.cpp): passes to a fixed point; a quiet pass
  // records no statistics and flags any stored value it changes
  uint32_t quiet;
  uint32_t *changed;
  uint32_t first;                  // the first quiet pass: acc_prev holds contention-free relative maxima
  // incremental quiet passes (round 5): traces in chunks of 2^cshift; a pass
  // recomputes the step begins, arrivals and finishes of the items whose
  // chunk had a value change in the previous pass (dcur; null: every item),
  // and marks the chunks whose values it changes (dnext).  Queue scans stay
  // whole-round (a change moves later traces of the queue: their chunks are
  // marked as their starts change)
  // Round 6: the same marks per TRACE as well (dcur_t / dnext_t, n bytes):
  // after the first passes about 1 % of the items change per pass, spread
  // over enough traces that nearly every 256-trace chunk stays marked; a
  // chunk mark now only pre-filters, an item is recomputed when its own
  // trace changed (the invariant holds per trace: every dependence between
  // traces goes through the whole-round queue scans, which mark the traces
  // whose starts they change)
  const uint8_t *dcur;
  uint8_t *dnext;
  const uint8_t *dcur_t;
  uint8_t *dnext_t;
  uint32_t cshift;
  uint16_t *irep;                  // per item: its replica (drawn once per batch)
  // mode B: the walks draw the errors (a failed step ends its script); per
  // item the call step it failed at (kNone: it did not fail)
  uint32_t modeb;
  uint32_t *ifst;
  // a look-back that gave up after spin_limit polls (des_spin_limit) sets
  // *fault: the batch is not accumulated and des_items_launch fails
  uint32_t *fault;
  uint32_t spin_limit;
};

// a quiet pass flags a change with ONE atomic per wave, and none once the
// flag is set (millions of lanes changing values in the first passes would
// otherwise serialise on the flag's address)
__device__ __forceinline__ void store_tracked(const K &k, uint64_t *p, uint64_t v, uint32_t item) {
  if (k.changed) {
    const bool diff = *p != v;
    if (diff && k.dnext) {
      const uint32_t t = k.itr[item];
      k.dnext[t >> k.cshift] = 1;
      k.dnext_t[t] = 1;
    }
    const unsigned long long m = __ballot(diff);
    if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)m) - 1u) {
      if (__hip_atomic_load(k.changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(k.changed, 1u);
    }
  }
  *p = v;
}

__device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * kT + threadIdx.x; }
// the item is recomputed in this pass (its trace changed in the previous one;
// the chunk map first: it is small and cached)
__device__ __forceinline__ bool live(const K &k, uint32_t i) {
  if (!k.dcur) return true;
  const uint32_t t = k.itr[i];
  return k.dcur[t >> k.cshift] && k.dcur_t[t];
}
__device__ __forceinline__ uint64_t nthreads() { return (uint64_t)gridDim.x * kT; }
__device__ __forceinline__ uint64_t item_off(const K &k, uint64_t t) { return t ? k.tend[t - 1] : 0; }
