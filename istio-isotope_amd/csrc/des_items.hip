// DES item engine: the exact per-replica worker-pool DES of
// a DYNAMIC walk — probabilistic calls (shouldSkipRequest, isotope/service/
// pkg/srv/executable.go:84-90), and in mode B (EXT) scripts that a failed
// call step ends (handler.go:66-75 with the 500 propagated) — on the GPU.
//
// The static engine (des.hip) keeps one row per (position, trace): every
// invocation executes in every trace.  Here a trace executes a few of the
// tree's potential invocations (config 4's mesh: 5.7 of 3,280), so the unit
// is the ITEM — one executed invocation — and the work is proportional to
// the items, not the positions:
//   1. arrivals    A_t = prefix sum of the exponential gaps (des.h Q24 log)
//   2. pre-walk    the lane tree walk (tree_walk.h Lane, one trace per lane,
//                  waves refilling from a batch counter, no error draws)
//                  counts each trace's executed invocations, a scan gives
//                  the item offsets, a second walk writes each item's
//                  position, caller and contention-free duration (hop id =
//                  item index within the trace: executed invocations in
//                  preorder); the own errors are drawn per item afterwards;
//                  then the items are RENUMBERED position-major (a stable
//                  radix sort by position), so every later pass reads them
//                  nearly in sequence
//   3. buckets     the items sorted (stable radix sort) by their position's
//                  queue round and by (finish group, position) (des_plan.cpp's
//                  schedule over the tree's positions); step-begin ops by round
//   4. rounds      step begins (BK per item and call step), queues (a round
//                  whose positions arrive in trace order with one replica is
//                  already in FIFO order; otherwise ONE stable radix sort by
//                  row | replica | arrival — two when the bits do not fit —,
//                  ties in (trace, hop) order as the oracle's event heap pops
//                  them — then one segmented max-plus scan: S = max(a,
//                  S_prev + hold); a service with W workers per replica: the
//                  order refined first into each replica's W rank classes,
//                  one such queue each, des_workers.h), finishes (deepest group first: F from the
//                  start or last BK and the callees' maxima, which each callee
//                  folds into its caller's per-step slot with a 64-bit atomic
//                  max); statistics summed in LDS per 4,096-item chunk; a
//                  cyclic schedule runs quiet passes to its fixed point first
//   5. finalize    records and latency statistics per trace.
// Reference anchors: as des.hip (handler.go:37-79, executable.go:94-179,
// svc/service.go:30-31, prometheus/handler.go:87-106).  Parity: bit-exact
// against oracle/des_oracle.c (its pre-walk, semantics v1 §2.3).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/device/device_scan_by_key.hpp>

#include "des_layout.h"
#include "kernel_abi.h"
#include "load_profile.h"
#include "spans.h"
#include "tree_walk.h"

namespace isim {
namespace dit {

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

// ---- 1. the exponential inter-arrival gaps (summed by a rocPRIM scan)
__global__ void __launch_bounds__(kT) k_gaps(K k) {
  for (uint64_t t = gid(); t < k.n; t += nthreads())
    k.gap[t] = (k.mean_ns * exp_q24(draw0(k.trace_begin + t, 0u, 0x80000001u, k.k0, k.k1))) >> 24;
}

// ---- 2. the pre-walk
struct GNodes {
  const unsigned long long *__restrict__ p;
  __device__ __forceinline__ tw::NodeW load(uint32_t i) const {
    const unsigned long long v = p[i];
    return tw::NodeW{(uint32_t)v, (uint32_t)(v >> 32)};
  }
};
// a wide tree's 16-byte nodes
struct GNodesW {
  const uint4 *__restrict__ p;
  __device__ __forceinline__ tw::NodeW4 load(uint32_t i) const {
    const uint4 v = p[i];
    return tw::NodeW4{v.x, v.y, v.z, v.w};
  }
};
struct CountSink {
  __device__ __forceinline__ void call(uint32_t) {}
  __device__ __forceinline__ void resp_leaf(uint32_t, bool) {}
  template <typename TT>
  __device__ __forceinline__ void resp(uint32_t, uint32_t, TT, bool) {}
};
// records of the current trace go to rec[base + hop], each written once,
// whole, when its invocation closes (tree_walk.h close_rec): position, its
// duration without contention (a lower bound is all k_relmax needs: u64
// durations saturate at 2^32 - 1; the entry's is 0), caller hop, trace and
// in mode B the response status in bit 31 (mode A draws the own errors
// afterwards, k_own).  Before: the record at the open and the duration and
// status at the close — two scattered stores per item.
template <bool MB>
struct EmitSink : CountSink {
  static constexpr bool kCloseRec = true;
  uint4 *rec;
  uint64_t base;
  uint32_t t;
  template <typename TT>
  __device__ __forceinline__ void rec_close(uint32_t p, uint32_t hop, uint32_t caller, TT T, bool st) {
    rec[base + hop] = uint4{p, (uint64_t)T > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)T,
                            caller == tw::kNoCaller ? kNone : caller, t | (MB && st ? 0x80000000u : 0u)};
  }
};

// One trace per lane; a lane whose trace has responded takes the next trace
// id of its wave's batch of 64, the wave claiming batches from a global
// counter as it runs dry (the kind-7 kernel's refill, tree.hip): the waves
// stay full instead of waiting for their longest trace.
// the tree's nodes in LDS when they fit (one ds_read_b64 per visit instead of
// an L2 round trip; kind 7's LdsNodes)
struct LNodes {
  const __attribute__((address_space(3))) unsigned long long *p;
  __device__ __forceinline__ tw::NodeW load(uint32_t i) const {
    const unsigned long long v = p[i];
    return tw::NodeW{(uint32_t)v, (uint32_t)(v >> 32)};
  }
};

template <int FR, bool SPILL, bool EMIT, bool T64, bool MB, bool W, class Nodes>
__device__ __forceinline__ void prewalk_body(const K &k, unsigned long long *work, const Nodes &nodes) {
  // mode A: no error draws in the walk (DRAW = false): an invocation's own
  // error changes no skip, so the walks only need the skip residues; the
  // errors are drawn per item afterwards (k_own), fully parallel.  Mode B:
  // the errors decide which steps run, so the walk draws them (MODEB, DRAW)
  tw::Lane<FR, MB, true, SPILL, MB, std::conditional_t<T64, uint64_t, uint32_t>, W> L;
  if constexpr (SPILL) {
    L.sp = k.spill + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    L.sp_stride = gridDim.x * blockDim.x;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint64_t nxt = 0, lim = 0;
  bool dry = false, active = false;
  uint32_t t = 0;
  EmitSink<MB> s;
  s.rec = k.erec;
  s.base = 0;
  s.t = 0;
  CountSink cs;
  while (true) {
    if (active && L.done) {
      if constexpr (!EMIT) k.cnt[t] = L.hops();
      active = false;
    }
    unsigned long long idle = __ballot(!active);
    while (idle && !dry) {
      if (nxt >= lim) {
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(work, 1ull);
        b = __shfl(b, 0, 64);
        if (b * 64 >= k.n) {
          dry = true;
          break;
        }
        nxt = b * 64;
        lim = nxt + 64 < k.n ? nxt + 64 : k.n;
      }
      const uint32_t rank = (uint32_t)__popcll(idle & lt);
      const bool take = ((idle >> lane) & 1ull) && rank < lim - nxt;
      if (take) {
        t = (uint32_t)(nxt + rank);
        active = true;
        L.start(k.trace_begin + t);
        if constexpr (EMIT) {
          s.base = item_off(k, t);
          s.t = t;
        }
      }
      const unsigned long long took = __ballot(take);
      nxt += (uint64_t)__popcll(took);
      idle &= ~took;
    }
    if (!__ballot(active)) break;
    if (active && !L.done) {
      if constexpr (EMIT) L.step(nodes, k.ext, k.tstep, s, k.k0, k.k1);
      else L.step(nodes, k.ext, k.tstep, cs, k.k0, k.k1);
    }
  }
}

// (W: a wide tree — 16-byte nodes in global memory)
template <int FR, bool SPILL, bool EMIT, bool LDSN, bool T64, bool MB, bool W = false>
__global__ void __launch_bounds__(LDSN ? 1024 : kT) k_prewalk(K k, unsigned long long *work) {
  if constexpr (W) {
    prewalk_body<FR, SPILL, EMIT, T64, MB, true>(k, work, GNodesW{(const uint4 *)k.nodes});
  } else if constexpr (LDSN) {
    extern __shared__ unsigned long long s_nodes[];
    for (uint32_t i = threadIdx.x; i < k.n_nodes; i += blockDim.x) s_nodes[i] = k.nodes[i];
    __syncthreads();
    prewalk_body<FR, SPILL, EMIT, T64, MB, false>(
        k, work, LNodes{(const __attribute__((address_space(3))) unsigned long long *)s_nodes});
  } else {
    prewalk_body<FR, SPILL, EMIT, T64, MB, false>(k, work, GNodes{k.nodes});
  }
}

// ---- 2a. own errors (RecordRequestReceived's status in mode A): word
// (hop & 3) of Philox (t, hop >> 2, 0, 0) against the callee's threshold, as
// the walk draws it (tree_walk.h own_error); the trace's 500 count by atomics
// (errors are rare), its entry status below.  Mode B: the walk wrote each
// item's status (EmitSink::dur), only counted here.  Runs in trace order
// after the renumbering's inverse (inv) is known: the caller hop becomes the
// caller's NEW index here, where the caller's inv entry is a near read (same
// trace), so k_perm_apply gathers nothing but the record
__global__ void __launch_bounds__(kT) k_own(K k, const uint32_t *inv) {
  for (uint64_t i = gid(); i < k.M; i += nthreads()) {
    const uint4 r = k.erec[i];
    const uint32_t t = r.w & 0x7FFFFFFFu;
    const uint32_t hop = (uint32_t)(i - item_off(k, t));  // (a near read: t advances with i)
    const DesPos P = k.pos[r.x];
    bool own = k.modeb ? (r.w >> 31) != 0 : (P.flags & kDesFlagAlways) != 0;
    if (!k.modeb && !own && P.thr) {
      uint32_t a = (uint32_t)(k.trace_begin + t), b = (uint32_t)((k.trace_begin + t) >> 32), c = hop >> 2, d = 0;
      tw::philox10(a, b, c, d, k.k0, k.k1);
      own = tw::word4(hop & 3u, a, b, c, d) < P.thr;
    }
    k.erec[i] = uint4{hop, r.y, r.z == kNone ? kNone : inv[i - hop + r.z], t | (own ? 0x80000000u : 0u)};
    if (own) atomicAdd(k.terr + t, 1u);
  }
}
__global__ void __launch_bounds__(kT) k_root500(K k) {
  for (uint64_t t = gid(); t < k.n; t += nthreads())
    if (k.erec[item_off(k, t)].w >> 31) k.terr[t] |= 0x80000000u;
}

// ---- 2b. renumbering: items in (position, trace) order (a stable radix
// sort of the trace-ordered items by position) so that the passes, which
// visit a position's items together (queues by service, finishes by
// position), read the per-item arrays nearly in sequence
// (the sort reads its keys from the records: an item's position)
struct PosOf {
  __host__ __device__ uint32_t operator()(const uint4 &r) const { return r.x; }
};
// inv[old] = new
__global__ void __launch_bounds__(kT) k_perm_inv(K k, const uint32_t *perm, uint32_t *inv) {
  for (uint64_t j = gid(); j < k.M; j += nthreads()) inv[perm[j]] = (uint32_t)j;
}
__global__ void __launch_bounds__(kT) k_perm_apply(K k, const uint32_t *perm) {
  for (uint64_t j = gid(); j < k.M; j += nthreads()) {
    const uint4 r = k.erec[perm[j]];
    k.itr[j] = r.w & 0x7FFFFFFFu;
    k.iown[j] = (uint8_t)(r.w >> 31);
    k.ihop[j] = r.x;  // the hop (k_own)
    k.ipar[j] = r.z;  // the caller's new index (k_own)
  }
}
// mode B: an item with a callee that responded 500 failed at that callee's
// call step — the last it ran, so the smallest such step (statuses in iown)
__global__ void __launch_bounds__(kT) k_fail(K k) {
  for (uint64_t j = gid(); j < k.M; j += nthreads()) {
    const uint32_t par = k.ipar[j];
    if (par != kNone && k.iown[j]) atomicMin(k.ifst + par, (uint32_t)k.ip[k.ipos[j]].kstep);
  }
}

// cyclic schedules: the first quiet pass starts its cut step begins from the
// contention-free callee durations instead of zero (a lower bound of every
// callee's finish: F(c) >= begin(step) + H(c) + T(c)), so the passes only
// have to settle the queueing, not the whole chain of cut links.  Per
// (caller, call step): max over its callees of H + T, relative to the
// step's begin
__global__ void __launch_bounds__(kT) k_relmax(K k, const uint32_t *perm, unsigned long long *rel) {
  for (uint64_t j = gid(); j < k.M; j += nthreads()) {
    const uint32_t par = k.ipar[j];
    if (par == kNone) continue;
    const uint32_t v = k.ipos[j];
    const DesItemPos p = k.ip[v];
    const DesItemPos pp = k.ip[k.ipos[par]];
    if (pp.nsteps < 2) continue;  // no step begins: nothing reads it
    // off = H, except in the first call step: pre + H relative to the start (the step begins at start + pre)
    const uint64_t h = k.pos[v].off - (p.kstep == 0 ? k.steps[pp.bk_first].add : 0ull);
    atomicMax(rel + (uint64_t)par * k.aw + p.kstep, (unsigned long long)(h + k.erec[perm[j]].y));
  }
}

// a pass's callee maxima: for the items it recomputes, the maxima of the last
// pass that computed them move to `prev` (a cut step begin reads them) and
// the current ones restart from zero (a start can move down when a queue's
// order changes, so maxima are never carried over); the other items keep
// both (their finishes are not recomputed: the maxima they built stay valid)
__global__ void __launch_bounds__(kT) k_acc_init(K k, uint64_t *prev, uint64_t *cur) {
  for (uint64_t i = gid(); i < k.M; i += nthreads()) {
    if (!live(k, (uint32_t)i)) continue;
    for (uint32_t s = 0; s < k.aw; ++s) {
      if (prev) prev[i * k.aw + s] = cur[i * k.aw + s];
      cur[i * k.aw + s] = 0ull;
    }
  }
}

__global__ void __launch_bounds__(kT) k_roots(K k, const uint32_t *inv) {
  for (uint64_t t = gid(); t < k.n; t += nthreads()) k.troot[t] = inv[item_off(k, t)];
}

// ---- 3. bucket keys: the position's queue round and finish group
// (finish groups keyed with the position below them, so a group's items come
// position by position: k_fin sums runs), and the step-begin ops of the
// multi-step items: (round, item << 16 | step), appended one atomic per wave
__global__ void __launch_bounds__(kT) k_bucket_keys(K k, uint32_t *sk, unsigned long long *sv, uint32_t *n_ops) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t i0 = gid() - lane; i0 < k.M; i0 += nthreads()) {  // whole waves stay in the loop
    const uint64_t i = i0 + lane;
    uint32_t nst = 0;
    DesItemPos p{};
    if (i < k.M) {
      p = k.ip[k.ipos[i]];
      nst = p.nsteps >= 2 ? p.nsteps : 0u;
    }
    // wave prefix sum of the op counts
    uint32_t incl = nst;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t x = __shfl_up(incl, d, 64);
      if (lane >= d) incl += x;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    if (!total) continue;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(n_ops, total);
    base = __shfl(base, 0, 64);
    for (uint32_t s2 = 0; s2 < nst; ++s2) {
      const uint32_t o = base + incl - nst + s2;
      sk[o] = k.step_round[p.bk_first + s2] & ~kDesStepCut;
      // (item, step) and, in the top 16 bits, the item's trace chunk (k_steps'
      // liveness test without a gather)
      sv[o] = ((unsigned long long)(k.itr[i] >> k.cshift) << 48) | ((unsigned long long)i << 16) | s2;
    }
  }
}

// off[b] = first index of key b in the sorted keys >> shift (b = 0..nb)
__global__ void __launch_bounds__(kT) k_bounds(const uint32_t *keys, uint64_t m, uint32_t nb, uint32_t shift,
                                               uint32_t *off) {
  for (uint64_t i = gid(); i <= m; i += nthreads()) {
    const uint32_t lo = i == 0 ? 0u : (keys[i - 1] >> shift) + 1u;  // keys (keys[i-1], keys[i]] start here
    const uint32_t hi = i == m ? nb : (keys[i] >> shift);
    for (uint32_t b = lo; b <= hi && b <= nb; ++b) off[b] = (uint32_t)i;
  }
}

// The rounds' and finish groups' item lists from the position-major ids: a
// position's items are one contiguous range [poff[v], poff[v + 1]) in trace
// order, so each list is its positions' ranges, concatenated in position
// order (the host places them: qdst / fdst) — no sort of the items
__global__ void __launch_bounds__(kT) k_scatter_ids(K k, const uint32_t *poff, const uint32_t *qdst,
                                                    const uint32_t *fdst, uint32_t *qids, uint32_t *fids) {
  for (uint64_t j = gid(); j < k.M; j += nthreads()) {
    const uint32_t v = k.ipos[j];
    const uint32_t rel = (uint32_t)j - poff[v];
    qids[qdst[v] + rel] = (uint32_t)j;
    fids[fdst[v] + rel] = (uint32_t)j;
  }
}

// ---- 4a. step begins of round r (calls after calls, des.h DesStep)
__global__ void __launch_bounds__(kT) k_steps(K k, const unsigned long long *ops, uint64_t m) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const unsigned long long op = ops[j];
    if (k.dcur && !k.dcur[op >> 48]) continue;  // not recomputed in this pass (its chunk)
    const uint64_t i = (op >> 16) & 0xFFFFFFFFull;
    if (k.dcur && !k.dcur_t[k.itr[i]]) continue;  // (its trace)
    const uint32_t s = (uint32_t)(op & 0xFFFFu);
    if (k.ifst && s > k.ifst[i]) continue;  // mode B: the script failed at an earlier step
    const DesItemPos p = k.ip[k.ipos[i]];
    const uint32_t b = p.bk_first + s;
    const uint32_t sr = k.step_round[b];
    const DesStep st = k.steps[b];
    uint64_t v;
    if (s == 0) {
      v = k.IS[i];
    } else {
      v = k.bk[i * k.bw + (s - 1)] + st.smax;
      // a cut step's callees finish later in the pass: their maxima of the
      // previous one (the first pass: the contention-free lower bound)
      uint64_t c;
      if (!(sr & kDesStepCut)) c = k.acc[i * k.aw + (s - 1)];
      else if (k.first) c = k.bk[i * k.bw + (s - 1)] + k.acc_prev[i * k.aw + (s - 1)];
      else c = k.acc_prev[i * k.aw + (s - 1)];
      v = c > v ? c : v;
    }
    store_tracked(k, k.bk + i * k.bw + s, v + st.add, (uint32_t)i);
  }
}

// composition of two workers' max-plus maps (MP: des_layout.h)
struct MPThen {
  __device__ __forceinline__ MP operator()(const MP &a, const MP &b) const {
    const uint64_t c = a.C + b.B;
    return MP{a.B + b.B, c > b.C ? c : b.C};
  }
};

// ---- 4b. queues of round r: each item's arrival and replica, and the
// round's arrival range (mm[0..1]: one 64-bit atomic min / max per
// workgroup); in a quiet pass of a cyclic schedule mm[2] flags an arrival
// that differs from the previous pass's (none: the round's queues are as
// they were and the pass skips them); mm[3]: k_ordchk's flag.  The words
// alternate between two slots by launch; this launch empties the other slot
// for the next one.
// an item's arrival: its trace's, or its caller's start / step begin + off
__device__ __forceinline__ uint64_t item_arrival(const K &k, uint32_t i, uint32_t v, uint64_t off) {
  const uint32_t par = k.ipar[i];
  if (par == kNone) return k.A[k.itr[i]];
  const uint32_t ks = k.ip[v].kstep;
  return (ks == 0 ? k.IS[par] : k.bk[(uint64_t)par * k.bw + ks]) + off;
}
__device__ __forceinline__ void qarr_reset(unsigned long long *mm_next) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // vector atomics: no scalar-cache stores
    atomicExch(mm_next, ~0ull);
    atomicExch(mm_next + 1, 0ull);
    atomicExch(mm_next + 2, 0ull);
    atomicExch(mm_next + 3, 0ull);
  }
}
// the workgroup's range into mm[0..1]: one min / max per workgroup, and only
// when it improves on the current range (thousands of workgroups on one
// address otherwise serialise)
__device__ __forceinline__ void qarr_range(unsigned long long lo, unsigned long long hi, unsigned long long *mm) {
  for (uint32_t d = 32; d > 0; d >>= 1) {
    const unsigned long long x = __shfl_xor(lo, d, 64), y = __shfl_xor(hi, d, 64);
    lo = x < lo ? x : lo;
    hi = y > hi ? y : hi;
  }
  __shared__ unsigned long long s_lo[kT / 64], s_hi[kT / 64];
  if ((threadIdx.x & 63u) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kT / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    if (lo <= hi) {
      if (lo < __hip_atomic_load(mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(mm, lo);
      if (hi > __hip_atomic_load(mm + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mm + 1, hi);
    }
  }
}
// a quiet pass: flag an arrival that differs from the previous pass's (one atomic per wave at most)
__device__ __forceinline__ void qarr_changed(const K &k, bool diff, unsigned long long *mm) {
  const unsigned long long dm = __ballot(diff);
  if (dm && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)dm) - 1u &&
      __hip_atomic_load(mm + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull)
    atomicOr(mm + 2, 1ull);
}
__global__ void __launch_bounds__(kT) k_qarr(K k, const uint32_t *ids, uint64_t m, unsigned long long *mm,
                                             unsigned long long *mm_next) {
  qarr_reset(mm_next);
  unsigned long long lo = ~0ull, hi = 0;
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t i = ids[j];
    if (!live(k, i)) continue;  // its arrival is the previous pass's (the host keeps the round's range)
    const uint32_t v = k.ipos[i];
    const uint64_t a = item_arrival(k, i, v, k.pos[v].off);
    if (k.changed) qarr_changed(k, k.IA[i] != a, mm);
    k.IA[i] = a;
    lo = a < lo ? a : lo;
    hi = a > hi ? a : hi;
  }
  qarr_range(lo, hi, mm);
}

// each item's replica (the oracle's draw at its hop), once per batch
__global__ void __launch_bounds__(kT) k_reps(K k) {
  for (uint64_t i = gid(); i < k.M; i += nthreads()) {
    const DesPos P = k.pos[k.ipos[i]];
    uint32_t rep = 0;
    if (P.reps > 1) rep = draw0(k.trace_begin + k.itr[i], k.ihop[i], 0x80000002u, k.k0, k.k1) % P.reps;
    k.irep[i] = (uint16_t)rep;
  }
}

// ONE sort key when the bits fit: row | replica | arrival - amin (equal keys
// are put in (trace, hop) order afterwards: k_tiefix)
// (the value is the list index j: a cyclic schedule keeps each round's sorted
// order for the next pass, k_ordchk)
__global__ void __launch_bounds__(kT) k_qkey1(K k, const uint32_t *ids, uint64_t m, uint64_t amin, uint32_t rb,
                                              uint32_t ab, uint64_t *key, uint32_t *val) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t i = ids[j];
    const uint64_t row = k.pos[k.ipos[i]].row;
    key[j] = (((row << rb) | k.irep[i]) << ab) | (k.IA[i] - amin);
    val[j] = (uint32_t)j;
  }
}

// the previous pass's sorted order of a round (list indices j) against this
// pass's (row, replica, arrival): when (row, replica, arrival, j) strictly
// increases along it, it IS the stable sort of the round's queue keys, and
// the sort is skipped (k_qscan reads it); any inversion raises mm[3]
// (k_ordchk) and the host sorts (des_items_launch)
// the oracle's tie order of equal (row, replica, arrival): (trace, hop) —
// the event heap pops the earlier trace first (des_oracle.c).  The rounds'
// lists are position-major, so a stable sort alone would break such ties by
// position (a service reached from several positions, arrivals that meet
// exactly: starts chained by a hold equal to a hop cost, for one)
__device__ __forceinline__ uint64_t tie_key(const K &k, uint32_t i) {
  return ((uint64_t)k.itr[i] << 32) | k.ihop[i];
}
// runs of equal keys in a sorted round, re-ordered by (trace, hop): the run's
// first thread sorts it — insertion sort (runs are mostly short, or long
// and already in order), bounded on runs past kTieInsert by 8 moves per item,
// then heapsort, so that one lane's work stays O(r log r) when many items
// meet one service at one instant out of order (a wide fan-out to one
// replica, near-zero gaps).  Tie keys are unique
// (one item per (trace, hop)), so the order is the same either way.  LIST:
// the values are list indices into ids (k_qkey1), else item ids (k_qkey2)
constexpr uint64_t kTieInsert = 32;
template <bool LIST>
__global__ void __launch_bounds__(kT) k_tiefix(K k, const uint64_t *key, uint32_t *val, uint64_t m,
                                               const uint32_t *ids) {
  auto tk = [&](uint32_t v) { return tie_key(k, LIST ? ids[v] : v); };
  for (uint64_t j = gid(); j + 1 < m; j += nthreads()) {
    const uint64_t kj = key[j];
    if (key[j + 1] != kj || (j > 0 && key[j - 1] == kj)) continue;  // the first of a run of ties only
    uint64_t e = j + 2;
    while (e < m && key[e] == kj) ++e;
    // insertion sort: the stable radix sort leaves a run in its list order,
    // usually (trace, hop) order already, so this is O(run) — with a budget
    // of moves on a long run; past it (a wide fan-out meeting one service at
    // one instant) a heapsort, O(run log run).  (Heapsort alone
    // on every run past 32 items made c5p 26x slower: its long runs are
    // already in order.)
    const uint64_t budget = e - j <= kTieInsert ? ~0ull : 8u * (e - j);
    uint64_t moves = 0;
    for (uint64_t x = j + 1; x < e && moves <= budget; ++x) {
      const uint32_t v = val[x];
      const uint64_t t = tk(v);
      uint64_t y = x;
      while (y > j && tk(val[y - 1]) > t && ++moves <= budget) {
        val[y] = val[y - 1];
        --y;
      }
      val[y] = v;  // (the run stays a permutation when the budget runs out)
    }
    if (moves <= budget) continue;
    // heapsort of val[j, e) by tie key (a max-heap, then the max moved to the end)
    uint32_t *a = val + j;
    const uint64_t r = e - j;
    auto sift = [&](uint64_t root, uint64_t len) {
      const uint32_t v = a[root];
      const uint64_t t = tk(v);
      for (;;) {
        uint64_t c = 2 * root + 1;
        if (c >= len) break;
        uint64_t tc = tk(a[c]);
        if (c + 1 < len) {
          const uint64_t t1 = tk(a[c + 1]);
          if (t1 > tc) {
            ++c;
            tc = t1;
          }
        }
        if (tc <= t) break;
        a[root] = a[c];
        root = c;
      }
      a[root] = v;
    };
    for (uint64_t x = r / 2; x-- > 0;) sift(x, r);
    for (uint64_t len = r - 1; len > 0; --len) {
      const uint32_t top = a[0];
      a[0] = a[len];
      a[len] = top;
      sift(0, len);
    }
  }
}
// the kept order against this pass's arrivals (k_qarr's, in list order):
// any inversion raises mm[3] (this slot's, emptied by the launch before)
__global__ void __launch_bounds__(kT) k_ordchk(K k, const uint32_t *ids, const uint32_t *ord, const uint16_t *ordc,
                                               uint64_t m, unsigned long long *mm) {
  auto tuple = [&](uint32_t i, uint64_t &h, uint64_t &a) {
    h = ((uint64_t)k.pos[k.ipos[i]].row << 32) | k.irep[i];
    a = k.IA[i];
  };
  for (uint64_t jj = gid(); jj < m; jj += nthreads()) {
    bool inv = false;
    // a pair of items neither of which this pass recomputes kept its keys:
    // its order stands (ordc: their trace chunks, stored with the order)
    if (jj > 0 && (!k.dcur || k.dcur[ordc[jj]] || k.dcur[ordc[jj - 1]])) {
      const uint32_t i = ids[ord[jj]], ip = ids[ord[jj - 1]];
      uint64_t h, a, hp, ap;
      tuple(i, h, a);
      tuple(ip, hp, ap);
      inv = hp > h || (hp == h && (ap > a || (ap == a && tie_key(k, ip) > tie_key(k, i))));
    }
    const unsigned long long bm = __ballot(inv);
    if (bm && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)bm) - 1u &&
        __hip_atomic_load(mm + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull)
      atomicOr(mm + 3, 1ull);
  }
}

// a sort round's order kept for the next pass: the list indices and the
// items' trace chunks
__global__ void __launch_bounds__(kT) k_keep_ord(K k, const uint32_t *js, const uint32_t *ids, uint64_t m,
                                                 uint32_t *ord, uint16_t *ordc) {
  for (uint64_t jj = gid(); jj < m; jj += nthreads()) {
    const uint32_t j = js[jj];
    ord[jj] = j;
    ordc[jj] = (uint16_t)(k.itr[ids[j]] >> k.cshift);
  }
}

// k_pairs1's outputs along a kept order
__global__ void __launch_bounds__(kT) k_pairs1o(K k, uint64_t m, const uint32_t *ord, const uint32_t *ids,
                                                uint32_t rb, uint32_t *segk, uint32_t *rowk,
                                                MP *mp, uint32_t *sid) {
  for (uint64_t jj = gid(); jj < m; jj += nthreads()) {
    const uint32_t j = ord[jj];
    const uint32_t i = ids[j];
    const uint32_t row = k.pos[k.ipos[i]].row;
    const uint64_t hold = k.row_hold[row];
    segk[jj] = (row << rb) | k.irep[i];
    rowk[jj] = row;
    mp[jj] = MP{hold, k.IA[i] + hold};
    sid[jj] = i;
  }
}

// the segment key (row | replica), row, map (hold, a + hold) and item of
// each position of the sorted order
__global__ void __launch_bounds__(kT) k_pairs1(K k, uint64_t m, const uint64_t *key, const uint32_t *js,
                                               const uint32_t *ids, uint32_t rb, uint32_t ab, uint64_t amin,
                                               uint32_t *segk, uint32_t *rowk, MP *mp, uint32_t *sid) {
  const uint64_t amask = (1ull << ab) - 1ull;
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint64_t kk = key[j];
    const uint32_t row = (uint32_t)(kk >> (ab + rb));
    const uint64_t hold = k.row_hold[row];
    segk[j] = (uint32_t)(kk >> ab);
    rowk[j] = row;
    mp[j] = MP{hold, (kk & amask) + amin + hold};
    sid[j] = ids[js[j]];
  }
}

// a round whose positions need no sort (DesPlan::round_nosort): its items in
// their (position, trace) order are each position's FIFO already; the
// segment key is the position.  A zero-hold position (its arrivals need not
// come in trace order) starts each item at its own arrival (des_oracle.c: an
// invocation holding its worker for 0 starts when it arrives): every item is
// a segment of its own, keys alternating by list index above any position
__global__ void __launch_bounds__(kT) k_pairs0(K k, const uint32_t *ids, uint64_t m, uint32_t *segk, uint32_t *rowk,
                                               MP *mp, uint32_t *sid) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t i = ids[j];
    const uint32_t v = k.ipos[i];
    const uint32_t row = k.pos[v].row;
    const uint64_t hold = k.row_hold[row];
    segk[j] = hold ? v : 0x80000000u | (uint32_t)(j & 1u);
    rowk[j] = row;
    mp[j] = MP{hold, k.IA[i] + hold};
    sid[j] = i;
  }
}

// TWO stable sorts otherwise: replica | arrival - amin first, then the row
__global__ void __launch_bounds__(kT) k_qkey2(K k, const uint32_t *ids, uint64_t m, uint64_t amin, uint32_t rb,
                                              uint64_t *key, uint32_t *val,
                                              uint32_t *ovf) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t i = ids[j];
    const uint64_t a = k.IA[i] - amin;
    if (rb && (a >> (64 - rb))) atomicOr(ovf, 1u);
    key[j] = rb ? ((uint64_t)k.irep[i] << (64 - rb)) | a : a;
    val[j] = i;
  }
}

// the service's duration-table row of each item, in the arrival order
__global__ void __launch_bounds__(kT) k_rkeys(K k, const uint32_t *items, uint64_t m, uint32_t *rk, uint32_t *rv) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    rk[j] = k.pos[k.ipos[items[j]]].row;
    rv[j] = (uint32_t)j;
  }
}

__global__ void __launch_bounds__(kT) k_pairs2(K k, uint64_t m, const uint32_t *rkb, const uint32_t *rvb,
                                               const uint64_t *key, const uint32_t *items, uint32_t rb, uint32_t *segk,
                                               MP *mp, uint32_t *sid) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t j1 = rvb[j];
    const uint32_t i = items[j1];
    const uint32_t rep = rb ? (uint32_t)(key[j1] >> (64 - rb)) : 0u;
    const uint64_t hold = k.row_hold[rkb[j]];
    segk[j] = (rkb[j] << 16) | rep;
    mp[j] = MP{hold, k.IA[i] + hold};
    sid[j] = i;
  }
}

// start times; the queue figures per table row (runs of one row within a
// thread's span are summed before the atomics)
constexpr uint32_t kQSpan = 16;
__global__ void __launch_bounds__(kT) k_qout(K k, uint64_t m, const uint32_t *rkb, const uint32_t *sid,
                                             const MP *in, const MP *inc, uint32_t span) {
  // the chunk's first row's queue figures in LDS (a chunk of 4,096 items is
  // mostly one row: one global atomic per figure and chunk, not per lane run)
  __shared__ unsigned long long s_n, s_sw, s_mw, s_sh;
  __shared__ uint32_t s_row;
  // a workgroup takes kT x span consecutive sorted items (uniform trip
  // count: its barriers), a wave 64 x span, lane l the items l, l + 64, ...
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t kChunk = (uint64_t)kT * span;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kChunk; c0 < m; c0 += (uint64_t)gridDim.x * kChunk) {
    if (!k.quiet) {
      if (threadIdx.x == 0) {
        s_n = s_sw = s_mw = s_sh = 0;
        s_row = rkb[c0];
      }
      __syncthreads();
    }
    const uint32_t hrow = k.quiet ? kNone : s_row;
    const uint64_t j0 = c0 + (uint64_t)wave * 64 * span;
    uint32_t row = kNone;
    unsigned long long n = 0, sw = 0, mw = 0, sh = 0;
    auto flush = [&]() {
      if (row == kNone || !n) return;
      if (row == hrow) {
        atomicAdd(&s_n, n);
        if (sw) atomicAdd(&s_sw, sw);
        if (mw) atomicMax(&s_mw, mw);
        if (sh) atomicAdd(&s_sh, sh);
        return;
      }
      unsigned long long *tr = k.table + (uint64_t)row * ISIM_DES_ROW_WORDS;
      atomicAdd(tr + ISIM_DES_COUNT, n);
      if (sw) atomicAdd(tr + ISIM_DES_SUM_WAIT, sw);
      if (mw) atomicMax(tr + ISIM_DES_MAX_WAIT, mw);
      if (sh) atomicAdd(tr + ISIM_DES_SUM_HOLD, sh);
    };
    for (uint64_t j = j0 + lane; j < j0 + 64 * span && j < m; j += 64) {
      const uint32_t i = sid[j];
      const uint32_t r = rkb[j];
      const uint64_t hold = k.row_hold[r];
      const uint64_t S = inc[j].C - hold;
      const uint64_t a = in[j].C - hold;
      store_tracked(k, k.IS + i, S, i);
      if (r != row) {
        if (!k.quiet) flush();
        row = r;
        n = sw = mw = sh = 0;
      }
      const uint64_t w = S - a;
      n += 1;
      sw += w;
      mw = w > mw ? w : mw;
      sh += hold;
    }
    if (!k.quiet) {
      flush();
      __syncthreads();
      if (threadIdx.x == 0 && s_n) {
        unsigned long long *tr = k.table + (uint64_t)hrow * ISIM_DES_ROW_WORDS;
        atomicAdd(tr + ISIM_DES_COUNT, s_n);
        if (s_sw) atomicAdd(tr + ISIM_DES_SUM_WAIT, s_sw);
        if (s_mw) atomicMax(tr + ISIM_DES_MAX_WAIT, s_mw);
        if (s_sh) atomicAdd(tr + ISIM_DES_SUM_HOLD, s_sh);
      }
      __syncthreads();  // the LDS figures are reset for the next chunk
    }
  }
}

// ---- 4b'. the scan and k_qout in one pass.  The FIFO of one replica with a
// constant hold h (a segment: a run of one (row, replica) in the round's
// order; a zero-hold item is a segment of its own) starts its j-th item at
//   S_j = max over the segment's items i <= j of a_i + (j - i) h
//       = j h + max(a_i - i h),
// a segmented prefix maximum of the keys a_i - i h (i, j: list indices; the
// offset cancels within a segment; the host keeps j h below 2^62).  A
// workgroup takes a tile of kT x IPT items by ticket; tiles are chained by a
// decoupled look-back (des.hip chain_body's hand-off: sc1 stores drained
// before the flag store, sc1 loads).  The flag word carries the launch's
// epoch, so the states are cleared once per batch, not per launch.
// (QState, one per tile: des_layout.h)
constexpr uint32_t kQAgg = 1, kQInc = 2, kQEpochShift = 2;
constexpr int64_t kQMin = INT64_MIN;
__device__ __forceinline__ int64_t qmax(int64_t a, int64_t b) { return a > b ? a : b; }

// Where a round's queue order comes from (the kernel reads it directly, so
// no k_pairs* arrays are written and read back, except for kQArrays):
//   kQArrays  k_pairs2's arrays (segment key, row, item, (hold, a + hold))
//   kQList    a round that needs no sort: its list in (position, trace)
//             order; segment = the position (a zero-hold item alone); the
//             arrival computed here as k_qarr would (no k_qarr launched)
//   kQKept    a cyclic schedule's kept order that still sorts the round
//             (list indices; k_ordchk checked it)
//   kQSorted  the round's sorted keys row | replica | arrival - amin with
//             their list indices
constexpr int kQArrays = 0, kQList = 1, kQKept = 2, kQSorted = 3;
struct QSrc {
  const uint32_t *list;  // the round's item list
  const uint32_t *ord;   // kQKept
  const uint64_t *key;   // kQSorted
  const uint32_t *val;   // kQSorted
  uint64_t amin;         // kQSorted
  uint32_t rb, ab;       // replica bits; kQSorted: arrival bits
  const uint32_t *segk, *rowk, *sid;  // kQArrays
  const MP *mp;                       // kQArrays
};

// item j of the order: its segment key (hold-free: kQList treats zero holds
// itself), and with FULL its item, row, hold and arrival
template <int SRC, bool FULL>
__device__ __forceinline__ uint64_t qitem(const K &k, const QSrc &q, uint64_t j, uint32_t &i, uint32_t &row,
                                          uint64_t &h, uint64_t &a) {
  uint64_t sk;
  if constexpr (SRC == kQArrays) {
    sk = q.segk[j];
    if (FULL) {
      i = q.sid[j];
      row = q.rowk[j];
      const MP p = q.mp[j];
      h = p.B;
      a = p.C - p.B;
    }
  } else if constexpr (SRC == kQSorted) {
    const uint64_t kk = q.key[j];
    sk = kk >> q.ab;
    if (FULL) {
      i = q.list[q.val[j]];
      row = (uint32_t)(kk >> (q.ab + q.rb));
      h = k.row_hold[row];
      a = (kk & ((1ull << q.ab) - 1ull)) + q.amin;
    }
  } else {
    i = q.list[SRC == kQKept ? q.ord[j] : (uint32_t)j];
    const uint32_t v = k.ipos[i];
    if (SRC == kQList) {
      sk = v;
    } else {
      row = k.pos[v].row;
      sk = ((uint64_t)row << q.rb) | k.irep[i];
    }
    if (FULL) {
      const DesPos P = k.pos[v];
      row = P.row;
      h = k.row_hold[row];
      if (SRC == kQKept || !live(k, i)) {
        a = k.IA[i];  // (kQList: an item a quiet pass does not recompute keeps its own)
      } else {
        a = item_arrival(k, i, v, P.off);
        k.IA[i] = a;
      }
    }
  }
  return sk;
}

template <uint32_t IPT, int SRC>
__global__ void __launch_bounds__(kT) k_qscan(K k, uint64_t m, QSrc q, QState *qs, uint32_t *ticket, uint32_t tbase,
                                              uint32_t epoch) {
  constexpr uint32_t NW = kT / 64;
  __shared__ uint32_t s_tile, s_row;
  __shared__ int64_t w_v[NW], s_cin;
  __shared__ uint32_t w_f[NW];
  __shared__ unsigned long long s_n, s_sw, s_mw, s_sh;
  if (threadIdx.x == 0) {
    const uint32_t t = atomicAdd(ticket, 1u) - tbase;
    s_tile = t;
    const uint64_t j0 = (uint64_t)t * kT * IPT;
    if constexpr (SRC == kQArrays) s_row = q.rowk[j0];
    else if constexpr (SRC == kQSorted) s_row = (uint32_t)(q.key[j0] >> (q.ab + q.rb));
    else s_row = k.pos[k.ipos[q.list[SRC == kQKept ? q.ord[j0] : (uint32_t)j0]]].row;
    s_n = s_sw = s_mw = s_sh = 0;
  }
  __syncthreads();
  const uint32_t tile = s_tile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t w0 = (uint64_t)tile * kT * IPT + (uint64_t)wave * 64 * IPT;
  // the wave's rows of 64 items: a segmented max over the lanes, then over
  // the rows (cf, cv: the wave's items so far)
  int64_t v[IPT];
  bool f[IPT];
  uint64_t a[IPT], h[IPT];
  uint32_t it[IPT], rw[IPT];
  bool cf = false;
  int64_t cv = kQMin;
#pragma unroll
  for (uint32_t r = 0; r < IPT; ++r) {
    const uint64_t j = w0 + r * 64 + lane;
    bool s = false;
    int64_t x = kQMin;
    a[r] = h[r] = 0;
    it[r] = rw[r] = 0;
    // the previous item's segment: the lane below's, lane 0 reads it
    uint64_t sk = ~0ull, ps = ~0ull;
    if (j < m) {
      sk = qitem<SRC, true>(k, q, j, it[r], rw[r], h[r], a[r]);
      if (lane == 0 && j > 0) {
        uint32_t i1, r1;
        uint64_t h1, a1;
        ps = qitem<SRC, false>(k, q, j - 1, i1, r1, h1, a1);
      }
    }
    const uint64_t up = __shfl_up(sk, 1, 64);
    if (lane > 0) ps = up;
    if (j < m) {
      s = j == 0 || ps != sk || (SRC == kQList && h[r] == 0);
      x = (int64_t)(a[r] - j * h[r]);
    }
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const int64_t ox = __shfl_up(x, d, 64);
      const int os = __shfl_up((int)s, d, 64);
      if (lane >= d) {
        if (!s) x = qmax(x, ox);
        s = s || os;
      }
    }
    v[r] = s ? x : qmax(cv, x);
    f[r] = s || cf;
    cv = __shfl(v[r], 63, 64);
    cf = __shfl((int)f[r], 63, 64);
  }
  if (lane == 0) {
    w_v[wave] = cv;
    w_f[wave] = cf;
  }
  __syncthreads();
  if (wave == 0) {
    bool bf = false;
    int64_t bv = kQMin;
    for (uint32_t w = 0; w < NW; ++w) {
      bv = w_f[w] ? w_v[w] : qmax(bv, w_v[w]);
      bf = bf || w_f[w];
    }
    QState *me = qs + tile;
    const uint32_t ep = epoch << kQEpochShift;
    if (lane == 0 && (bf || tile > 0)) {  // a tile with a segment start knows its prefix already
      __hip_atomic_store(&me->agg, (uint64_t)bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bf) __hip_atomic_store(&me->inc, (uint64_t)bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&me->flag, ep | (bf ? kQAgg | kQInc : kQAgg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the open segment's max before the tile, unless its first item starts one
    int64_t cin = kQMin;
    if (tile > 0 && !__shfl((int)f[0], 0, 64)) {
      int64_t top = (int64_t)tile - 1;
      uint32_t spins = 0;
      for (;;) {
        if (spins >= k.spin_limit) {  // never expected (tickets order the tiles): fail the batch
          if (lane == 0) atomicOr(k.fault, 1u);
          break;
        }
        const int64_t jt = top - (int64_t)lane;  // lane 0: the nearest tile
        uint32_t fl = kQInc;                    // before tile 0: an empty prefix
        if (jt >= 0) {
          fl = __hip_atomic_load(&qs[jt].flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          fl = (fl >> kQEpochShift) == epoch ? fl & (kQAgg | kQInc) : 0u;
        }
        const uint64_t m0 = __ballot(fl == 0), mi = __ballot((fl & kQInc) != 0);
        const uint32_t fi = mi ? (uint32_t)__builtin_ctzll(mi) : 64u;
        const uint64_t upto = fi >= 63 ? ~0ull : ((1ull << (fi + 1)) - 1);
        if (m0 & upto) {  // a tile this one needs has not published yet
          __builtin_amdgcn_s_sleep(1);
          ++spins;
          continue;
        }
        int64_t x = kQMin;
        if (jt >= 0 && lane <= fi)
          x = (int64_t)__hip_atomic_load(lane == fi ? &qs[jt].inc : &qs[jt].agg, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t d = 32; d > 0; d >>= 1) x = qmax(x, __shfl_xor(x, d, 64));
        cin = qmax(cin, x);
        if (fi < 64) break;
        top -= 64;
      }
    }
    if (lane == 0) {
      if (!bf && tile > 0) {
        __hip_atomic_store(&me->inc, (uint64_t)qmax(cin, bv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&me->flag, ep | kQAgg | kQInc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s_cin = cin;
    }
  }
  __syncthreads();
  int64_t c = s_cin;
  for (uint32_t w = 0; w < wave; ++w) c = w_f[w] ? w_v[w] : qmax(c, w_v[w]);
  // starts; the queue figures as k_qout sums them
  const uint32_t hrow = k.quiet ? kNone : s_row;
  uint32_t row = kNone;
  unsigned long long n = 0, sw = 0, mw = 0, sh = 0;
  auto flush = [&]() {
    if (row == kNone || !n) return;
    if (row == hrow) {
      atomicAdd(&s_n, n);
      if (sw) atomicAdd(&s_sw, sw);
      if (mw) atomicMax(&s_mw, mw);
      if (sh) atomicAdd(&s_sh, sh);
      return;
    }
    unsigned long long *tr = k.table + (uint64_t)row * ISIM_DES_ROW_WORDS;
    atomicAdd(tr + ISIM_DES_COUNT, n);
    if (sw) atomicAdd(tr + ISIM_DES_SUM_WAIT, sw);
    if (mw) atomicMax(tr + ISIM_DES_MAX_WAIT, mw);
    if (sh) atomicAdd(tr + ISIM_DES_SUM_HOLD, sh);
  };
#pragma unroll
  for (uint32_t r = 0; r < IPT; ++r) {
    const uint64_t j = w0 + r * 64 + lane;
    if (j >= m) break;
    const uint64_t S = (uint64_t)(f[r] ? v[r] : qmax(c, v[r])) + j * h[r];
    const uint32_t i = it[r];
    store_tracked(k, k.IS + i, S, i);
    if (k.quiet) continue;
    const uint32_t rj = rw[r];
    if (rj != row) {
      flush();
      row = rj;
      n = sw = mw = sh = 0;
    }
    const uint64_t w = S - a[r];
    n += 1;
    sw += w;
    mw = w > mw ? w : mw;
    sh += h[r];
  }
  if (k.quiet) return;
  flush();
  __syncthreads();
  if (threadIdx.x == 0 && s_n) {
    unsigned long long *tr = k.table + (uint64_t)hrow * ISIM_DES_ROW_WORDS;
    atomicAdd(tr + ISIM_DES_COUNT, s_n);
    if (s_sw) atomicAdd(tr + ISIM_DES_SUM_WAIT, s_sw);
    if (s_mw) atomicMax(tr + ISIM_DES_MAX_WAIT, s_mw);
    if (s_sh) atomicAdd(tr + ISIM_DES_SUM_HOLD, s_sh);
  }
}

// ---- 4b''. worker pools: a pooled round's order refined into rank classes
#include "des_workers.h"

// ---- 4c. finishes of one group (its items position by position): per
// item the finish and its callee maximum into the caller's slot; the
// statistics summed over a thread's run of one position (and one bucket for
// the histogram) before the atomics
__global__ void __launch_bounds__(kT) k_fin(K k, const uint32_t *ids, uint64_t m, uint32_t span) {
  __shared__ uint8_t lut[kLutEntries];
  // the duration histogram of the chunk's first row (a chunk of 4,096 sorted
  // items is mostly one position): LDS atomics, one global add per bucket
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ uint32_t s_row, s_pos;
  // and the chunk's first position's duration sums and site counts
  __shared__ unsigned long long f_d0, f_d1, f_n, f_n5;
  if (!k.quiet) lut_init(lut);
  // a workgroup takes kT x span consecutive sorted items (uniform trip
  // count: its barriers), a wave 64 x span of them, lane l the items
  // l, l + 64, ...: coalesced loads, and a lane's items mostly share a
  // position, so its runs sum before the atomics
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t kChunk = (uint64_t)kT * span;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kChunk; c0 < m; c0 += (uint64_t)gridDim.x * kChunk) {
    if (!k.quiet) {
      for (uint32_t x = threadIdx.x; x < 2 * ISIM_N_PROM; x += kT) hist[x] = 0;
      if (threadIdx.x == 0) {
        s_pos = k.ipos[ids[c0]];
        s_row = k.pos[s_pos].row;
        f_d0 = f_d1 = f_n = f_n5 = 0;
      }
      __syncthreads();
    }
    const uint32_t hrow = k.quiet ? kNone : s_row, hpos = k.quiet ? kNone : s_pos;
    const uint64_t j0 = c0 + (uint64_t)wave * 64 * span;
    uint32_t v_run = kNone, b_run = kNone;
    DesPos P{};
    DesItemPos p{};
    unsigned long long n = 0, n5 = 0, d0 = 0, d1 = 0, nb = 0;
    auto flush_bucket = [&]() {
      if (!k.quiet && nb) {
        if (P.row == hrow) atomicAdd(&hist[b_run], (uint32_t)nb);
        else atomicAdd(k.table + (uint64_t)P.row * ISIM_DES_ROW_WORDS + b_run, nb);
      }
      nb = 0;
    };
    auto flush = [&]() {
      flush_bucket();
      if (k.quiet || v_run == kNone || !n) return;
      if (v_run == hpos) {
        atomicAdd(&f_n, n);
        if (n5) atomicAdd(&f_n5, n5);
        if (d0) atomicAdd(&f_d0, d0);
        if (d1) atomicAdd(&f_d1, d1);
        return;
      }
      unsigned long long *tr = k.table + (uint64_t)P.row * ISIM_DES_ROW_WORDS;
      if (d0) atomicAdd(tr + 2 * ISIM_N_PROM, d0);
      if (d1) atomicAdd(tr + 2 * ISIM_N_PROM + 1, d1);
      if (P.parent != kDesNoParent) {
        atomicAdd(k.stats + ISIM_ST_SITES + P.slot, n);
        if (n5) atomicAdd(k.stats + ISIM_ST_SITES + k.n_slots + P.slot, n5);
      }
    };
    for (uint64_t j = j0 + lane; j < j0 + 64 * span && j < m; j += 64) {
      const uint32_t i = ids[j];
      if (k.quiet && !live(k, i)) continue;
      const uint32_t v = k.ipos[i];
      if (v != v_run) {
        flush();
        v_run = v;
        P = k.pos[v];
        p = k.ip[v];
        n = n5 = d0 = d1 = 0;
        b_run = kNone;
      }
      uint64_t F;
      const uint32_t fst = k.ifst ? k.ifst[i] : kNone;
      if (P.flags & kDesFlagLeaf) {
        F = k.IS[i] + P.floor;
      } else if (fst != kNone) {
        // mode B, failed at call step fst: that step's end (its begin plus its
        // longest sleep, or its callees' finishes), no later command
        const uint64_t b0 = p.nsteps >= 2 ? k.bk[(uint64_t)i * k.bw + fst] : k.IS[i];
        const uint64_t sm = p.nsteps >= 2 && fst + 1u < p.nsteps ? k.steps[p.bk_first + fst + 1].smax : P.floor;
        const uint64_t c = k.acc[(uint64_t)i * k.aw + fst];
        F = c > b0 + sm ? c : b0 + sm;
      } else {
        const uint32_t last = p.nsteps >= 2 ? p.nsteps - 1u : 0u;
        F = (p.nsteps >= 2 ? k.bk[(uint64_t)i * k.bw + last] : k.IS[i]) + P.floor;
        const uint64_t c = k.acc[(uint64_t)i * k.aw + last];
        F = (c > F ? c : F) + P.post;
      }
      store_tracked(k, k.IF + i, F, i);
      const uint32_t par = k.ipar[i];
      if (par != kNone)
        atomicMax((unsigned long long *)(k.acc + (uint64_t)par * k.aw + p.kstep), (unsigned long long)F);
      if (k.quiet) continue;
      const uint32_t own = k.iown[i];
      const uint64_t dur = F - k.IA[i];
      const uint32_t b = own * ISIM_N_PROM + lut_bucket(lut, dur);
      if (b != b_run) {
        flush_bucket();
        b_run = b;
      }
      nb += 1;
      n += 1;
      n5 += own;
      if (own) d1 += dur;
      else d0 += dur;
    }
    flush();
    if (!k.quiet) {
      __syncthreads();
      for (uint32_t x = threadIdx.x; x < 2 * ISIM_N_PROM; x += kT)
        if (hist[x]) atomicAdd(k.table + (uint64_t)hrow * ISIM_DES_ROW_WORDS + x, (unsigned long long)hist[x]);
      if (threadIdx.x == 0 && f_n) {
        unsigned long long *tr = k.table + (uint64_t)hrow * ISIM_DES_ROW_WORDS;
        if (f_d0) atomicAdd(tr + 2 * ISIM_N_PROM, f_d0);
        if (f_d1) atomicAdd(tr + 2 * ISIM_N_PROM + 1, f_d1);
        const DesPos P0 = k.pos[hpos];
        if (P0.parent != kDesNoParent) {
          atomicAdd(k.stats + ISIM_ST_SITES + P0.slot, f_n);
          if (f_n5) atomicAdd(k.stats + ISIM_ST_SITES + k.n_slots + P0.slot, f_n5);
        }
      }
      __syncthreads();  // the LDS figures are reset for the next chunk
    }
  }
}

// ---- 5. records and the latency statistics
__global__ void __launch_bounds__(kT) k_final(K k) {
  if (*k.fault) return;  // a failed batch writes no record and accumulates nothing
  __shared__ uint32_t hp[2 * ISIM_N_PROM], hl[2 * ISIM_N_LOG2];
  __shared__ unsigned long long red[6][kT / 64];
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kT) hp[i] = 0;
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_LOG2; i += kT) hl[i] = 0;
  __syncthreads();
  unsigned long long sl = 0, sh = 0, se = 0, n5 = 0, mn = ~0ull, mx = 0;
  for (uint64_t t = gid(); t < k.n; t += nthreads()) {
    const uint64_t root = k.troot[t];
    const uint64_t L = k.IF[root] - k.A[t];
    const uint32_t hops = (uint32_t)(k.tend[t] - item_off(k, t));
    const uint32_t s_e = k.terr[t];
    const uint32_t st = s_e >> 31, e = s_e & 0x7FFFFFFFu;
    if (k.records) {
      isim_trace_rec r;
      r.latency_ns = L;
      r.hops = hops;
      r.status_err = s_e;
      k.records[t] = r;
    }
    sl += L;
    sh += hops;
    se += e;
    n5 += st;
    mn = L < mn ? L : mn;
    mx = L > mx ? L : mx;
    atomicAdd(&hp[st * ISIM_N_PROM + prom_bucket(L)], 1u);
    atomicAdd(&hl[st * ISIM_N_LOG2 + (L ? 64u - (uint32_t)__builtin_clzll(L) : 0u)], 1u);
  }
  for (uint32_t d = 32; d > 0; d >>= 1) {
    sl += __shfl_xor(sl, d, 64);
    sh += __shfl_xor(sh, d, 64);
    se += __shfl_xor(se, d, 64);
    n5 += __shfl_xor(n5, d, 64);
    const unsigned long long a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63u) == 0) {
    const uint32_t w = threadIdx.x >> 6;
    red[0][w] = sl;
    red[1][w] = sh;
    red[2][w] = se;
    red[3][w] = n5;
    red[4][w] = mn;
    red[5][w] = mx;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kT)
    if (hp[i]) atomicAdd(k.stats + ISIM_ST_PROM + i, (unsigned long long)hp[i]);
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_LOG2; i += kT)
    if (hl[i]) atomicAdd(k.stats + ISIM_ST_LOG2 + i, (unsigned long long)hl[i]);
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < kT / 64; ++w) {
      for (uint32_t q = 0; q < 4; ++q) red[q][0] += red[q][w];
      red[4][0] = red[4][w] < red[4][0] ? red[4][w] : red[4][0];
      red[5][0] = red[5][w] > red[5][0] ? red[5][w] : red[5][0];
    }
    if (blockIdx.x == 0) atomicAdd(k.stats + ISIM_ST_N_TRACES, (unsigned long long)k.n);
    atomicAdd(k.stats + ISIM_ST_SUM_LATENCY, red[0][0]);
    atomicAdd(k.stats + ISIM_ST_SUM_HOPS, red[1][0]);
    atomicAdd(k.stats + ISIM_ST_SUM_ERR_HOPS, red[2][0]);
    atomicAdd(k.stats + ISIM_ST_N_500, red[3][0]);
    if (red[4][0] != ~0ull) atomicMax(k.stats + ISIM_ST_NOT_MIN_LATENCY, ~red[4][0]);
    atomicMax(k.stats + ISIM_ST_MAX_LATENCY, red[5][0]);
  }
}

__global__ void k_flag_retry(unsigned long long *stats, const uint32_t *ovf) {
  if (ovf[2]) atomicAdd(stats + ISIM_ST_DES_RETRY, (unsigned long long)kDesFaultUnit);  // a fault: an error
  else if (ovf[0] || ovf[1]) atomicAdd(stats + ISIM_ST_DES_RETRY, 1ull);
}

// ---- 6. the span tap: the executed invocations of chosen
// traces out of the live item arrays.  The chosen ids are ascending; a trace's
// span count is its item count
struct TapK {
  const uint64_t *ids;          // [n_sel]
  const uint64_t *off;          // [n_sel + 1]: the exclusive scan of the counts
  const uint64_t *info;         // ISIM_SPAN_WRITTEN: the traces that fit (a prefix of the list)
  const uint32_t *inv;          // trace-order item -> position-major item
  const uint32_t *slot_callee;
  isim_des_span *spans;
  unsigned long long *wait;     // the wait table (null: none)
  uint32_t entry, n_services, wide;
};

__global__ void __launch_bounds__(kT) k_tap_count(K k, const uint64_t *ids, uint64_t n_sel, uint32_t *cnt,
                                                  uint64_t *info, uint64_t matches) {
  if (gid() == 0) info[ISIM_DES_SPAN_MATCHES] = matches;
  for (uint64_t i = gid(); i < n_sel; i += nthreads()) {
    const uint64_t t = ids[i] - k.trace_begin;
    cnt[i] = (uint32_t)(k.tend[t] - item_off(k, t));
  }
}

// One span per lane: span g belongs to the list entry i with off[i] <= g <
// off[i + 1] (a binary search of the small offset array), its hop is g - off[i],
// its item inv[first item of the trace + hop].  The gathers are scattered; a
// wave stores 64 consecutive 64-byte spans, each as four 16-byte stores.  Table:
// one set of atomics per span into its service's row; the entries (one per
// trace, all of one service) and the header are summed over the wave first
__global__ void __launch_bounds__(kT) k_tap_emit(K k, TapK q) {
  const uint64_t written = q.info[ISIM_SPAN_WRITTEN];
  const uint64_t total = q.off[written];
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t g0 = gid() - lane; g0 < total; g0 += nthreads()) {  // whole waves stay in the loop
    const uint64_t g = g0 + lane;
    const bool on = g < total;
    bool entry = false, st = false;
    uint64_t w = 0, dur = 0;
    if (on) {
      uint64_t lo = 0, hi = written;  // off[lo] <= g < off[hi]
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (q.off[mid] <= g) lo = mid;
        else hi = mid;
      }
      const uint32_t hop = (uint32_t)(g - q.off[lo]);
      const uint64_t trace = q.ids[lo], t = trace - k.trace_begin;
      const uint32_t j = q.inv[item_off(k, t) + hop];
      const uint32_t v = k.ipos[j], par = k.ipar[j];
      const uint64_t a = k.IA[j], S = k.IS[j], F = k.IF[j];
      entry = par == kNone;
      st = k.iown[j] != 0;
      const TreeExt x = tw::load_ext(k.ext, v);
      uint32_t slot, fl;
      if (q.wide) {
        const tw::NodeW4 nd = GNodesW{(const uint4 *)k.nodes}.load(v);
        slot = nd.slot();
        fl = nd.flags();
      } else {
        const tw::NodeW nd = GNodes{k.nodes}.load(v);
        slot = nd.slot();
        fl = nd.flags();
      }
      const uint32_t svc = entry ? q.entry : q.slot_callee[slot];
      const bool leaf = (fl & TF_LEAF) != 0;
      const uint32_t status =
          k.modeb ? spans::span_status<true>(st, leaf, (uint32_t)trace, (uint32_t)(trace >> 32), hop, fl, x.thr, k.k0, k.k1)
                  : spans::span_status<false>(st, leaf, (uint32_t)trace, (uint32_t)(trace >> 32), hop, fl, x.thr, k.k0,
                                              k.k1);
      const uint64_t H = entry ? 0ull : (uint64_t)x.H;
      uint4 *o = (uint4 *)(q.spans + g);
      o[0] = uint4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)S, (uint32_t)(S >> 32)};
      o[1] = uint4{(uint32_t)F, (uint32_t)(F >> 32), (uint32_t)H, (uint32_t)(H >> 32)};
      o[2] = uint4{hop, entry ? kNone : k.ihop[par], v, entry ? kNone : slot};
      o[3] = uint4{svc, status, (uint32_t)k.irep[j], 0u};
      w = S - a;
      dur = F - a;
      if (q.wait && !entry && svc < q.n_services) {
        unsigned long long *row = q.wait + (uint64_t)svc * ISIM_DW_ROW_WORDS;
        atomicAdd(row + ISIM_DW_INVOCATIONS, 1ull);
        if (w) {
          atomicAdd(row + ISIM_DW_WAITED, 1ull);
          atomicAdd(row + ISIM_DW_SUM_WAIT, (unsigned long long)w);
          atomicMax(row + ISIM_DW_MAX_WAIT, (unsigned long long)w);
        }
        atomicAdd(row + ISIM_DW_SUM_DURATION, (unsigned long long)dur);
        if (st) atomicAdd(row + ISIM_DW_RESP_500, 1ull);
      }
    }
    if (!q.wait) continue;
    // the entries and the header: one set of atomics per wave
    const unsigned long long n_sp = (unsigned long long)__popcll(__ballot(on));
    const unsigned long long em = __ballot(entry);
    if (!em) {
      if (lane == 0) atomicAdd(q.wait + (uint64_t)q.n_services * ISIM_DW_ROW_WORDS + ISIM_DW_H_SPANS, n_sp);
      continue;
    }
    unsigned long long sw = entry ? w : 0ull, mw = sw, sd = entry ? dur : 0ull;
    for (uint32_t d = 32; d > 0; d >>= 1) {
      sw += __shfl_xor(sw, d, 64);
      sd += __shfl_xor(sd, d, 64);
      const unsigned long long y = __shfl_xor(mw, d, 64);
      mw = y > mw ? y : mw;
    }
    const unsigned long long n_e = (unsigned long long)__popcll(em), n_w = (unsigned long long)__popcll(__ballot(entry && w)),
                             n_5 = (unsigned long long)__popcll(__ballot(entry && st));
    if (lane == 0) {
      unsigned long long *row = q.wait + (uint64_t)q.entry * ISIM_DW_ROW_WORDS;
      unsigned long long *hd = q.wait + (uint64_t)q.n_services * ISIM_DW_ROW_WORDS;
      atomicAdd(row + ISIM_DW_INVOCATIONS, n_e);
      if (n_w) {
        atomicAdd(row + ISIM_DW_WAITED, n_w);
        atomicAdd(row + ISIM_DW_SUM_WAIT, sw);
        atomicMax(row + ISIM_DW_MAX_WAIT, mw);
      }
      atomicAdd(row + ISIM_DW_SUM_DURATION, sd);
      if (n_5) atomicAdd(row + ISIM_DW_RESP_500, n_5);
      atomicAdd(hd + ISIM_DW_H_TRACES, n_e);
      atomicAdd(hd + ISIM_DW_H_SPANS, n_sp);
      atomicAdd(hd + ISIM_DW_H_SUM_LATENCY, sd);
      if (sw) atomicAdd(hd + ISIM_DW_H_SUM_WAIT, sw);
    }
  }
}

}  // namespace dit

namespace {

using namespace dit;

uint32_t grid_for(uint64_t m, uint32_t cap = 8192) {
  const uint64_t g = (m + kT - 1) / kT;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g, cap));
}
uint32_t bits_for(uint64_t v) {  // bits of the largest key v
  uint32_t b = 0;
  while (b < 64 && (v >> b)) ++b;
  return std::max<uint32_t>(b, 1);
}
size_t scan_u64_bytes(uint64_t n) {
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n,
                                rocprim::plus<uint64_t>());
  return b;
}
constexpr uint32_t kPrewalkBlocks = 2048;  // pre-walk grid (waves refill from a global batch counter)
// incremental quiet passes: chunks of 256 traces, or larger so that a chunk
// id fits 16 bits (step ops and kept orders carry it)
uint32_t chunk_shift(uint64_t n) { return std::max<uint32_t>(8u, bits_for(n) > 16u ? bits_for(n) - 16u : 0u); }

// The pre-walk variant: register frames (8 + spill, 16, 8), time width, error
// mode (mode B walks draw errors), where the nodes are read (a wide tree's
// 16-byte nodes, LDS, global memory), counting or emitting.
using PrewalkFn = void (*)(K, unsigned long long *);
enum PrewalkNodes : uint32_t { kNodesWide = 0, kNodesLds = 1, kNodesGlobal = 2 };
template <int FR, bool SP, bool T6, bool MB>
PrewalkFn prewalk_variant(PrewalkNodes nodes, bool emit) {
  static const PrewalkFn v[3][2] = {
      {k_prewalk<FR, SP, false, false, T6, MB, true>, k_prewalk<FR, SP, true, false, T6, MB, true>},
      {k_prewalk<FR, SP, false, true, T6, MB>, k_prewalk<FR, SP, true, true, T6, MB>},
      {k_prewalk<FR, SP, false, false, T6, MB>, k_prewalk<FR, SP, true, false, T6, MB>}};
  return v[nodes][emit];
}
PrewalkFn prewalk_kernel(uint32_t frames, bool t64, bool modeb, PrewalkNodes nodes, bool emit) {
  // [frames: 8 + spill, 16, 8][t64][mode B]
  static PrewalkFn (*const pick[3][2][2])(PrewalkNodes, bool) = {
      {{prewalk_variant<8, true, false, false>, prewalk_variant<8, true, false, true>},
       {prewalk_variant<8, true, true, false>, prewalk_variant<8, true, true, true>}},
      {{prewalk_variant<16, false, false, false>, prewalk_variant<16, false, false, true>},
       {prewalk_variant<16, false, true, false>, prewalk_variant<16, false, true, true>}},
      {{prewalk_variant<8, false, false, false>, prewalk_variant<8, false, false, true>},
       {prewalk_variant<8, false, true, false>, prewalk_variant<8, false, true, true>}}};
  return pick[frames > 16 ? 0 : frames > 8 ? 1 : 2][t64][modeb](nodes, emit);
}

// per-batch buffers come from the handler's private pool (DesItemsLaunch::pool:
// never the device's default pool, whose attributes belong to the application)
// and go back to it on every return
struct PoolBuf {
  void *p = nullptr;
  hipStream_t s;
  ~PoolBuf() {
    if (p) (void)hipFreeAsync(p, s);
  }
};

// One batch: the stages of the file's header comment in stream order.  Every
// stage returns 0, or the launcher's return code with the reason in `err`.
struct Batch {
  const DesItemsLaunch &L;
  const DesPlan &pl;
  hipStream_t s;
  std::string &err;
  const uint64_t n;
  const uint32_t R, G;  // rounds, finish groups
  K k{};
  ItemTraceBufs T{};
  ItemBufs B{};
  PoolBuf spill_mem, item_mem;
  DesItemsReport rep{};  // isim_des_last_batch: host synchronisations, passes, items
  size_t scan_bytes = 0, tmp_bytes = 0;
  ItemDims dims{};
  uint64_t M = 0;
  std::vector<uint64_t> row_hold;  // per duration-table row: the service's worker hold
  // worker pools (des_workers.h): per row its workers when some row has more than one (else empty), and per
  // round whether a pooled row queues in it
  std::vector<uint32_t> row_workers;
  std::vector<uint8_t> round_pooled;
  uint32_t rep_bits = 0, row_bits = 0;
  bool qscan = false, two_sorts = false, keep_ord = false;
  uint32_t qepoch = 0, qtbase = 0;  // k_qscan launches (the states' epochs: 1, 2, ...) and tickets taken
  uint32_t qn = 0;                  // k_qarr launches: the arrival-range slot alternates
  std::vector<uint32_t> qoff, foff, soff;  // item ranges of the rounds' queues, finish groups, step ops
  std::vector<uint8_t> have_ord;           // per sort round: an order is kept
  std::vector<uint64_t> rlo, rhi;          // per sort round: its arrival range over the passes

  Batch(const DesItemsLaunch &L_, hipStream_t s_, std::string &err_)
      : L(L_), pl(*L_.plan), s(s_), err(err_), n(L_.n_traces), R(pl.rounds()), G((uint32_t)pl.fin_off.size() - 1),
        spill_mem{nullptr, s_}, item_mem{nullptr, s_} {}
  ~Batch() {
    if (L.report) *L.report = rep;
  }
  int fail(const char *what) {
    err = std::string("DES items: ") + what;
    return 1;
  }
  hipError_t sync_s() {
    ++rep.syncs;
    return hipStreamSynchronize(s);
  }
  bool pool_alloc(PoolBuf &b, uint64_t bytes) {
    return hipMallocFromPoolAsync(&b.p, bytes, (hipMemPool_t)L.pool, s) == hipSuccess;
  }

  int run() {
    setup();
    if (int rc = arrivals()) return rc;
    if (int rc = count_items()) return rc;
    if (int rc = allocate()) return rc;
    if (int rc = emit_items()) return rc;
    if (int rc = renumber()) return rc;
    if (int rc = buckets()) return rc;
    if (int rc = fixed_point()) return rc;
    return finalize();
  }

  void setup() {
    Arena ws(L.workspace);
    scan_bytes = scan_u64_bytes(n);
    des_items_trace_layout(ws, T, n, scan_bytes);
    k.pos = (const DesPos *)L.d_pos;
    k.ip = (const DesItemPos *)L.d_item_pos;
    k.steps = (const DesStep *)L.d_steps;
    k.step_round = L.d_step_round;
    k.nodes = (const unsigned long long *)L.d_nodes;
    k.ext = (const TreeExt *)L.d_ext;
    k.tstep = (const TreeStep *)L.d_tstep;
    k.n_nodes = L.n_nodes;
    k.gap = T.gap;
    k.A = T.A;
    k.cnt = T.cnt;
    k.tend = T.tend;
    k.terr = T.terr;
    k.stats = (unsigned long long *)L.d_stats;
    k.table = (unsigned long long *)L.d_table;
    k.records = L.d_records;
    k.n = n;
    k.trace_begin = L.trace_begin;
    k.mean_ns = L.mean_ns;
    k.k0 = (uint32_t)L.seed;
    k.k1 = (uint32_t)(L.seed >> 32);
    k.n_slots = L.n_slots;
    k.modeb = pl.modeb ? 1u : 0u;
    k.aw = pl.item_acc;
    k.bw = pl.item_bk;
    k.cshift = chunk_shift(n);
    k.spin_limit = des_spin_limit();
    uint32_t max_reps = 1, max_row = 0;
    for (const DesPos &q : pl.pos) {
      max_reps = std::max(max_reps, q.reps);
      max_row = std::max(max_row, q.row);
    }
    rep_bits = max_reps > 1 ? bits_for(max_reps - 1) : 0u;
    row_bits = bits_for(max_row);
    row_hold.assign((size_t)max_row + 1, 0);
    for (const DesPos &q : pl.pos) row_hold[q.row] = q.hold;
    round_pooled.assign(R, 0);
    if (L.row_workers && std::any_of(L.row_workers, L.row_workers + row_hold.size(), [](uint32_t w) { return w > 1; })) {
      row_workers.assign(L.row_workers, L.row_workers + row_hold.size());
      for (size_t v = 0; v < pl.pos.size(); ++v)
        if (row_workers[pl.pos[v].row] > 1) round_pooled[pl.item_pos[v].qround] = 1;
    }
    // ISIM_FLAG_DES_TWO_SORTS: always the two-sort queue path; ISIM_FLAG_DES_SORT_ALL:
    // never reuse a kept order (independent checks)
    two_sorts = (L.flags & ISIM_FLAG_DES_TWO_SORTS) != 0;
    keep_ord = pl.cyclic && !(L.flags & ISIM_FLAG_DES_SORT_ALL);
    have_ord.assign(R, 0);
    rlo.assign(R, ~0ull);
    rhi.assign(R, 0);
  }

  // 1. arrivals
  int arrivals() {
    // under a load profile the gaps are work (Q24) and the scan's sums are mapped to times in place
    if (L.profile) {
      if (lp::work_launch(L.seed, *L.profile, L.trace_begin, n, k.gap, s)) return fail("profile work");
    } else {
      hipLaunchKernelGGL(k_gaps, dim3(grid_for(n)), dim3(kT), 0, s, k);
    }
    size_t b = scan_bytes;
    if (rocprim::inclusive_scan(T.scan_tmp, b, k.gap, k.A, (size_t)n, rocprim::plus<uint64_t>(), s) != hipSuccess)
      return fail("arrival scan");
    if (L.profile && lp::map_launch(*L.profile, n, k.A, s)) return fail("profile map");
    return 0;
  }

  // 2. the pre-walk, counting or emitting.  The nodes in LDS (1024-thread
  // workgroups, one per CU at these register counts) when they fit in 96 KB
  void prewalk(bool emit) {
    const uint32_t lds_nodes = L.n_nodes * 8u;
    const bool ldsn = !L.tree_wide && lds_nodes <= 96u * 1024u;
    const PrewalkFn kern = prewalk_kernel(L.tree_frames, L.tree_t64 != 0, pl.modeb,
                                          L.tree_wide ? kNodesWide : ldsn ? kNodesLds : kNodesGlobal, emit);
    unsigned long long *w = T.work + (emit ? 1 : 0);
    if (ldsn) {
      (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_nodes);
      hipLaunchKernelGGL(kern, dim3(kPrewalkBlocks / 4), dim3(1024), lds_nodes, s, k, w);
    } else {
      hipLaunchKernelGGL(kern, dim3(kPrewalkBlocks), dim3(kT), 0, s, k, w);
    }
  }

  // 2a. each trace's executed invocations, the item offsets, the batch's items
  int count_items() {
    const uint32_t fr = L.tree_frames;
    if (fr > 16) {  // frames past the registers spill to global memory
      const uint64_t words = (uint64_t)(fr - 8 + 1) *
                             ((L.tree_t64 ? kTreeSpillWords64 : kTreeSpillWords) + (L.tree_wide ? kTreeSpillWide : 0u)) *
                             kPrewalkBlocks * kT;
      if (!pool_alloc(spill_mem, words * 4)) return fail("spill allocation");
    }
    k.spill = (uint32_t *)spill_mem.p;
    if (hipMemsetAsync(T.work, 0, 16, s) != hipSuccess) return fail("memset");
    prewalk(false);
    size_t b = scan_bytes;
    if (rocprim::inclusive_scan(T.scan_tmp, b, k.cnt, k.tend, (size_t)n, rocprim::plus<uint64_t>(), s) != hipSuccess)
      return fail("item offset scan");
    if (hipMemcpyAsync(&M, k.tend + (n - 1), 8, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess)
      return fail("item count read-back");
    if (M >= 0xFFFFFFFFull) {
      err = "DES items: a batch of more than 2^32 - 1 executed invocations (use smaller batches)";
      return 2;
    }
    k.M = M;
    rep.items = M;
    rep.passes = 1;
    return 0;
  }

  // the per-item arrays and the rounds' sort buffers, one allocation (des_items_layout)
  int allocate() {
    // (isim_des_workers_set refuses them; their kept orders and quiet passes know no rank classes)
    if (!row_workers.empty() && pl.cyclic) return fail("worker pools on a cyclic schedule");
    size_t sort32_bytes = 0, sort64_bytes = 0, sbk_bytes = 0, sop_bytes = 0, perm_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort32_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)M, 0, 32);
    (void)rocprim::radix_sort_pairs(nullptr, sort64_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)M, 0, 64);
    (void)rocprim::inclusive_scan_by_key(nullptr, sbk_bytes, (const uint32_t *)nullptr, (const MP *)nullptr,
                                         (MP *)nullptr, (size_t)M, MPThen(), rocprim::equal_to<uint32_t>());
    if (pl.item_bk)
      (void)rocprim::radix_sort_pairs(nullptr, sop_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      (size_t)(M * pl.item_bk), 0, 32);
    (void)rocprim::radix_sort_pairs(nullptr, perm_bytes,
                                    rocprim::make_transform_iterator((const uint4 *)nullptr, PosOf()),
                                    (uint32_t *)nullptr, rocprim::make_counting_iterator<uint32_t>(0u),
                                    (uint32_t *)nullptr, (size_t)M, 0, 32);
    tmp_bytes = std::max({sort32_bytes, sort64_bytes, sbk_bytes, sop_bytes, perm_bytes});
    dims = ItemDims{M, n, k.aw, k.bw, R, row_hold.size(), pl.pos.size(), pl.cyclic, pl.modeb, tmp_bytes, k.cshift,
                    !row_workers.empty()};
    Arena sizing;
    des_items_layout(sizing, B, dims);
    if (!pool_alloc(item_mem, sizing.bytes())) return fail("item allocation");
    Arena carving(item_mem.p);
    des_items_layout(carving, B, dims);
    k.ipos = B.ipos;
    k.ipar = B.ipar;
    k.itr = B.itr;
    k.iown = B.iown;
    k.IA = B.IA;
    k.IS = B.IS;
    k.IF = B.IF;
    k.acc = B.acc;
    k.bk = B.bk;
    k.ihop = B.ihop;
    k.troot = B.troot;
    k.erec = (uint4 *)B.erec;
    k.irep = B.irep;
    k.ifst = pl.modeb ? B.ifst : nullptr;
    k.fault = B.ovf + 2;
    // the rounds' queues by k_qscan (its keys a - j h need j h < 2^62), else
    // rocPRIM's scan by key over the maps and k_qout (ISIM_FLAG_DES_SCAN_BY_KEY:
    // always, an independent check of k_qscan)
    const uint64_t max_hold = *std::max_element(row_hold.begin(), row_hold.end());
    qscan = !(L.flags & ISIM_FLAG_DES_SCAN_BY_KEY) && (max_hold == 0 || M <= (1ull << 62) / max_hold);
    return 0;
  }

  // 2b. each item's position, caller and contention-free duration
  int emit_items() {
    static const uint64_t mm_empty[8] = {~0ull, 0ull, 0ull, 0ull, ~0ull, 0ull, 0ull, 0ull};
    if (hipMemsetAsync(B.ovf, 0, 16, s) != hipSuccess ||
        hipMemcpyAsync(B.mm, mm_empty, 64, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail("memset");
    prewalk(true);
    if (hipMemsetAsync(k.terr, 0, n * 4, s) != hipSuccess) return fail("memset");
    return 0;
  }

  // 2c. renumber position-major: ipos = the sorted keys, the rest gathered
  // (keys read from the records, values counted: no key / index arrays);
  // own errors, entry items, replicas
  int renumber() {
    size_t tb = tmp_bytes;
    if (rocprim::radix_sort_pairs(B.tmp, tb, rocprim::make_transform_iterator((const uint4 *)k.erec, PosOf()), k.ipos,
                                  rocprim::make_counting_iterator<uint32_t>(0u), B.qids, (size_t)M, 0,
                                  bits_for(std::max<size_t>(1, pl.pos.size()) - 1), s) != hipSuccess)
      return fail("position sort");
    hipLaunchKernelGGL(k_perm_inv, dim3(grid_for(M)), dim3(kT), 0, s, k, B.qids, B.inv);
    hipLaunchKernelGGL(k_own, dim3(grid_for(M)), dim3(kT), 0, s, k, (const uint32_t *)B.inv);
    hipLaunchKernelGGL(k_root500, dim3(grid_for(n)), dim3(kT), 0, s, k);
    hipLaunchKernelGGL(k_perm_apply, dim3(grid_for(M)), dim3(kT), 0, s, k, B.qids);
    if (pl.modeb) {
      if (hipMemsetAsync(B.ifst, 0xFF, M * 4, s) != hipSuccess) return fail("memset");
      hipLaunchKernelGGL(k_fail, dim3(grid_for(M)), dim3(kT), 0, s, k);
    }
    hipLaunchKernelGGL(k_roots, dim3(grid_for(n)), dim3(kT), 0, s, k, B.inv);
    hipLaunchKernelGGL(k_reps, dim3(grid_for(M)), dim3(kT), 0, s, k);
    if (pl.cyclic) {  // the first pass's cut step begins: contention-free callee maxima (k_relmax)
      if (hipMemsetAsync(k.acc, 0, M * 8 * k.aw, s) != hipSuccess) return fail("memset");
      hipLaunchKernelGGL(k_relmax, dim3(grid_for(M)), dim3(kT), 0, s, k, B.qids, (unsigned long long *)k.acc);
    }
    return 0;
  }

  // 3. buckets: the rounds' and finish groups' item lists, the step-begin ops by round
  int buckets() {
    if (hipMemcpyAsync(B.d_row_hold, row_hold.data(), row_hold.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail("hold table upload");
    k.row_hold = B.d_row_hold;
    if (!row_workers.empty() && hipMemcpyAsync(B.d_row_workers, row_workers.data(), row_workers.size() * 4,
                                               hipMemcpyHostToDevice, s) != hipSuccess)
      return fail("worker table upload");
    // the step-begin ops; each position's item range (k.ipos is sorted)
    hipLaunchKernelGGL(k_bucket_keys, dim3(grid_for(M)), dim3(kT), 0, s, k, B.op_k, B.op_v, B.ovf + 3);
    const uint32_t NP = (uint32_t)pl.pos.size();
    hipLaunchKernelGGL(k_bounds, dim3(grid_for(M + 1)), dim3(kT), 0, s, (const uint32_t *)k.ipos, M, NP, 0u, B.d_poff);
    uint32_t n_ops = 0;
    std::vector<uint32_t> poff(NP + 1);
    if (hipMemcpyAsync(&n_ops, B.ovf + 3, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(poff.data(), B.d_poff, (NP + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        sync_s() != hipSuccess)
      return fail("bucket read-back");
    // the rounds' and groups' lists: positions in increasing order within each
    std::vector<uint32_t> qdst(NP), fdst(NP);
    std::vector<uint64_t> qc(R + 1, 0), fc(G + 1, 0);
    for (uint32_t v = 0; v < NP; ++v) {
      qc[pl.item_pos[v].qround + 1] += poff[v + 1] - poff[v];
      fc[pl.item_pos[v].fgroup + 1] += poff[v + 1] - poff[v];
    }
    for (uint32_t r = 0; r < R; ++r) qc[r + 1] += qc[r];
    for (uint32_t g = 0; g < G; ++g) fc[g + 1] += fc[g];
    qoff.assign(qc.begin(), qc.end());
    foff.assign(fc.begin(), fc.end());
    for (uint32_t v = 0; v < NP; ++v) {
      const uint32_t c = poff[v + 1] - poff[v];
      qdst[v] = (uint32_t)qc[pl.item_pos[v].qround];
      qc[pl.item_pos[v].qround] += c;
      fdst[v] = (uint32_t)fc[pl.item_pos[v].fgroup];
      fc[pl.item_pos[v].fgroup] += c;
    }
    if (hipMemcpyAsync(B.d_qdst, qdst.data(), NP * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(B.d_fdst, fdst.data(), NP * 4, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail("list upload");
    hipLaunchKernelGGL(k_scatter_ids, dim3(grid_for(M)), dim3(kT), 0, s, k, B.d_poff, B.d_qdst, B.d_fdst, B.qids,
                       B.fids);
    soff.assign(R + 1, 0);
    if (n_ops) {
      size_t tb = tmp_bytes;
      if (rocprim::radix_sort_pairs(B.tmp, tb, B.op_k, B.op_k2, B.op_v, B.op_v2, (size_t)n_ops, 0, bits_for(R), s) !=
          hipSuccess)
        return fail("step-op sort");
      hipLaunchKernelGGL(k_bounds, dim3(grid_for(n_ops + 1)), dim3(kT), 0, s, B.op_k2, (uint64_t)n_ops, R, 0u,
                         B.d_soff);
      if (hipMemcpyAsync(soff.data(), B.d_soff, (R + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
          sync_s() != hipSuccess)
        return fail("step-op offsets read-back");
    }
    return 0;
  }

  // 4b. the queues of round r (its m > 0 items): arrivals, the FIFO order
  // (kept, in list order, one sort or two), one segmented max-plus scan.
  // Returns early, with the starts as they are, when a quiet pass finds every
  // arrival of the round unchanged.
  int round_queue(K &kk, uint32_t r, uint64_t m, uint32_t span) {
    uint32_t *const list = B.qids + qoff[r], *const ord = B.ord + qoff[r];
    uint16_t *const ordc = B.ordc + qoff[r];
    const bool nosort = pl.round_nosort[r] && !two_sorts;
    // (a no-sort round reads no arrival range back; k_qscan computes its arrivals)
    uint64_t *slot = B.mm + 4 * (qn & 1u), *slot_next = B.mm + 4 * ((qn + 1) & 1u);
    const bool chk = !nosort && have_ord[r];
    // a pooled round (des_workers.h) builds k_pairs*'s arrays whatever scans them: they are what it refines;
    // `direct`: k_qscan reads the round's order itself
    const bool pooled = round_pooled[r] != 0;
    const bool direct = qscan && !pooled;
    if (!(nosort && direct)) {
      ++qn;
      hipLaunchKernelGGL(k_qarr, dim3(grid_for(m)), dim3(kT), 0, s, kk, list, m, (unsigned long long *)slot,
                         (unsigned long long *)slot_next);
      if (chk)  // (its flag in the same slot: one read-back)
        hipLaunchKernelGGL(k_ordchk, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint32_t *)list,
                           (const uint32_t *)ord, (const uint16_t *)ordc, m, (unsigned long long *)slot);
    }
    // a quiet pass after the first: a round whose arrivals all equal the
    // previous pass's keeps its starts (its queues are skipped)
    // (sort rounds only: they read the range back anyway; a sort-free
    // round would pay a stream synchronisation for the check)
    const bool may_skip = kk.quiet && !kk.first && !nosort;
    // range, change flag, kept-order flag (k_ordchk)
    uint64_t hmm[4] = {0, 0, 1, 1};
    if ((!nosort || may_skip) &&
        (hipMemcpyAsync(hmm, slot, 32, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess))
      return fail("arrival range read-back");
    const bool bad = hmm[3] != 0;
    if (may_skip && !hmm[2]) return 0;
    if (!nosort) {
      // the round's arrival range over the passes: the items a pass does
      // not recompute keep their arrivals (a superset range is a valid key)
      rlo[r] = std::min<uint64_t>(rlo[r], hmm[0]);
      rhi[r] = std::max<uint64_t>(rhi[r], hmm[1]);
      hmm[0] = rlo[r];
      hmm[1] = rhi[r];
    }
    const uint32_t ab = bits_for(hmm[1] - hmm[0]);
    size_t tb = tmp_bytes;
    // k_qscan's source of the round's order (k_pairs* only for the two-sort path)
    QSrc qsrc{list, ord, B.key_b, B.val_b, hmm[0], rep_bits, ab, B.rk_a, B.rk_b, B.sid, B.mp_in};
    int qsk = kQArrays;
    if (chk && !bad) {  // the kept order holds: no sort
      qsk = kQKept;
      if (!direct)
        hipLaunchKernelGGL(k_pairs1o, dim3(grid_for(m)), dim3(kT), 0, s, kk, m, (const uint32_t *)ord,
                           (const uint32_t *)list, rep_bits, B.rk_a, B.rk_b, B.mp_in, B.sid);
    } else if (nosort) {
      qsk = kQList;
      if (!direct)  // k_qscan reads the list itself
        hipLaunchKernelGGL(k_pairs0, dim3(grid_for(m)), dim3(kT), 0, s, kk, list, m, B.rk_a, B.rk_b, B.mp_in, B.sid);
    } else if (!two_sorts && row_bits + rep_bits + ab <= 64) {
      hipLaunchKernelGGL(k_qkey1, dim3(grid_for(m)), dim3(kT), 0, s, kk, list, m, hmm[0], rep_bits, ab, B.key_a,
                         B.val_a);
      if (rocprim::radix_sort_pairs(B.tmp, tb, B.key_a, B.key_b, B.val_a, B.val_b, (size_t)m, 0,
                                    row_bits + rep_bits + ab, s) != hipSuccess)
        return fail("queue sort");
      hipLaunchKernelGGL(k_tiefix<true>, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint64_t *)B.key_b, B.val_b, m,
                         (const uint32_t *)list);
      if (keep_ord) {  // the next pass checks this order first
        hipLaunchKernelGGL(k_keep_ord, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint32_t *)B.val_b,
                           (const uint32_t *)list, m, ord, ordc);
        have_ord[r] = 1;
      }
      qsk = kQSorted;
      if (!direct)
        hipLaunchKernelGGL(k_pairs1, dim3(grid_for(m)), dim3(kT), 0, s, kk, m, B.key_b, B.val_b,
                           (const uint32_t *)list, rep_bits, ab, hmm[0], B.rk_a, B.rk_b, B.mp_in, B.sid);
    } else {
      hipLaunchKernelGGL(k_qkey2, dim3(grid_for(m)), dim3(kT), 0, s, kk, list, m, hmm[0], rep_bits, B.key_a, B.val_a,
                         B.ovf);
      if (rocprim::radix_sort_pairs(B.tmp, tb, B.key_a, B.key_b, B.val_a, B.val_b, (size_t)m, 0, 64, s) != hipSuccess)
        return fail("arrival sort");
      // ties of (replica, arrival) by (trace, hop); the stable row sort keeps them
      hipLaunchKernelGGL(k_tiefix<false>, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint64_t *)B.key_b, B.val_b, m,
                         (const uint32_t *)nullptr);
      hipLaunchKernelGGL(k_rkeys, dim3(grid_for(m)), dim3(kT), 0, s, kk, B.val_b, m, B.rk_a, B.rv_a);
      tb = tmp_bytes;
      if (rocprim::radix_sort_pairs(B.tmp, tb, B.rk_a, B.rk_b, B.rv_a, B.rv_b, (size_t)m, 0, row_bits, s) != hipSuccess)
        return fail("service sort");
      hipLaunchKernelGGL(k_pairs2, dim3(grid_for(m)), dim3(kT), 0, s, kk, m, B.rk_b, B.rv_b, B.key_b, B.val_b, rep_bits,
                         B.rk_a, B.mp_in, B.sid);
    }
    const uint32_t *seg_keys = B.rk_a, *seg_rows = B.rk_b, *seg_items = B.sid;
    const MP *seg_maps = B.mp_in;
    if (pooled) {  // the order refined: every (row, replica) segment as its rank classes, each a segment
      const uint32_t wt = (uint32_t)((m + kWkTile - 1) / kWkTile);
      hipLaunchKernelGGL(k_wk_tile, dim3(wt), dim3(kT), 0, s, (const uint32_t *)B.rk_a, m, B.wk_tile);
      hipLaunchKernelGGL(k_wk_carry, dim3(1), dim3(kT), 0, s, B.wk_tile, wt);
      hipLaunchKernelGGL(k_wk_rank, dim3(wt), dim3(kT), 0, s, (const uint32_t *)B.rk_a, m,
                         (const uint32_t *)B.wk_tile, B.wk_start, B.wk_len);
      hipLaunchKernelGGL(k_wk_scatter, dim3(grid_for(m)), dim3(kT), 0, s,
                         WkArrays{B.rk_a, B.rk_b, B.sid, B.mp_in, B.wk_start, B.wk_len, B.d_row_workers, B.wk_seg,
                                  B.wk_row, B.wk_sid, B.wk_mp},
                         m);
      seg_keys = B.wk_seg, seg_rows = B.wk_row, seg_items = B.wk_sid, seg_maps = B.wk_mp;
      qsrc.segk = seg_keys, qsrc.rowk = seg_rows, qsrc.sid = seg_items, qsrc.mp = seg_maps;
      qsk = kQArrays;
    }
    if (qscan) {
      // 8 items per lane on a large round, 2 otherwise (more tiles to spread)
      const bool big = m >= 2048ull * 512;
      const uint32_t tiles = (uint32_t)((m + (big ? 2047 : 511)) / (big ? 2048 : 512));
      if (qtbase > 0xFFFFFFFFu - tiles) {  // the ticket counter restarts
        if (hipMemsetAsync(B.qticket, 0, 4, s) != hipSuccess) return fail("memset");
        qtbase = 0;
      }
      ++qepoch;
      static void (*const qs_k[2][4])(K, uint64_t, QSrc, QState *, uint32_t *, uint32_t, uint32_t) = {
          {k_qscan<2, kQArrays>, k_qscan<2, kQList>, k_qscan<2, kQKept>, k_qscan<2, kQSorted>},
          {k_qscan<8, kQArrays>, k_qscan<8, kQList>, k_qscan<8, kQKept>, k_qscan<8, kQSorted>}};
      hipLaunchKernelGGL(qs_k[big][qsk], dim3(tiles), dim3(kT), 0, s, kk, m, qsrc, B.qstate, B.qticket, qtbase, qepoch);
      qtbase += tiles;
    } else {
      tb = tmp_bytes;
      if (rocprim::inclusive_scan_by_key(B.tmp, tb, seg_keys, seg_maps, B.mp_out, (size_t)m, MPThen(),
                                         rocprim::equal_to<uint32_t>(), s) != hipSuccess)
        return fail("queue scan");
      hipLaunchKernelGGL(k_qout, dim3(grid_for((m + span - 1) / span)), dim3(kT), 0, s, kk, m, seg_rows, seg_items,
                         seg_maps, B.mp_out, span);
    }
    return 0;
  }

  // 4. one pass over the rounds: step begins (4a), queues (4b), finishes (4c).
  // Callee maxima restart from zero for every item a pass recomputes (a
  // start can move down when the order of a queue changes, so maxima are
  // never carried over); a cut step begin reads the last computed ones
  // (k_acc_init moves them to acc_prev)
  int pass(K &kk) {
    hipLaunchKernelGGL(k_acc_init, dim3(grid_for(M)), dim3(kT), 0, s, kk, pl.cyclic ? B.acc_b : nullptr, kk.acc);
    // items per lane of k_qout / k_fin: runs of one row / position summed
    // before the statistics atomics; a quiet pass records none, and one item
    // per lane gives its finish groups (~0.8 M items on c4d) 16x the waves
    const uint32_t span = kk.quiet ? 1u : kQSpan;
    for (uint32_t r = 0; r < R; ++r) {
      if (soff[r + 1] > soff[r])
        hipLaunchKernelGGL(k_steps, dim3(grid_for(soff[r + 1] - soff[r])), dim3(kT), 0, s, kk, B.op_v2 + soff[r],
                           (uint64_t)(soff[r + 1] - soff[r]));
      if (const uint64_t m = qoff[r + 1] - qoff[r]) {
        if (int rc = round_queue(kk, r, m, span)) return rc;
      }
      for (uint32_t gi = pl.fin_round_off[r]; gi < pl.fin_round_off[r + 1]; ++gi) {
        const uint64_t mg = foff[gi + 1] - foff[gi];
        if (mg) hipLaunchKernelGGL(k_fin, dim3(grid_for((mg + span - 1) / span)), dim3(kT), 0, s, kk,
                                   B.fids + foff[gi], mg, span);  // grid_for(ceil(mg / span)) blocks of kT: >= the chunks
      }
    }
    return 0;
  }

  // A cyclic schedule: quiet passes from zero (a lower bound of every time:
  // the iteration only raises values) until no stored value changes, then the
  // pass that records the statistics (des.hip des_launch).  After the first
  // pass a quiet pass recomputes only the items of the traces the previous
  // pass changed (k.dcur, k.dcur_t)
  int fixed_point() {
    // k_qscan's states and ticket
    if (qscan && (hipMemsetAsync(B.qstate, 0, (M + kQTile - 1) / kQTile * sizeof(QState), s) != hipSuccess ||
                  hipMemsetAsync(B.qticket, 0, 4, s) != hipSuccess))
      return fail("memset");
    if (pl.cyclic) {
      if (hipMemsetAsync(k.IS, 0, M * 8, s) != hipSuccess || hipMemsetAsync(k.IF, 0, M * 8, s) != hipSuccess ||
          (k.bw && hipMemsetAsync(k.bk, 0, M * 8 * k.bw, s) != hipSuccess))
        return fail("memset");
      K kq = k;
      kq.quiet = 1;
      kq.acc_prev = B.acc_b;
      kq.changed = B.chg;
      uint32_t p = 0;
      for (; p < kMaxPasses; ++p) {
        uint32_t changed[2] = {1, 0};
        if (hipMemsetAsync(kq.changed, 0, 8, s) != hipSuccess ||
            hipMemsetAsync(B.chg_b, 0, dims.n_chunks(), s) != hipSuccess ||
            hipMemsetAsync(B.chg_tb, 0, n, s) != hipSuccess)
          return fail("memset");
        kq.first = p == 0 ? 1u : 0u;
        // the first pass recomputes everything; later ones the chunks the
        // previous pass changed
        kq.dcur = p == 0 ? nullptr : B.chg_a;
        kq.dnext = B.chg_b;
        kq.dcur_t = B.chg_ta;
        kq.dnext_t = B.chg_tb;
        if (int rc = pass(kq)) return rc;
        std::swap(B.chg_a, B.chg_b);
        std::swap(B.chg_ta, B.chg_tb);
        if (hipMemcpyAsync(changed, kq.changed, 8, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess)
          return fail("fixed-point read-back");
        rep.passes = p + 2;  // the quiet passes so far and the recording pass
        if (!changed[0]) break;
      }
      if (p == kMaxPasses) {
        static const uint32_t one = 1;
        if (hipMemcpyAsync(B.ovf + 1, &one, 4, hipMemcpyHostToDevice, s) != hipSuccess) return fail("flag");
      }
    }
    k.acc_prev = B.acc_b;
    return pass(k);  // dcur null: every item
  }

  // 5. records and statistics
  int finalize() {
    hipLaunchKernelGGL(k_final, dim3(grid_for(n, 1024)), dim3(kT), 0, s, k);
    hipLaunchKernelGGL(k_flag_retry, dim3(1), dim3(1), 0, s, k.stats, B.ovf);
    if (hipGetLastError() != hipSuccess) return fail("kernel launch");
    // a look-back that gave up (k_qscan) fails the batch loudly: nothing was
    // accumulated (k_final) and the call returns the error
    uint32_t ovf[3] = {0, 0, 0};  // key overflow, no fixed point (k_flag_retry counted them), look-back fault
    if (hipMemcpyAsync(ovf, B.ovf, 12, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess)
      return fail("fault read-back");
    if (ovf[2]) {
      if (L.tap) (void)tap_none();
      return fail("a queue scan's look-back gave up waiting for an earlier tile (k_qscan): the batch was not "
                  "accumulated");
    }
    if (!L.tap) return 0;
    return ovf[0] || ovf[1] ? tap_none() : tap();
  }

  // 6. the span tap.  A batch that is not accumulated (a fault, ISIM_ST_DES_RETRY) has no trace chosen:
  // d_off[0] = 0, d_info of an empty list, nothing else
  int tap_none() { return des_items_tap_none(*L.tap, s) ? fail("tap launch") : 0; }

  // The chosen traces (the threshold given, or this batch's order statistic: §13's select and one word read
  // back), their ids by the selection of spans.hip, the counts scanned by its scan, the spans and the table
  int tap() {
    const isim_des_tap &tp = *L.tap;
    const uint64_t bound = std::min<uint64_t>(tp.max_traces, n);  // no more traces than the batch has
    uint64_t qws_bytes = 0;
    if (isim_quantiles_workspace_bytes(1, &qws_bytes) != ISIM_OK) return fail("tap workspace");
    struct {
      uint64_t *qout, *sel, *tile;
      uint32_t *cnt;
      void *qws;
    } W{};
    auto layout = [&](Arena &a) {
      W.qout = a.take<uint64_t>(ISIM_Q_OUT_WORDS(1));
      W.sel = a.take<uint64_t>(2);
      W.tile = a.take<uint64_t>(spans::tiles_of(n) + 1);  // the selection's tiles over n, then the scan's over the list
      W.cnt = a.take<uint32_t>(bound);
      W.qws = a.take<char>(qws_bytes);
    };
    Arena sizing;
    layout(sizing);
    PoolBuf mem{nullptr, s};
    if (!pool_alloc(mem, sizing.bytes())) return fail("tap allocation");
    Arena carving(mem.p);
    layout(carving);
    uint64_t thr = tp.min_latency_ns;
    if (tp.q_ppm) {
      const uint32_t q = tp.q_ppm;
      if (isim_latency_quantiles_device(k.records, n, &q, 1, W.qout, W.qws, qws_bytes, s) != ISIM_OK)
        return fail("tap: the percentile select was refused");
      if (hipMemcpyAsync(&thr, W.qout + (uint64_t)tp.cls * 2 + 1, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
          sync_s() != hipSuccess)
        return fail("tap threshold read-back");
    }
    if (spans::select_launch(k.records, n, L.trace_begin, thr, tp.cls, tp.max_traces, tp.d_ids, W.sel, W.tile, s) !=
        ISIM_OK)
      return fail("tap selection launch");
    uint64_t sel[2] = {0, 0};  // matches, written
    if (hipMemcpyAsync(sel, W.sel, 16, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess)
      return fail("tap selection read-back");
    const uint64_t n_sel = sel[1];
    hipLaunchKernelGGL(k_tap_count, dim3(grid_for(n_sel)), dim3(kT), 0, s, k, (const uint64_t *)tp.d_ids, n_sel, W.cnt,
                       tp.d_info, sel[0]);
    if (spans::scan_launch(W.cnt, n_sel, W.tile, tp.d_off, tp.cap_spans, tp.d_info, s) != ISIM_OK)
      return fail("tap scan launch");
    if (n_sel && tp.cap_spans) {
      TapK q{};
      q.ids = tp.d_ids;
      q.off = tp.d_off;
      q.info = tp.d_info;
      q.inv = B.inv;
      q.slot_callee = L.d_slot_callee;
      q.spans = tp.d_spans;
      q.wait = (unsigned long long *)tp.d_wait_table;
      q.entry = L.entry_service;
      q.n_services = L.n_services;
      q.wide = L.tree_wide;
      hipLaunchKernelGGL(k_tap_emit, dim3(grid_for(std::min<uint64_t>(tp.cap_spans, M))), dim3(kT), 0, s, k, q);
    }
    if (hipGetLastError() != hipSuccess) return fail("tap launch");
    // the pool takes the buffers back in stream order, after the kernels above
    return 0;
  }
};

}  // namespace

uint64_t des_items_workspace_bytes(uint64_t n) {
  Arena sizing;
  ItemTraceBufs t;
  des_items_trace_layout(sizing, t, n, scan_u64_bytes(n));
  return sizing.bytes();
}

int des_items_tap_none(const isim_des_tap &tap, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (spans::scan_launch(nullptr, 0, nullptr, tap.d_off, tap.cap_spans, tap.d_info, s) != ISIM_OK) return 1;
  hipLaunchKernelGGL(dit::k_tap_count, dim3(1), dim3(dit::kT), 0, s, dit::K{}, (const uint64_t *)nullptr, 0ull,
                     (uint32_t *)nullptr, tap.d_info, 0ull);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int des_items_launch(const DesItemsLaunch &L, void *stream, std::string &err) {
  return Batch(L, (hipStream_t)stream, err).run();
}

}  // namespace isim
