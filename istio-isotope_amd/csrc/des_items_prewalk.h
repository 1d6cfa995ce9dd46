// DES item engine, stages 2, 2a, 2b: the pre-walk
// that counts and emits the items, their own errors, the position-major
// renumbering, and what is drawn or derived once per batch from it (failed
// steps, contention-free maxima, entry items, replicas).  A part of
// des_items.hip, included inside namespace isim::dit after des_items_k.h.
#pragma once

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

// each item's replica (the oracle's draw at its hop), once per batch
__global__ void __launch_bounds__(kT) k_reps(K k) {
  for (uint64_t i = gid(); i < k.M; i += nthreads()) {
    const DesPos P = k.pos[k.ipos[i]];
    uint32_t rep = 0;
    if (P.reps > 1) rep = draw0(k.trace_begin + k.itr[i], k.ihop[i], 0x80000002u, k.k0, k.k1) % P.reps;
    k.irep[i] = (uint16_t)rep;
  }
}
