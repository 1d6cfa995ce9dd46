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

#include "des_items_k.h"

// ---- 1. the exponential inter-arrival gaps (summed by a rocPRIM scan)
__global__ void __launch_bounds__(kT) k_gaps(K k) {
  for (uint64_t t = gid(); t < k.n; t += nthreads())
    k.gap[t] = (k.mean_ns * exp_q24(draw0(k.trace_begin + t, 0u, 0x80000001u, k.k0, k.k1))) >> 24;
}

#include "des_items_prewalk.h"

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

#include "des_items_queue.h"
#include "des_items_fin.h"
#include "des_items_tap.h"

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
  // What the steps of one round share:
  struct Round {
    uint32_t r;
    uint64_t m;
    uint32_t *list, *ord;  // the round's items; its kept order (list indices) and the items' trace chunks
    uint16_t *ordc;
    bool nosort;         // its list is its FIFO order (DesPlan::round_nosort)
    bool pooled;         // a row with several workers queues in it (des_workers.h)
    bool direct;         // k_qscan reads the order at its source: no arrays, and no k_qarr for a list
    bool chk;            // a kept order is checked first (k_ordchk)
    uint64_t *slot;      // k_qarr's words of this round, and what the host read of them:
    uint64_t hmm[4];     // the arrival range, the change flag, k_ordchk's flag
    bool unchanged;      // a quiet pass found every arrival as it was: the starts stand
    int src;             // kQ*: where the order is (round_order)
    QSrc q;              // the order for the kernel that reads it
  };

  int round_queue(K &kk, uint32_t r, uint64_t m, uint32_t span) {
    Round q{};
    q.r = r, q.m = m;
    q.list = B.qids + qoff[r], q.ord = B.ord + qoff[r], q.ordc = B.ordc + qoff[r];
    q.nosort = pl.round_nosort[r] && !two_sorts;
    q.pooled = round_pooled[r] != 0;
    q.direct = qscan && !q.pooled;
    q.chk = !q.nosort && have_ord[r];
    if (int rc = round_arrivals(kk, q)) return rc;
    if (q.unchanged) return 0;
    if (int rc = round_order(kk, q)) return rc;
    if (!q.direct && q.src != kQArrays) round_arrays(kk, q);
    if (q.pooled) round_refine(q);
    return round_scan(kk, q, span);
  }

  // the items' arrivals (k_qarr) and, for a sort round, their range read back.
  // A list that k_qscan reads itself launches nothing: k_qscan computes the
  // arrivals.  A quiet pass after the first keeps the starts of a round whose
  // arrivals all equal the previous pass's (sort rounds only: they read the
  // range back anyway; a sort-free round would pay a stream synchronisation
  // for the check)
  int round_arrivals(K &kk, Round &q) {
    q.slot = B.mm + 4 * (qn & 1u);
    uint64_t *const slot_next = B.mm + 4 * ((qn + 1) & 1u);
    if (!(q.nosort && q.direct)) {
      ++qn;
      hipLaunchKernelGGL(k_qarr, dim3(grid_for(q.m)), dim3(kT), 0, s, kk, q.list, q.m, (unsigned long long *)q.slot,
                         (unsigned long long *)slot_next);
      if (q.chk)  // (its flag in the same slot: one read-back)
        hipLaunchKernelGGL(k_ordchk, dim3(grid_for(q.m)), dim3(kT), 0, s, kk, (const uint32_t *)q.list,
                           (const uint32_t *)q.ord, (const uint16_t *)q.ordc, q.m, (unsigned long long *)q.slot);
    }
    q.hmm[0] = q.hmm[1] = 0, q.hmm[2] = q.hmm[3] = 1;
    if (q.nosort) return 0;
    if (hipMemcpyAsync(q.hmm, q.slot, 32, hipMemcpyDeviceToHost, s) != hipSuccess || sync_s() != hipSuccess)
      return fail("arrival range read-back");
    if (kk.quiet && !kk.first && !q.hmm[2]) {
      q.unchanged = true;
      return 0;
    }
    // the round's arrival range over the passes: the items a pass does
    // not recompute keep their arrivals (a superset range is a valid key)
    rlo[q.r] = std::min<uint64_t>(rlo[q.r], q.hmm[0]);
    rhi[q.r] = std::max<uint64_t>(rhi[q.r], q.hmm[1]);
    q.hmm[0] = rlo[q.r];
    q.hmm[1] = rhi[q.r];
    return 0;
  }

  // where the round's FIFO order is: the kept order when it still holds, the
  // list itself, one sort (row | replica | arrival in 64 bits) or two, which
  // leave arrays
  int round_order(K &kk, Round &q) {
    const uint64_t m = q.m, amin = q.hmm[0];
    const uint32_t ab = bits_for(q.hmm[1] - amin);
    q.q = QSrc{q.list, q.ord, B.key_b, B.val_b, amin, rep_bits, ab, B.rk_a, B.rk_b, B.sid, B.mp_in};
    size_t tb = tmp_bytes;
    if (q.chk && !q.hmm[3]) {  // the kept order holds: no sort
      q.src = kQKept;
    } else if (q.nosort) {
      q.src = kQList;
    } else if (!two_sorts && row_bits + rep_bits + ab <= 64) {
      hipLaunchKernelGGL(k_qkey1, dim3(grid_for(m)), dim3(kT), 0, s, kk, q.list, m, amin, rep_bits, ab, B.key_a,
                         B.val_a);
      if (rocprim::radix_sort_pairs(B.tmp, tb, B.key_a, B.key_b, B.val_a, B.val_b, (size_t)m, 0,
                                    row_bits + rep_bits + ab, s) != hipSuccess)
        return fail("queue sort");
      hipLaunchKernelGGL(k_tiefix<true>, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint64_t *)B.key_b, B.val_b, m,
                         (const uint32_t *)q.list);
      if (keep_ord) {  // the next pass checks this order first
        hipLaunchKernelGGL(k_keep_ord, dim3(grid_for(m)), dim3(kT), 0, s, kk, (const uint32_t *)B.val_b,
                           (const uint32_t *)q.list, m, q.ord, q.ordc);
        have_ord[q.r] = 1;
      }
      q.src = kQSorted;
    } else {
      hipLaunchKernelGGL(k_qkey2, dim3(grid_for(m)), dim3(kT), 0, s, kk, q.list, m, amin, rep_bits, B.key_a, B.val_a,
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
      q.src = kQArrays;  // (the rows: the second sort's keys, B.rk_b)
    }
    return 0;
  }

  // the order as arrays, when something other than k_qscan reads it: the scan
  // by key, or a pooled round's refinement
  void round_arrays(K &kk, Round &q) {
    static void (*const pairs[4])(K, uint64_t, QSrc, uint32_t *, uint32_t *, MP *, uint32_t *) = {
        nullptr, k_pairs<kQList>, k_pairs<kQKept>, k_pairs<kQSorted>};
    hipLaunchKernelGGL(pairs[q.src], dim3(grid_for(q.m)), dim3(kT), 0, s, kk, q.m, q.q, B.rk_a, B.rk_b, B.mp_in,
                       B.sid);
  }

  // a pooled round: every (row, replica) segment of the arrays as its rank classes, each a segment
  void round_refine(Round &q) {
    const uint64_t m = q.m;
    const uint32_t wt = (uint32_t)((m + kWkTile - 1) / kWkTile);
    hipLaunchKernelGGL(k_wk_tile, dim3(wt), dim3(kT), 0, s, (const uint32_t *)B.rk_a, m, B.wk_tile);
    hipLaunchKernelGGL(k_wk_carry, dim3(1), dim3(kT), 0, s, B.wk_tile, wt);
    hipLaunchKernelGGL(k_wk_rank, dim3(wt), dim3(kT), 0, s, (const uint32_t *)B.rk_a, m, (const uint32_t *)B.wk_tile,
                       B.wk_start, B.wk_len);
    hipLaunchKernelGGL(k_wk_scatter, dim3(grid_for(m)), dim3(kT), 0, s,
                       WkArrays{B.rk_a, B.rk_b, B.sid, B.mp_in, B.wk_start, B.wk_len, B.d_row_workers, B.wk_seg,
                                B.wk_row, B.wk_sid, B.wk_mp},
                       m);
    q.q.segk = B.wk_seg, q.q.rowk = B.wk_row, q.q.sid = B.wk_sid, q.q.mp = B.wk_mp;
  }

  // the starts and the queue figures: k_qscan over the order's source or the
  // arrays, else rocPRIM's scan by key over the arrays' maps and k_qout
  int round_scan(K &kk, Round &q, uint32_t span) {
    const uint64_t m = q.m;
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
      hipLaunchKernelGGL(qs_k[big][q.direct ? q.src : kQArrays], dim3(tiles), dim3(kT), 0, s, kk, m, q.q, B.qstate,
                         B.qticket, qtbase, qepoch);
      qtbase += tiles;
    } else {
      size_t tb = tmp_bytes;
      if (rocprim::inclusive_scan_by_key(B.tmp, tb, q.q.segk, q.q.mp, B.mp_out, (size_t)m, MPThen(),
                                         rocprim::equal_to<uint32_t>(), s) != hipSuccess)
        return fail("queue scan");
      hipLaunchKernelGGL(k_qout, dim3(grid_for((m + span - 1) / span)), dim3(kT), 0, s, kk, m, q.q.rowk, q.q.sid,
                         q.q.mp, B.mp_out, span);
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
