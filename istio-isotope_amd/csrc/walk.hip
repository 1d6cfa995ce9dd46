// isim_walk — the hot path on gfx950 (CDNA4): one wavefront simulates 64
// independent request traces (one per lane) by interpreting the flattened
// service scripts of program.h in lock-step.  Semantics: "isim semantics v1"
// (DESIGN.md §2), i.e. isotope's Handler.ServeHTTP / execute recursion
// (isotope/service/pkg/srv/handler.go:37-79, executable.go:43-179) in virtual
// integer-nanosecond time.
//
// Execution model:
//  * The program counter, the current instruction and the call depth are
//    wave-uniform (SGPRs).  The next instruction is known before the current
//    one executes (pc+1, a CALL's target, or the return pc of a RET), so the
//    loop issues one s_load_dwordx16 of [npc-1, npc] first and consumes it on
//    the next iteration; for a RET the first half is the CALL record.
//  * Per-lane booleans — "this lane's trace executes the current invocation",
//    "a step failed", "error in the current concurrent step", "this
//    invocation's own error draw" — are 64-bit lane masks in SGPRs.
//  * STATIC walks (no probabilistic calls, no mode-B abort that could skip a
//    step) execute the identical invocation sequence in every lane, so virtual
//    time and hop ids are wave-uniform (SGPRs); the per-lane work is the
//    Philox error draws, the status masks and the per-trace error count.
//    Other walks keep time (u32 or u64 by the program's latency bound) and
//    hop ids per lane.
//  * Call frames: wave-uniform parts live in VGPR lanes (lane d holds frame
//    d: v_writelane / v_readlane); per-lane time and hop of dynamic walks go
//    to an LDS stack [frame][lane].
//  * Error draws: word (h&3) of Philox4x32-10((t_lo, t_hi, h>>2, 0), seed):
//    one block serves four consecutive invocations of a lane.
//  * Per-call-site counters (executed calls, callee 500s) are one ds_add per
//    instruction per wave into a workgroup LDS table, flushed to HBM with
//    global atomics once per workgroup; latency histograms are reduced per
//    64-trace batch with a wave "match" loop.
// The draw-stream walks (kernel kinds 4, 5, 6 and 8: static walks laid out in
// hop order, no interpreter) are in stream_walk.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernel_abi.h"
#include "stream_walk.h"
#include "walk_dev.h"

#ifndef ISIM_STREAM_TPL
#define ISIM_STREAM_TPL 2
#endif
#ifndef ISIM_STREAM_WAVES
#define ISIM_STREAM_WAVES 8  // waves per SIMD the draw-stream kernel is compiled for
#endif

namespace isim {
namespace dev {

constexpr int kStreamTPL = ISIM_STREAM_TPL;  // traces per lane in the draw-stream kernel

// ======================================================================
// STATIC walk: uniform time (UT = u32 when the latency bound fits) and hops.
// ======================================================================
template <bool MODEB, typename UT>
__device__ __forceinline__ void walk_static(const Ctx &c, uint64_t trace_begin, uint64_t n_traces,
                                            uint64_t base) {
  const uint32_t lane = lane_id();
  const uint64_t idx = base + lane;
  const bool valid = idx < n_traces;
  const uint64_t t = trace_begin + idx;
  const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32);
  const uint32_t t_hi_u = rfl(t_hi);
  const bool hi_uniform = ballot(t_hi != t_hi_u) == 0;  // the batch does not straddle 2^32
  const uint64_t all = ballot(valid);
  const Ins *__restrict__ prog = c.prog;

  UT acc = 0, cmax = 0;
  uint64_t own = 0, failed = 0, cerr = 0, root_st = 0;
  uint32_t hop = 0, have = 0xFFFFFFFFu, depth = 0, pc = 0;
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0, errh = 0;
  LaneStack<uint32_t> f_ret;
  LaneStack<uint64_t> f_own, f_cerr;
  LaneStack<UT> f_acc, f_cmax;

  auto fold = [&](uint32_t flags, UT v, uint64_t st) {
    if (flags & F_ROOT) {
      root_st = st;
      acc = v;
    } else if (flags & F_CONC) {
      cmax = v > cmax ? v : cmax;
      if constexpr (MODEB) cerr |= st;
    } else {
      acc += v;
      if constexpr (MODEB) failed |= st;
    }
  };

  Ins cur = prog[0];
  while (true) {
    const uint32_t op = cur.opf & 0xFFu;
    if (op == OP_HALT) break;
    const uint32_t flags = (cur.opf >> 8) & 0xFFu;
    uint32_t npc = pc + 1;
    if (op == OP_CALL) npc = cur.b_lo;
    if (op == OP_RET) npc = f_ret.get(depth - 1);
    const Ins2 pre = *reinterpret_cast<const Ins2 *>(prog + (npc - 1));  // [npc-1, npc]
    switch (op) {
      case OP_SLEEP:
        acc += (UT)u64of(cur.a_lo, cur.a_hi);
        break;
      case OP_CBEGIN:
        cmax = 0;
        cerr = 0;
        break;
      case OP_CSLEEP: {
        const UT d = (UT)u64of(cur.a_lo, cur.a_hi);
        cmax = d > cmax ? d : cmax;
        break;
      }
      case OP_CEND:
        acc += cmax;
        if constexpr (MODEB) failed |= cerr;
        break;
      case OP_LEAF:
      case OP_CALL: {
        uint64_t st = 0;
        if (flags & F_ERR_ALWAYS) {
          st = all;
        } else if (flags & F_ERR_DRAW) {
          const uint32_t blk = hop >> 2;
          if (blk != have) {
            have = blk;
            uint32_t a = t_lo, b = t_hi, cc = blk, d = 0;
            if (hi_uniform) {
              // rounds 1-2 with the uniform counter words folded into SGPR math
              // keep the key schedule out of SGPRs between refills (recomputed
              // with 2 SALU adds per round instead of 20 hoisted registers)
              uint32_t k0a = c.k0, k1a = c.k1;
              asm volatile("" : "+s"(k0a), "+s"(k1a));
              const uint64_t q1 = (uint64_t)M1 * blk;                    // scalar
              const uint64_t p0 = (uint64_t)M0 * t_lo;                   // per lane
              const uint32_t u0 = (uint32_t)(q1 >> 32) ^ t_hi_u ^ k0a;   // uniform
              const uint32_t u1 = (uint32_t)q1;                          // uniform
              const uint32_t v2 = (uint32_t)(p0 >> 32) ^ k1a;            // per lane
              const uint32_t v3 = (uint32_t)p0;                          // per lane
              const uint32_t k0b = k0a + W0, k1b = k1a + W1;
              const uint64_t q0 = (uint64_t)M0 * u0;                     // scalar
              const uint64_t p1 = (uint64_t)M1 * v2;                     // per lane
              a = (uint32_t)(p1 >> 32) ^ u1 ^ k0b;
              b = (uint32_t)p1;
              cc = (uint32_t)(q0 >> 32) ^ v3 ^ k1b;
              d = (uint32_t)q0;
              uint32_t k0 = k0b + W0, k1 = k1b + W1;
#pragma unroll
              for (int r = 2; r < 10; ++r) {
                round1(a, b, cc, d, k0, k1);
                k0 += W0;
                k1 += W1;
              }
            } else {
              philox10(a, b, cc, d, c.k0, c.k1);
            }
            x0 = a;
            x1 = b;
            x2 = cc;
            x3 = d;
          }
          const uint32_t w = hop & 3u;
          const uint32_t lo = (w & 1u) ? x1 : x0;
          const uint32_t hi = (w & 1u) ? x3 : x2;
          st = ballot(((w & 2u) ? hi : lo) < cur.thr) & all;
        }
        ++hop;
        if (!(flags & F_ROOT)) count(c.gstats, c.cnt, cur.slot, popc(all));
        const UT H = (UT)u64of(cur.a_lo, cur.a_hi);
        if (op == OP_LEAF) {
          if (!(flags & F_ROOT)) count(c.gstats, c.cnt, c.n_slots + cur.slot, popc(st));
          if (lane_in(st)) ++errh;
          fold(flags, H + (UT)u64of(cur.b_lo, cur.b_hi), st);
        } else {
          f_ret.put(depth, pc + 1);
          f_own.put(depth, own);
          f_acc.put(depth, acc);
          f_cmax.put(depth, cmax);
          if constexpr (MODEB) f_cerr.put(depth, cerr);
          ++depth;
          acc = 0;
          cmax = 0;
          cerr = 0;
          failed = 0;
          own = st;
        }
        break;
      }
      case OP_RET: {
        const uint64_t st = (failed | own) & all;
        const UT T = acc;
        --depth;
        own = f_own.get(depth);
        acc = f_acc.get(depth);
        cmax = f_cmax.get(depth);
        if constexpr (MODEB) cerr = f_cerr.get(depth);
        failed = 0;  // static walks never call after a failed step
        const Ins &cin = pre.a;
        const uint32_t cflags = (cin.opf >> 8) & 0xFFu;
        if (!(cflags & F_ROOT)) count(c.gstats, c.cnt, c.n_slots + cin.slot, popc(st));
        if (lane_in(st)) ++errh;
        fold(cflags, (UT)u64of(cin.a_lo, cin.a_hi) + T, st);
        break;
      }
      default:
        __builtin_trap();
    }
    cur = pre.b;
    pc = npc;
  }
  finish_batch(c, idx, valid, all, (uint64_t)acc, hop, root_st, errh);
}

// ======================================================================
// DYNAMIC walk: per-lane time (TT) and hop ids, LDS frame stack.
// ======================================================================
// Per-service invocation durations (RecordResponseSent, srv/prometheus/
// handler.go:101-106): row = [code][33] bucket counts + [code] sums (ns).
// A leaf callee's duration is its fixed latency (bucket precomputed in the
// table word); a RET has per-lane durations.
__device__ __forceinline__ void leaf_duration(const Ctx &c, uint32_t w, uint64_t T, uint64_t e, uint64_t st) {
  if (lane_id() != 0) return;
  unsigned long long *row = (unsigned long long *)(c.svc_tab + (uint64_t)(w & kDurRowMask) * ISIM_SVC_DUR_WORDS);
  const uint32_t b = w >> 24;
  const uint32_t n5 = popc(st), n2 = popc(e) - n5;
  if (n2) {
    atomicAdd(row + b, (unsigned long long)n2);
    atomicAdd(row + 2 * ISIM_N_PROM, (unsigned long long)(T * n2));
  }
  if (n5) {
    atomicAdd(row + ISIM_N_PROM + b, (unsigned long long)n5);
    atomicAdd(row + 2 * ISIM_N_PROM + 1, (unsigned long long)(T * n5));
  }
}

__device__ __forceinline__ void ret_duration(const Ctx &c, uint32_t row_i, uint64_t T, uint64_t e, uint64_t st) {
  uint64_t *row = c.svc_tab + (uint64_t)row_i * ISIM_SVC_DUR_WORDS;
  const bool is5 = lane_in(st);
  hist_add_global(row, (is5 ? ISIM_N_PROM : 0u) + prom_bucket(T), e);
  const uint64_t s2 = wave_sum64(lane_in(e & ~st) ? T : 0);
  const uint64_t s5 = st ? wave_sum64(is5 ? T : 0) : 0;
  if (lane_id() == 0) {
    if (s2) atomicAdd((unsigned long long *)(row + 2 * ISIM_N_PROM), (unsigned long long)s2);
    if (s5) atomicAdd((unsigned long long *)(row + 2 * ISIM_N_PROM + 1), (unsigned long long)s5);
  }
}

template <bool MODEB, typename TT>
__device__ __forceinline__ void walk_dynamic(const Ctx &c, uint64_t trace_begin, uint64_t n_traces,
                                             uint64_t base, TT *__restrict__ lstk, uint32_t *__restrict__ hstk) {
  const uint32_t lane = lane_id();
  const uint64_t idx = base + lane;
  const bool valid = idx < n_traces;
  const uint64_t t = trace_begin + idx;
  const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32);
  const uint64_t all = ballot(valid);
  const Ins *__restrict__ prog = c.prog;

  uint64_t live = all, failed = 0, cerr = 0, own = 0, root_st = 0;
  uint32_t depth = 0, pc = 0;
  TT acc = 0, cmax = 0;
  uint32_t myhop = 0, hopn = 0, cblk = 0xFFFFFFFFu;
  uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0, errh = 0;
  LaneStack<uint32_t> f_ret;
  LaneStack<uint64_t> f_live, f_failed, f_cerr, f_own;

  auto fold = [&](uint32_t flags, uint64_t H, TT T, uint64_t e, uint64_t st) {
    if (flags & F_ROOT) {
      root_st = st;
      if (lane_in(e)) acc = (TT)H + T;
    } else if (flags & F_CONC) {
      if (lane_in(e)) {
        const TT v = (TT)H + T;
        cmax = v > cmax ? v : cmax;
      }
      if constexpr (MODEB) cerr |= st;
    } else {
      if (lane_in(e)) acc += (TT)H + T;
      if constexpr (MODEB) failed |= st;
    }
  };

  Ins cur = prog[0];
  while (true) {
    const uint32_t op = cur.opf & 0xFFu;
    if (op == OP_HALT) break;
    const uint32_t flags = (cur.opf >> 8) & 0xFFu;
    uint32_t npc = pc + 1;
    if (op == OP_CALL) npc = cur.b_lo;
    if (op == OP_RET) npc = f_ret.get(depth - 1);
    Ins2 pre = *reinterpret_cast<const Ins2 *>(prog + (npc - 1));
    const uint64_t act = live & ~failed;
    switch (op) {
      case OP_SLEEP:
        if (lane_in(act)) acc += (TT)u64of(cur.a_lo, cur.a_hi);
        break;
      case OP_CBEGIN:
        if (lane_in(act)) cmax = 0;
        cerr = 0;
        break;
      case OP_CSLEEP:
        if (lane_in(act)) {
          const TT d = (TT)u64of(cur.a_lo, cur.a_hi);
          cmax = d > cmax ? d : cmax;
        }
        break;
      case OP_CEND:
        if (lane_in(act)) acc += cmax;
        if constexpr (MODEB) failed |= cerr & live;
        break;
      case OP_LEAF:
      case OP_CALL: {
        uint64_t e = act;
        if (flags & F_PROB) {  // shouldSkipRequest: Intn(100) < 100 - p
          bool skip = false;
          if (lane_in(e)) {
            uint32_t c0 = t_lo, c1 = t_hi, c2 = myhop, c3 = 1u + (cur.k >> 2);
            philox10(c0, c1, c2, c3, c.k0, c.k1);
            const uint32_t sel = cur.k & 3u;
            const uint32_t word = sel == 0 ? c0 : sel == 1 ? c1 : sel == 2 ? c2 : c3;
            skip = (word % 100u) < 100u - (cur.opf >> 16);
          }
          e &= ~ballot(skip);
        }
        if (e == 0) {  // no lane makes this call: fall through to pc+1
          if (op == OP_CALL) {
            npc = pc + 1;
            pre = *reinterpret_cast<const Ins2 *>(prog + (npc - 1));
          }
          break;
        }
        uint64_t st = 0;
        if (flags & F_ERR_ALWAYS) {
          st = e;
        } else if (flags & F_ERR_DRAW) {
          const uint32_t blk = hopn >> 2;
          const uint64_t need = ballot(blk != cblk) & e;
          if (need && lane_in(need)) {
            uint32_t a = t_lo, b = t_hi, cc = blk, d = 0;
            philox10(a, b, cc, d, c.k0, c.k1);
            x0 = a;
            x1 = b;
            x2 = cc;
            x3 = d;
            cblk = blk;
          }
          const uint32_t w = hopn & 3u;
          const uint32_t lo = (w & 1u) ? x1 : x0;
          const uint32_t hi = (w & 1u) ? x3 : x2;
          st = ballot(((w & 2u) ? hi : lo) < cur.thr) & e;
        }
        const uint32_t myh = hopn;
        if (lane_in(e)) ++hopn;
        if (!(flags & F_ROOT)) count(c.gstats, c.cnt, cur.slot, popc(e));
        const uint64_t H = u64of(cur.a_lo, cur.a_hi);
        if (op == OP_LEAF) {
          if (!(flags & F_ROOT)) count(c.gstats, c.cnt, c.n_slots + cur.slot, popc(st));
          if (lane_in(st)) ++errh;
          if (c.svc_tab) leaf_duration(c, (flags & F_ROOT) ? c.root_dur : c.dur[cur.slot],
                                       u64of(cur.b_lo, cur.b_hi), e, st);
          fold(flags, H, (TT)u64of(cur.b_lo, cur.b_hi), e, st);
        } else {
          f_ret.put(depth, pc + 1);
          f_own.put(depth, own);
          f_live.put(depth, live);
          f_failed.put(depth, failed);
          if constexpr (MODEB) f_cerr.put(depth, cerr);
          lstk[(2 * depth) * 64 + lane] = acc;
          lstk[(2 * depth + 1) * 64 + lane] = cmax;
          hstk[depth * 64 + lane] = myhop;
          ++depth;
          acc = 0;
          cmax = 0;
          myhop = myh;
          live = e;
          failed = 0;
          cerr = 0;
          own = st;
        }
        break;
      }
      case OP_RET: {
        const uint64_t e = live;
        const uint64_t st = (failed | own) & e;
        const TT T = acc;
        --depth;
        own = f_own.get(depth);
        live = f_live.get(depth);
        failed = f_failed.get(depth);
        if constexpr (MODEB) cerr = f_cerr.get(depth);
        else cerr = 0;
        acc = lstk[(2 * depth) * 64 + lane];
        cmax = lstk[(2 * depth + 1) * 64 + lane];
        myhop = hstk[depth * 64 + lane];
        const Ins &cin = pre.a;
        const uint32_t cflags = (cin.opf >> 8) & 0xFFu;
        if (!(cflags & F_ROOT)) count(c.gstats, c.cnt, c.n_slots + cin.slot, popc(st));
        if (lane_in(st)) ++errh;
        if (c.svc_tab) ret_duration(c, ((cflags & F_ROOT) ? c.root_dur : c.dur[cin.slot]) & kDurRowMask,
                                    (uint64_t)T, e, st);
        fold(cflags, u64of(cin.a_lo, cin.a_hi), T, e, st);
        break;
      }
      default:
        __builtin_trap();
    }
    cur = pre.b;
    pc = npc;
  }
  finish_batch(c, idx, valid, all, (uint64_t)acc, hopn, root_st, errh);
}

// Kind 8's per-launch fold (one workgroup): the launch's position marks
// (u32, wrapping: the -1s at an LCA reached often go "negative") become
// subtree sums S(v) = P[end(v)] - P[v - 1] over their prefix sums P — the
// launch's count of 500 responses of the invocation at record v, below 2^32
// (launch_walk's split) — added to the per-site 500 counters; the row is
// zeroed for the next launch that takes this work slot.
__global__ void __launch_bounds__(1024) isim_mark_fold(uint32_t *__restrict__ stage, uint32_t n, uint32_t words,
                                                       const uint32_t *__restrict__ end,
                                                       const uint32_t *__restrict__ slot,
                                                       uint64_t *__restrict__ gstats, uint32_t n_slots) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint32_t *P = reinterpret_cast<uint32_t *>(lds);
  __shared__ uint32_t wtot[16];
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  for (uint32_t i = tid; i < words; i += nt) {
    P[i] = i < n ? stage[i] : 0u;
    stage[i] = 0u;
  }
  __syncthreads();
  // each thread a contiguous segment: local sums, a block scan of the
  // segment totals, then the segment rewritten as inclusive prefix sums
  const uint32_t seg = (n + nt - 1) / nt;
  const uint32_t b = tid * seg, e = b + seg < n ? b + seg : n;
  uint32_t tot = 0;
  for (uint32_t i = b; i < e; ++i) tot += P[i];
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  uint32_t inc = tot;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  uint32_t pre = inc - tot;
  for (uint32_t w = 0; w < wave; ++w) pre += wtot[w];
  for (uint32_t i = b; i < e; ++i) {
    pre += P[i];
    P[i] = pre;
  }
  __syncthreads();
  unsigned long long *st = reinterpret_cast<unsigned long long *>(gstats + ISIM_ST_SITES + n_slots);
  for (uint32_t v = 1 + tid; v < n; v += nt) {
    const uint32_t s = P[end[v]] - P[v - 1];
    if (s) atomicAdd(st + slot[v], (unsigned long long)s);
  }
}

// Executed-call counters of a static walk: every trace makes mult[slot] calls
// through each reachable call site, so a launch over n_traces adds
// mult[slot] * n_traces (exact; added once per launch).
// draw-free static walks: n copies of one trace's record, n x its statistics
__global__ void __launch_bounds__(256) isim_fill_const(isim_trace_rec *__restrict__ rec, uint64_t n,
                                                       isim_trace_rec r, const uint64_t *__restrict__ s1,
                                                       uint64_t *__restrict__ gstats, uint32_t words) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
  if (rec) {
    // streaming stores, 4 in flight per lane
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {(uint32_t)r.latency_ns, (uint32_t)(r.latency_ns >> 32), r.hops, r.status_err};
    u32x4 *out = reinterpret_cast<u32x4 *>(rec);
    uint64_t i = tid;
    for (; i + 3 * stride < n; i += 4 * stride) {
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) __builtin_nontemporal_store(v, out + i + u * stride);
    }
    for (; i < n; i += stride) __builtin_nontemporal_store(v, out + i);
  }
  unsigned long long *st = reinterpret_cast<unsigned long long *>(gstats);
  for (uint64_t w = tid; w < words; w += stride) {
    const uint64_t x = s1[w];
    if (!x) continue;
    if (w == ISIM_ST_NOT_MIN_LATENCY || w == ISIM_ST_MAX_LATENCY) atomicMax(st + w, (unsigned long long)x);
    else atomicAdd(st + w, (unsigned long long)(x * n));
  }
}

__global__ void isim_stream_calls(const uint32_t *__restrict__ mult, uint32_t n_slots, uint64_t n_traces,
                                  uint64_t *__restrict__ gstats, uint32_t *__restrict__ stage) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  gstats[ISIM_ST_SITES + i] += (uint64_t)mult[i] * n_traces;
  if (stage) {  // the launch's staged 500 counts (u32) into the stats; the row is zero again after
    const uint32_t v = stage[i];
    if (v) {
      gstats[ISIM_ST_SITES + n_slots + i] += v;
      stage[i] = 0;
    }
  }
}

// The group table of one draw-stream launch (kernel_abi.h GroupEnt), launched
// before the walk on the same stream: entry g holds rounds 1-2 of the
// wave-uniform counter words of group g's Philox blocks, for trace ids with
// high word t_hi, and the group's record tests; kGroupPad zero entries follow.
__global__ void isim_group_table(const Node *__restrict__ stream, uint32_t n_groups, uint32_t seed_lo,
                                 uint32_t seed_hi, uint32_t t_hi, GroupEnt *__restrict__ tab) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups + kGroupPad) return;
  GroupEnt e{0u, 0u, 0u, 0u};
  if (g < n_groups) {
    philox_uniform_rounds(t_hi, g, seed_lo, seed_hi, e.uk0, e.uk1, e.d);
    uint32_t thr = 0, meta = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      thr |= stream[4u * g + j].thr;
      meta |= stream[4u * g + j].meta;
    }
    e.flags = (thr ? kGroupAnyThr : 0u) | (meta & kGroupAnyAlways);
  }
  tab[g] = e;
}

// KIND: 0 static/u32 time, 1 static/u64, 2 dynamic/u32, 3 dynamic/u64, 4 draw stream
// (mode B: the wave-mask stack), 5 draw stream with the mode-B bit stack (call
// depth <= 32), 6 draw stream with the mode-B close list, 8 draw stream with
// mode-B sparse ancestor marking (stream_walk.h; 7 is the lane tree walk, tree.hip)
// LDSC: per-site counters in the workgroup LDS table (else global atomics)
// LEAN (KIND 4, mode A): every batch of the launch draws from the group table,
// so walk_stream_a's table loop is the only one compiled in, and the group
// loop takes its round keys and multipliers from VGPRs (stream_walk.h)
template <int KIND, bool MODEB, bool LDSC, bool LEAN = false>
__global__ void __launch_bounds__(kWgThreads, KIND >= 4 ? ISIM_STREAM_WAVES : 1)
    isim_walk(const Ins *__restrict__ prog, isim_trace_rec *__restrict__ records, uint64_t *__restrict__ gstats,
              const uint32_t *__restrict__ dur, KParams kp) {
  static_assert(!LEAN || (KIND == 4 && !MODEB), "the lean kernel is mode A on the draw stream");
  using TT = typename std::conditional<KIND == 0 || KIND == 2, uint32_t, uint64_t>::type;
  constexpr bool STATIC = KIND < 2 || KIND >= 4;
  extern __shared__ __align__(16) unsigned char lds[];
  Ctx c;
  c.prog = prog;
  c.records = records;
  c.gstats = gstats;
  c.dur = dur;
  c.svc_tab = kp.svc_dur ? gstats + ISIM_ST_SVC_DUR(kp.n_slots) : nullptr;
  c.root_dur = kp.root_dur;
  c.acc = reinterpret_cast<WgAcc *>(lds);
  c.hist = reinterpret_cast<uint32_t *>(lds + kLdsAccBytes);
  c.cnt = LDSC ? c.hist + kHistWords : nullptr;
  c.n_slots = kp.n_slots;
  c.k0 = kp.seed_lo;
  c.k1 = kp.seed_hi;
  unsigned char *stk = lds + kLdsAccBytes + kHistWords * 4 + (LDSC ? 8u * kp.n_slots : 0u);
  stk = (unsigned char *)(((uintptr_t)stk + 15) & ~(uintptr_t)15);
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t waves = blockDim.x >> 6;
  TT *lstk = nullptr;
  uint32_t *hstk = nullptr;
  if constexpr (!STATIC) {
    const uint32_t per_wave = kp.max_frames * 64u * (2u * (uint32_t)sizeof(TT) + 4u);
    lstk = reinterpret_cast<TT *>(stk + wave * per_wave);
    hstk = reinterpret_cast<uint32_t *>(stk + wave * per_wave + kp.max_frames * 64u * 2u * (uint32_t)sizeof(TT));
  }
  const uint32_t zero_words = (kLdsAccBytes / 4) + kHistWords + (LDSC ? (KIND == 8 ? kp.mark_words : 2u * kp.n_slots) : 0u);
  uint32_t *z = reinterpret_cast<uint32_t *>(lds);
  for (uint32_t i = threadIdx.x; i < zero_words; i += blockDim.x) z[i] = 0;
  __syncthreads();

  constexpr uint64_t kBatch = KIND >= 4 ? 64ull * kStreamTPL : 64ull;
  const uint64_t n_batches = (kp.n_traces + kBatch - 1) / kBatch;
  const uint64_t stride = (uint64_t)gridDim.x * waves;
  // Batches: the first wave-stride statically, the rest claimed from the
  // launch's queues, so waves the SIMD arbiter favours take more batches and
  // the grid drains within about one batch of the last claim.  Queue q (the
  // workgroup's XCD; every queue in use has workgroups) deals batches
  // stride + nq c + q.
  const uint32_t nq = gridDim.x < kWorkQueues ? gridDim.x : kWorkQueues;
  const uint32_t q = blockIdx.x % nq;
  unsigned long long *queue = kp.work + q * kWorkLine;
  auto claim = [&]() -> uint64_t {
    unsigned long long v = 0;
    if (lane_id() == 0) v = atomicAdd(queue, 1ull);
    const uint64_t c = (uint64_t)rfl((uint32_t)(v >> 32)) << 32 | rfl((uint32_t)v);
    return stride + c * nq + q;
  };
  for (uint64_t b = (uint64_t)blockIdx.x * waves + wave; b < n_batches; b = claim()) {
    if constexpr (KIND >= 4) {
      const uint64_t base = b * kBatch;
      CNode4 *st = (CNode4 *)(const __attribute__((address_space(1))) Ins *)prog;
      const uint32_t ng = kp.n_nodes ? (kp.n_nodes + 3) / 4 : 0;
      CEnt *gt = (CEnt *)(const __attribute__((address_space(1))) GroupEnt *)kp.gtab;
      const uint32_t gth = kp.gtab_t_hi;
      // FULL (every lane of every trace slot valid) stays a plain if/else per
      // kind: behind a generic-lambda helper the same walkers were scheduled
      // differently and mode A measured 0.5 % slower
      if constexpr (KIND == 8) {
        if (base + 64 * kStreamTPL <= kp.n_traces)
          walk_stream_mark<kStreamTPL, true>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces, base, gt,
                                             gth);
        else
          walk_stream_mark<kStreamTPL, false>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces, base, gt,
                                              gth);
      } else if constexpr (KIND == 6) {
        CClose *cl = (CClose *)(const __attribute__((address_space(1))) StreamClose *)kp.closes;
        CU32 *ce = (CU32 *)(const __attribute__((address_space(1))) uint32_t *)kp.close_end;
        if (base + 64 * kStreamTPL <= kp.n_traces)
          walk_stream_cl<LDSC, kStreamTPL, true>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces,
                                                 base, cl, kp.close_slot, ce, (const uint32_t *)prog, gt, gth);
        else
          walk_stream_cl<LDSC, kStreamTPL, false>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces,
                                                  base, cl, kp.close_slot, ce, (const uint32_t *)prog, gt, gth);
      } else if constexpr (MODEB) {
        walk_stream<LDSC, kStreamTPL, KIND == 5>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces, base,
                                                 gt, gth);
      } else if constexpr (LEAN) {
        if (base + 64 * kStreamTPL <= kp.n_traces)
          walk_stream_a<LDSC, kStreamTPL, true, true>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces,
                                                      base, (const uint32_t *)prog, gt, gth);
        else
          walk_stream_a<LDSC, kStreamTPL, false, true>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces,
                                                       base, (const uint32_t *)prog, gt, gth);
      } else if (base + 64 * kStreamTPL <= kp.n_traces)  // every lane of every trace slot valid
        walk_stream_a<LDSC, kStreamTPL, true>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces, base,
                                              (const uint32_t *)prog, gt, gth);
      else
        walk_stream_a<LDSC, kStreamTPL, false>(c, st, ng, kp.n_nodes, kp.t_static, kp.trace_begin, kp.n_traces, base,
                                               (const uint32_t *)prog, gt, gth);
    }
    else if constexpr (STATIC) walk_static<MODEB, TT>(c, kp.trace_begin, kp.n_traces, b * 64);
    else walk_dynamic<MODEB, TT>(c, kp.trace_begin, kp.n_traces, b * 64, lstk, hstk);
  }

  // every wave has stopped claiming once all have counted out: the last one re-arms the queue
  if (lane_id() == 0 && atomicAdd(kp.work + kWorkQueues * kWorkLine, 1ull) == stride - 1) {
    for (uint32_t i = 0; i <= kWorkQueues; ++i) atomicExch(kp.work + i * kWorkLine, 0ull);
  }
  __syncthreads();
  // ---- flush workgroup accumulators to HBM
  unsigned long long *st = reinterpret_cast<unsigned long long *>(gstats);
  for (uint32_t i = threadIdx.x; i < kHistWords; i += blockDim.x)
    if (c.hist[i]) atomicAdd(st + ISIM_ST_PROM + i, (unsigned long long)c.hist[i]);
  if constexpr (KIND == 8) {  // the position marks, folded into the site counters by isim_mark_fold
    for (uint32_t i = threadIdx.x; i < kp.mark_words; i += blockDim.x)
      if (c.cnt[i]) atomicAdd(kp.stage + i, c.cnt[i]);
  } else if constexpr (LDSC) {
    if (kp.stage) {  // draw stream: only the 500 counts are counted here (calls: isim_stream_calls)
      for (uint32_t i = threadIdx.x; i < kp.n_slots; i += blockDim.x)
        if (c.cnt[kp.n_slots + i]) atomicAdd(kp.stage + i, c.cnt[kp.n_slots + i]);
    } else {
      for (uint32_t i = threadIdx.x; i < 2u * kp.n_slots; i += blockDim.x)
        if (c.cnt[i]) atomicAdd(st + ISIM_ST_SITES + i, (unsigned long long)c.cnt[i]);
    }
  }
  if (threadIdx.x == 0 && c.acc->ntr) {
    atomicAdd(st + ISIM_ST_N_TRACES, c.acc->ntr);
    atomicAdd(st + ISIM_ST_SUM_LATENCY, c.acc->sum_latency);
    atomicAdd(st + ISIM_ST_SUM_HOPS, c.acc->sum_hops);
    atomicAdd(st + ISIM_ST_SUM_ERR_HOPS, c.acc->sum_err);
    atomicAdd(st + ISIM_ST_N_500, c.acc->n500);
    atomicMax(st + ISIM_ST_NOT_MIN_LATENCY, c.acc->notmin);
    atomicMax(st + ISIM_ST_MAX_LATENCY, c.acc->max);
  }
}

}  // namespace dev

template <int K>
static void *pick(bool modeb, bool ldsc) {
  using namespace dev;
  if (ldsc) return modeb ? (void *)&isim_walk<K, true, true> : (void *)&isim_walk<K, false, true>;
  return modeb ? (void *)&isim_walk<K, true, false> : (void *)&isim_walk<K, false, false>;
}

void *walk_kernel(int kind, bool modeb, bool lds_counters) {
  switch (kind) {
    case 0: return pick<0>(modeb, lds_counters);
    case 1: return pick<1>(modeb, lds_counters);
    case 2: return pick<2>(modeb, lds_counters);
    case 3: return pick<3>(modeb, lds_counters);
    case 4: return pick<4>(modeb, lds_counters);
    case 5:  // the bit stack only exists in mode B
      if (!modeb) return pick<4>(false, lds_counters);
      return lds_counters ? (void *)&dev::isim_walk<5, true, true> : (void *)&dev::isim_walk<5, true, false>;
    case 8:  // sparse ancestor marking: mode B, position marks in LDS only
      if (!modeb) return pick<4>(false, lds_counters);
      return lds_counters ? (void *)&dev::isim_walk<8, true, true> : nullptr;
    default:  // 6: the close list only exists in mode B
      if (!modeb) return pick<4>(false, lds_counters);
      return lds_counters ? (void *)&dev::isim_walk<6, true, true> : (void *)&dev::isim_walk<6, true, false>;
  }
}

void *walk_kernel_lean(bool lds_counters) {
  return lds_counters ? (void *)&dev::isim_walk<4, false, true, true> : (void *)&dev::isim_walk<4, false, false, true>;
}

void *mark_fold_kernel() { return (void *)&dev::isim_mark_fold; }

void *stream_calls_kernel() { return (void *)&dev::isim_stream_calls; }
void *group_table_kernel() { return (void *)&dev::isim_group_table; }
void *fill_const_kernel() { return (void *)&dev::isim_fill_const; }
uint32_t stream_traces_per_wave() { return 64u * (uint32_t)dev::kStreamTPL; }

}  // namespace isim
