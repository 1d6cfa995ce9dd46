// DRAW STREAM walks (static walks; included by walk.hip, kernel kinds 4, 5, 6
// and 8 of isim_walk): every trace executes the same invocation sequence, so
// the program compiler lays the invocations out in hop order (one 8-byte Node
// each) and folds the trace-invariant latency (t_static), hop count and
// per-site call multiplicities (the executed-call counters are mult[slot] x
// n_traces, added by isim_stream_calls).  Per lane and invocation only the
// stochastic part remains: the Philox error draw, the 500 status (mode B:
// OR-ed up the call tree at each subtree close), the per-trace error count and
// the per-site error counters.  Four records share one Philox block and one
// s_load_dwordx8, loaded one group ahead of the group being processed (the
// device buffer carries two zero groups of tail padding, so the group loops
// load past the last group without a bound test).  What a group's Philox
// blocks need of the wave-uniform counter words comes from the launch's group
// table (kernel_abi.h GroupEnt), loaded the same way, when the batch may use it.
//
// The five walkers differ in what a record's error mask is used for; they
// share the batch setup (StreamBatch), the group's draws (stream_draws), the
// group loops (stream_pingpong, stream_one_ahead) and the per-site 500
// counter add (site_err_add).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernel_abi.h"
#include "walk_dev.h"

namespace isim {
namespace dev {

struct Node4 {
  Node n[4];
};
// The stream is read-only for the whole launch: reading it through the
// constant address space lets the compiler issue s_load_dwordx8 (a uniform
// global-space load after the loop's stores would become a VMEM load +
// v_readfirstlane with an immediate vmcnt wait).
typedef const __attribute__((address_space(4))) Node4 CNode4;
__device__ __forceinline__ Node4 load_group(CNode4 *p) {
  Node4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r.n[j].thr = p->n[j].thr;
    r.n[j].meta = p->n[j].meta;
  }
  return r;
}

// The launch's group table (kernel_abi.h GroupEnt), read like the stream: one
// s_load_dwordx4 per group.
typedef const __attribute__((address_space(4))) GroupEnt CEnt;
__device__ __forceinline__ GroupEnt load_ent(CEnt *p) {
  GroupEnt r;
  r.uk0 = p->uk0;
  r.uk1 = p->uk1;
  r.d = p->d;
  r.flags = p->flags;
  return r;
}

// m = 2 m + (this lane in mask): one v_addc_co_u32 with the lane mask as carry-in
__device__ __forceinline__ void shift_in(uint32_t &m, uint64_t mask) {
  uint64_t co;
  asm("v_addc_co_u32 %0, %1, %0, %0, %2" : "+v"(m), "=s"(co) : "s"(mask));
}
// v += (this lane in mask)
__device__ __forceinline__ void add_lane(uint32_t &v, uint64_t mask) {
  uint64_t co;
  asm("v_addc_co_u32 %0, %1, 0, %0, %2" : "+v"(v), "=s"(co) : "s"(mask));
}

// A lane's add to the 500 counter of call site `slot` (LDS table, or global
// atomics when the table does not fit).  The caller picks the lanes: lane 0
// for a wave-uniform count, a lane per record or per close for the per-chunk
// count flushes.
template <bool LDSC>
__device__ __forceinline__ void site_err_add(const Ctx &c, uint32_t slot, uint32_t v) {
  if constexpr (LDSC) atomicAdd(c.cnt + c.n_slots + slot, v);
  else atomicAdd((unsigned long long *)(c.gstats + ISIM_ST_SITES + c.n_slots + slot), (unsigned long long)v);
}

// Round keys of the lockstep draws (philox_lockstep_from).  Rounds 1-2 run on
// the wave-uniform words and round 3's keys are folded into its operands, so
// the vector rounds that take a key are rounds 4-10.  The keys of the first
// NH of them are held in VGPRs for the whole batch (wave-uniform values; a
// VOP3 takes three VGPR sources, so they cost no instruction); the later
// rounds add theirs up in scalar code in every group (2 s_add each).  They do
// not go into SGPRs: the kernels sit at their SGPR cap, and held scalar keys
// spill to VGPR lanes and come back as v_readlane (VALU).
// NH per walker: what its kernels' VGPR budget (64 at ISIM_STREAM_WAVES 8)
// holds with no scratch and no v_readlane added to a group loop.
// What a held key saves is the SGPR source of its v_bitop3, not the s_add: a
// VALU instruction that reads an SGPR costs the group loop more issue time
// than one on VGPRs alone (measured on the lean kernel).
#ifndef ISIM_HELD_A
#define ISIM_HELD_A 4
#endif
#ifndef ISIM_HELD_MARK
#define ISIM_HELD_MARK 7
#endif
#ifndef ISIM_HELD_CL
#define ISIM_HELD_CL 2
#endif
#ifndef ISIM_HELD_STACK
#define ISIM_HELD_STACK 3
#endif
constexpr int kHeldA = ISIM_HELD_A;          // walk_stream_a (kind 4, mode A)
constexpr int kHeldMark = ISIM_HELD_MARK;    // walk_stream_mark (kind 8)
constexpr int kHeldCl = ISIM_HELD_CL;        // walk_stream_cl (kind 6)
constexpr int kHeldStack = ISIM_HELD_STACK;  // walk_stream (kinds 4 and 5, mode B)
constexpr int kFirstKeyRound = 3;  // 0-based: rounds 0-1 scalar, round 2 keyless
#ifndef ISIM_HELD_LEAN
#define ISIM_HELD_LEAN 6
#endif
constexpr int kHeldLean = ISIM_HELD_LEAN;    // walk_stream_a, the lean kernel
// The two Philox multipliers of the lockstep draws: the constants, or (LEAN)
// wave-uniform VGPR values, opaque, so that the v_mad_u64_u32 of the group
// loop read no SGPR either.
template <bool LEAN>
struct Mults {
  static constexpr uint32_t m0 = M0, m1 = M1;
};
template <>
struct Mults<true> {
  uint32_t m0 = M0, m1 = M1;
  __device__ __forceinline__ Mults() { asm volatile("" : "+v"(m0), "+v"(m1)); }
};
template <int NH>
struct HeldKeys {
  static_assert(NH >= 0 && NH <= 10 - kFirstKeyRound, "rounds 4-10 take a key");
  uint32_t k0[NH > 0 ? NH : 1], k1[NH > 0 ? NH : 1];
  __device__ __forceinline__ HeldKeys(uint32_t k0a, uint32_t k1a) {
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      k0[i] = k0a + (uint32_t)(kFirstKeyRound + i) * W0;
      k1[i] = k1a + (uint32_t)(kFirstKeyRound + i) * W1;
      // opaque VGPR values: neither rematerialised as s_add in the group
      // loop nor read back into SGPRs
      asm volatile("" : "+v"(k0[i]), "+v"(k1[i]));
    }
  }
};

// TPL traces per lane: the wave walks 64*TPL traces through one pass over the
// stream, so the per-record scalar work (fetch, decode, counter adds) is
// shared and each lane runs TPL independent Philox chains (ILP).  Trace u of
// a lane is trace base + 64 u + lane of the launch.
// LEAN (the lean mode-A kernel, which instantiates one chunk loop, not six,
// and so has registers left): the keys of the rounds past NH are plain
// loop-invariant sums of the seed words, which the compiler keeps in SGPRs,
// not re-added per group, and the multipliers are VGPR values (Mults).
template <int TPL, int NH, bool LEAN = false>
struct StreamBatch {
  uint64_t idx[TPL], all[TPL];  // index in the launch; ballot of valid
  uint32_t t_lo[TPL], t_hi[TPL];
  uint32_t t_hi_u;  // t_hi of the batch when hi_uniform
  bool valid[TPL];
  bool hi_uniform = true;
  HeldKeys<NH> keys;  // the lockstep draws' held round keys
  // the lockstep draws' round-2 word c1 of each trace (it depends on t_lo
  // alone) with round 3's key folded in.  Formed here, opaque: written next to
  // its use, the compiler re-associates the xor chain and pays a second xor
  // per trace in every group
  uint32_t bk[TPL];
  Mults<LEAN> mul;

  __device__ __forceinline__ StreamBatch(const Ctx &c, uint64_t trace_begin, uint64_t n_traces, uint64_t base)
      : keys(c.k0, c.k1) {
    const uint32_t lane = lane_id();
    uint32_t hi_u[TPL];
#pragma unroll
    for (int u = 0; u < TPL; ++u) {
      idx[u] = base + 64u * u + lane;
      valid[u] = idx[u] < n_traces;
      const uint64_t t = trace_begin + idx[u];
      t_lo[u] = (uint32_t)t;
      t_hi[u] = (uint32_t)(t >> 32);
      hi_u[u] = rfl(t_hi[u]);
      // the batch does not straddle 2^32: the high word of every trace id,
      // valid or not, is the one wave-uniform value that the lockstep draws
      // fold into scalar math
      hi_uniform = hi_uniform && ballot(t_hi[u] != hi_u[u]) == 0 && hi_u[u] == hi_u[0];
      all[u] = ballot(valid[u]);
      const uint32_t v2 = (uint32_t)(((uint64_t)M0 * t_lo[u]) >> 32) ^ c.k1;
      bk[u] = (uint32_t)((uint64_t)M1 * v2) ^ (c.k0 + 2u * W0);
      asm volatile("" : "+v"(bk[u]));
    }
    t_hi_u = hi_u[0];
  }

  __device__ __forceinline__ void finish(const Ctx &c, int u, uint64_t t_static, uint32_t n_nodes, uint64_t root_st,
                                         uint32_t errh) const {
    finish_batch(c, idx[u], valid[u], all[u], t_static, n_nodes, root_st, errh);
  }
};

// Rounds 1-2 of the wave-uniform counter words (t_hi, g, 0) of a group's
// Philox blocks: what the vector rounds need of them, as GroupEnt's words
// (d with round 3's key folded in: the word is used nowhere else).
// Shared by the walkers (scalar code, per wave and group) and the launch's
// group table (isim_group_table, once per group).
__host__ __device__ __forceinline__ void philox_uniform_rounds(uint32_t t_hi_u, uint32_t g, uint32_t k0a, uint32_t k1a,
                                                               uint32_t &uk0, uint32_t &uk1, uint32_t &d) {
  const uint64_t q1 = (uint64_t)M1 * g;                      // scalar
  const uint32_t u0 = (uint32_t)(q1 >> 32) ^ t_hi_u ^ k0a;   // uniform
  const uint32_t u1 = (uint32_t)q1;                          // uniform
  const uint32_t k0b = k0a + W0, k1b = k1a + W1;
  const uint64_t q0 = (uint64_t)M0 * u0;                     // scalar (round 2)
  uk0 = u1 ^ k0b;
  uk1 = (uint32_t)(q0 >> 32) ^ k1b;
  d = (uint32_t)q0 ^ (k1a + 2u * W1);
}

// TPL Philox blocks (one per trace of the lane) of counter (t_lo[u], t_hi, g, 0)
// in lockstep, given rounds 1-2 of the wave-uniform words (uk0, uk1, dk): the
// round keys are shared by the TPL chains.
template <int TPL, int NH, bool LEAN>
__device__ __forceinline__ void philox_lockstep_from(const StreamBatch<TPL, NH, LEAN> &bt, uint32_t k0a, uint32_t k1a,
                                                     uint32_t uk0, uint32_t uk1, uint32_t dk, uint32_t (&x)[TPL][4]) {
  uint32_t a[TPL], b[TPL], cc[TPL], d[TPL];
  // round 3 without keys: k1 + 2 W1 is in dk and k0 + 2 W0 in the batch's bk.
  // Two-input xors, and no v_mov to bring the wave-uniform d next to a
  // scalar key.
#pragma unroll
  for (int u = 0; u < TPL; ++u) {
    const uint64_t p0 = (uint64_t)M0 * bt.t_lo[u];           // per lane
    const uint32_t v2 = (uint32_t)(p0 >> 32) ^ k1a;
    const uint64_t p1 = (uint64_t)M1 * v2;
    const uint32_t bk = bt.bk[u];
    const uint32_t a2 = (uint32_t)(p1 >> 32) ^ uk0;
    const uint32_t c2 = (uint32_t)p0 ^ uk1;
    const uint64_t r0 = (uint64_t)bt.mul.m0 * a2;
    const uint64_t r1 = (uint64_t)bt.mul.m1 * c2;
    a[u] = (uint32_t)(r1 >> 32) ^ bk;
    b[u] = (uint32_t)r1;
    cc[u] = (uint32_t)(r0 >> 32) ^ dk;
    d[u] = (uint32_t)r0;
  }
#pragma unroll
  for (int i = 0; i < NH; ++i) {
#pragma unroll
    for (int u = 0; u < TPL; ++u) round1(a[u], b[u], cc[u], d[u], bt.keys.k0[i], bt.keys.k1[i], bt.mul.m0, bt.mul.m1);
  }
  if constexpr (LEAN) {
#pragma unroll
    for (int r = kFirstKeyRound + NH; r < 10; ++r) {
#pragma unroll
      for (int u = 0; u < TPL; ++u) round1(a[u], b[u], cc[u], d[u], k0a + (uint32_t)r * W0, k1a + (uint32_t)r * W1,
                                                   bt.mul.m0, bt.mul.m1);
    }
  } else if constexpr (kFirstKeyRound + NH < 10) {
    uint32_t k0 = k0a + (uint32_t)(kFirstKeyRound + NH) * W0;
    uint32_t k1 = k1a + (uint32_t)(kFirstKeyRound + NH) * W1;
#pragma unroll
    for (int r = kFirstKeyRound + NH; r < 10; ++r) {
      // recompute these round keys per group (2 s_add) instead of letting the
      // compiler hoist them into SGPRs (HeldKeys)
      asm volatile("" : "+s"(k0), "+s"(k1));
#pragma unroll
      for (int u = 0; u < TPL; ++u) round1(a[u], b[u], cc[u], d[u], k0, k1, bt.mul.m0, bt.mul.m1);
      k0 += W0;
      k1 += W1;
    }
  }
#pragma unroll
  for (int u = 0; u < TPL; ++u) {
    x[u][0] = a[u];
    x[u][1] = b[u];
    x[u][2] = cc[u];
    x[u][3] = d[u];
  }
}

// ... with the scalar rounds 1-2 computed here (all counter words but t_lo
// are wave-uniform): the batches without a group table.
template <int TPL, int NH>
__device__ __forceinline__ void philox_lockstep(const StreamBatch<TPL, NH> &bt, uint32_t g, uint32_t k0a, uint32_t k1a,
                                                uint32_t (&x)[TPL][4]) {
  uint32_t uk0, uk1, dk;
  philox_uniform_rounds(bt.t_hi_u, g, k0a, k1a, uk0, uk1, dk);
  // a VOP3 reads one SGPR: pre-xor the uniform words (opaque, so the
  // compiler does not re-fold them into a two-SGPR v_bitop3 + v_mov)
  asm volatile("" : "+s"(uk0), "+s"(uk1), "+s"(dk));
  philox_lockstep_from<TPL, NH>(bt, k0a, k1a, uk0, uk1, dk, x);
}

__device__ __forceinline__ uint32_t thr_or(const Node4 &q) {
  return q.n[0].thr | q.n[1].thr | q.n[2].thr | q.n[3].thr;
}

// The draws of group g: x[u][j] is trace u's draw for the group's record j,
// word j of Philox4x32-10((t_lo, t_hi, g, 0), seed); zero, and no Philox,
// when no record of the group has a threshold (thr_any == 0: nothing compares
// below 0).  hi_uniform is the batch's flag: a walker that instantiates its
// loop per value passes a constant and the test folds away.
template <int TPL, int NH>
__device__ __forceinline__ void stream_draws(const Ctx &c, const StreamBatch<TPL, NH> &bt, bool hi_uniform,
                                             uint32_t thr_any, uint32_t g, uint32_t (&x)[TPL][4]) {
#pragma unroll
  for (int u = 0; u < TPL; ++u) x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0;
  if (thr_any != 0) {
    if (hi_uniform) {
      philox_lockstep<TPL, NH>(bt, g, c.k0, c.k1, x);
    } else {
#pragma unroll
      for (int u = 0; u < TPL; ++u) {
        x[u][0] = bt.t_lo[u];
        x[u][1] = bt.t_hi[u];
        x[u][2] = g;
        philox10(x[u][0], x[u][1], x[u][2], x[u][3], c.k0, c.k1);
      }
    }
  }
}

// The same draws from the group's table entry (the batch is hi_uniform and
// its t_hi is the table's): no scalar rounds, and the threshold test is a bit
// of the entry.
template <int TPL, int NH, bool LEAN>
__device__ __forceinline__ void stream_draws_tab(const Ctx &c, const StreamBatch<TPL, NH, LEAN> &bt, const GroupEnt &e,
                                                 uint32_t (&x)[TPL][4]) {
  if (e.flags & kGroupAnyThr) {
    philox_lockstep_from<TPL, NH>(bt, c.k0, c.k1, e.uk0, e.uk1, e.d, x);
  } else {
    // the zeros stay in this (rare) branch: written before the test, as
    // `x = 0; if (...) philox`, they were 4 TPL v_mov in every group
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
#pragma unroll
    for (int u = 0; u < TPL; ++u) x[u][0] = x[u][1] = x[u][2] = x[u][3] = z;
  }
}

// A batch draws from the launch's group table when there is one, the batch
// does not straddle 2^32 and its t_hi is the one the table was built for (a
// launch that crosses 2^32: the batches before the crossing).
template <int TPL, int NH>
__device__ __forceinline__ bool use_group_table(const StreamBatch<TPL, NH> &bt, CEnt *tab, uint32_t tab_t_hi) {
  return tab != nullptr && bt.hi_uniform && bt.t_hi_u == tab_t_hi;
}

// Groups [g0, g1) through grp(records, entry, g), two per trip, each group's records
// loaded one group ahead into the other buffer; `cur` holds group g0 on entry
// and group g1 on return.  No register copy between the buffers: with
// `cur = nxt` the compiler waited for each prefetch right after issuing it,
// so every group paid the scalar load's latency.  Each load issues after the
// other buffer has arrived (an empty asm reads it): scalar loads return out of
// order, so a wait for that buffer placed after the load's issue would wait
// for the load too.
// TAB: the groups' table entries travel with their records (a second
// ping-pong buffer, ecur); else `tab` is not read and the entries are zero.
template <bool TAB, typename F>
__device__ __forceinline__ void stream_pingpong(CNode4 *__restrict__ stream, CEnt *__restrict__ tab, Node4 &cur,
                                                GroupEnt &ecur, uint32_t g0, uint32_t g1, F &&grp) {
  uint32_t g = g0;
  for (; g + 1 < g1; g += 2) {
    CNode4 *pb = stream + g + 1;
    GroupEnt eb{};
    if constexpr (TAB) {
      CEnt *qb = tab + g + 1;
      asm volatile("" : "+s"(pb), "+s"(qb) : "s"(cur.n[0].thr), "s"(ecur.flags));
      eb = load_ent(qb);
    } else {
      asm volatile("" : "+s"(pb) : "s"(cur.n[0].thr));
    }
    const Node4 b = load_group(pb);
    grp(cur, ecur, g);
    CNode4 *pc = stream + g + 2;
    if constexpr (TAB) {
      CEnt *qc = tab + g + 2;
      asm volatile("" : "+s"(pc), "+s"(qc) : "s"(b.n[0].thr), "s"(eb.flags));
      ecur = load_ent(qc);
    } else {
      asm volatile("" : "+s"(pc) : "s"(b.n[0].thr));
    }
    cur = load_group(pc);
    grp(b, eb, g + 1);
  }
  if (g < g1) {
    const Node4 b = load_group(stream + g + 1);
    GroupEnt eb{};
    if constexpr (TAB) eb = load_ent(tab + g + 1);
    grp(cur, ecur, g);
    cur = b;
    ecur = eb;
  }
}

// Every group of the stream through group(records, entry, g): group g + 1 is
// loaded before group g is processed and handed over by a loop-carried copy
// after it, so the s_waitcnt for the load lands after a whole group of Philox
// work.
template <bool TAB, typename F>
__device__ __forceinline__ void stream_one_ahead(CNode4 *__restrict__ stream, CEnt *__restrict__ tab,
                                                 uint32_t n_groups, F &&group) {
  Node4 cur = load_group(stream);
  GroupEnt ecur{};
  if constexpr (TAB) ecur = load_ent(tab);
  for (uint32_t g = 0; g < n_groups; ++g) {
    const Node4 nxt = load_group(stream + g + 1);
    GroupEnt enxt{};
    if constexpr (TAB) enxt = load_ent(tab + g + 1);
    group(cur, ecur, g);
    cur = nxt;
    ecur = enxt;
  }
}

// Mode B with a stack of open invocations (mode A: walk_stream_a).
// BS: the open invocations' statuses in a per-lane bit stack
// (bit p = running status of the frame at stack position p; VALU), for
// call depths <= 32 (kernel kind 5); otherwise (kind 4) as wave masks on a
// VGPR-lane stack.
template <bool LDSC, int TPL, bool BS>
__device__ __forceinline__ void walk_stream(const Ctx &c, CNode4 *__restrict__ stream, uint32_t n_groups,
                                            uint32_t n_nodes, uint64_t t_static, uint64_t trace_begin,
                                            uint64_t n_traces, uint64_t base, CEnt *__restrict__ tab,
                                            uint32_t tab_t_hi) {
  const StreamBatch<TPL, kHeldStack> bt(c, trace_begin, n_traces, base);
  const bool lane0 = lane_id() == 0;
  uint32_t errh[TPL];
  uint64_t root_st[TPL];
  // mode B: stack of open invocations; the top's running status in SGPRs
  uint64_t top[TPL];
  uint32_t top_slot = 0, depth = 0;
  LaneStack<uint64_t> s_mask[TPL];
  LaneStack<uint32_t> s_slot;
  // mode B, bit-stack form (BS): per lane and trace, bit p of stk_lo = the
  // running 500 status of the open frame at stack position p (p < 32)
  uint32_t stk_lo[TPL];
#pragma unroll
  for (int u = 0; u < TPL; ++u) {
    errh[u] = 0;
    root_st[u] = 0;
    top[u] = 0;
    stk_lo[u] = 0;
  }
  // set / test / clear bit p (wave-uniform, < 32) in the lanes of mask m: VALU only
  auto bs_set = [&](int u, uint32_t p, uint64_t m) {
    const uint32_t b = 1u << (p & 31u);
    stk_lo[u] |= lane_in(m) ? b : 0u;
  };
  auto bs_test = [&](int u, uint32_t p) -> uint64_t {
    const uint32_t b = 1u << (p & 31u);
    return ballot((stk_lo[u] & b) != 0u);
  };
  auto bs_clear = [&](int u, uint32_t p) {
    stk_lo[u] &= ~(1u << (p & 31u));
  };
  auto node = [&](uint32_t thr, uint32_t meta, const uint32_t (&xw)[TPL]) {
    const uint32_t slot = meta & 0xFFFFFFu;
    uint64_t own[TPL];
#pragma unroll
    for (int u = 0; u < TPL; ++u) own[u] = (meta & 0x80000000u) ? bt.all[u] : (ballot(xw[u] < thr) & bt.all[u]);
    if constexpr (BS) {
      if (slot == kSlotPad) return;
      uint32_t k = (meta >> 24) & 0x7Fu;
      const uint32_t d = depth;  // this invocation's stack position
      if (k > 0) {
        // a leaf opens and closes here: its status is its own draw; it
        // fails the caller (the open frame at d-1) in mode B
        uint64_t any = 0;
        uint32_t n = 0;
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
          add_lane(errh[u], own[u]);
          any |= own[u];
          n += popc(own[u]);
        }
        if (d == 0) {
#pragma unroll
          for (int u = 0; u < TPL; ++u) root_st[u] = own[u];
        } else if (any) {
          if (lane0) site_err_add<LDSC>(c, slot, n);
#pragma unroll
          for (int u = 0; u < TPL; ++u) bs_set(u, d - 1, own[u]);
        }
        --k;
      } else {
        uint64_t any = 0;
#pragma unroll
        for (int u = 0; u < TPL; ++u) any |= own[u];
        if (any) {
#pragma unroll
          for (int u = 0; u < TPL; ++u) bs_set(u, d, own[u]);
        }
        s_slot.put(d, slot);
        depth = d + 1;
      }
      for (; k > 0; --k) {  // the frame at position depth-1 closes
        const uint32_t p = depth - 1;
        uint64_t st[TPL], any = 0;
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
          st[u] = bs_test(u, p);
          any |= st[u];
        }
        if (p == 0) {
#pragma unroll
          for (int u = 0; u < TPL; ++u) {
            root_st[u] = st[u];
            add_lane(errh[u], st[u]);
          }
        } else if (any) {
          uint32_t n = 0;
#pragma unroll
          for (int u = 0; u < TPL; ++u) {
            add_lane(errh[u], st[u]);
            n += popc(st[u]);
            bs_set(u, p - 1, st[u]);  // mode B: a 500 fails the caller
            bs_clear(u, p);
          }
          if (lane0) site_err_add<LDSC>(c, s_slot.get(p), n);
        }
        depth = p;
      }
    } else {
      if (slot == kSlotPad) return;
      uint32_t k = (meta >> 24) & 0x7Fu;
      if (k > 0 && depth > 0) {
        // a leaf (opens and closes here): no push; its status is its own
        // draw, OR-ed into the caller's running status
        uint64_t any = 0;
        uint32_t n = 0;
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
          add_lane(errh[u], own[u]);
          any |= own[u];
          n += popc(own[u]);
          top[u] |= own[u];
        }
        if (any && lane0) site_err_add<LDSC>(c, slot, n);
        --k;
      } else {
        if (depth > 0) {
#pragma unroll
          for (int u = 0; u < TPL; ++u) s_mask[u].put(depth - 1, top[u]);
          s_slot.put(depth - 1, top_slot);
        }
#pragma unroll
        for (int u = 0; u < TPL; ++u) top[u] = own[u];
        top_slot = slot;
        ++depth;
      }
      for (; k > 0; --k) {  // subtree closes
        uint64_t any = 0;
        uint32_t n = 0;
        uint64_t st[TPL];
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
          st[u] = top[u];
          add_lane(errh[u], st[u]);
          any |= st[u];
          n += popc(st[u]);
        }
        if (any && top_slot != kSlotRoot && lane0) site_err_add<LDSC>(c, top_slot, n);
        --depth;
        if (depth > 0) {
#pragma unroll
          for (int u = 0; u < TPL; ++u) top[u] = s_mask[u].get(depth - 1) | st[u];  // mode B: 500 fails the caller
          top_slot = s_slot.get(depth - 1);
        } else {
#pragma unroll
          for (int u = 0; u < TPL; ++u) root_st[u] = st[u];
        }
      }
    }
  };
  // record 0 (in group 0) is the entry invocation (the client request).
  // T: the draws come from the group table (one instantiation of the loop
  // each, so the test stays out of it)
  auto groups = [&](auto T) {
    constexpr bool TAB = decltype(T)::value;
    stream_one_ahead<TAB>(stream, tab, n_groups, [&](const Node4 &q, const GroupEnt &e, uint32_t g) {
      uint32_t x[TPL][4];
      if constexpr (TAB) stream_draws_tab(c, bt, e, x);
      else stream_draws(c, bt, bt.hi_uniform, thr_or(q), g, x);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t xw[TPL];
#pragma unroll
        for (int u = 0; u < TPL; ++u) xw[u] = x[u][j];
        node(q.n[j].thr, q.n[j].meta, xw);
      }
    });
  };
  if (use_group_table(bt, tab, tab_t_hi)) groups(std::true_type{});
  else groups(std::false_type{});
#pragma unroll
  for (int u = 0; u < TPL; ++u) bt.finish(c, u, t_static, n_nodes, root_st[u], errh[u]);
}

// Mode A on the draw stream (kernel kind 4): an invocation's status is its own
// error draw, so per record and trace the vector unit runs one compare and
// one carried add (the trace's error count) and nothing else.  The record's
// 500 count is the popcount of its compare masks (scalar), at most 64 TPL, a
// byte: the four counts of a group are packed into one word and written to
// lane (g - g0) of a VGPR, one v_writelane per group.  After a chunk of 64
// groups each lane adds its group's four counts to the records' call sites
// (its group's records are loaded by vector loads before the chunk's Philox
// work).  No branch and no LDS operation per record; padding records and the
// entry (no call site) are dropped at the flush.
// FULL: every lane of every trace slot is valid.
// LEAN (isim_walk<4, false, LDSC, true>): the host has checked that every
// batch of the launch draws from the group table (walk_host.hip
// lean_walk_eligible: a table, and one high word for all trace ids), so only
// the table form of the chunk loop is instantiated.  With one loop instead of
// three the kernel has the registers to take no round key and no multiplier
// from an SGPR in the group loop (StreamBatch LEAN, kHeldLean).
constexpr uint32_t kCountGroups = 64;  // groups per chunk: one lane each
template <bool LDSC, int TPL, bool FULL, bool LEAN = false>
__device__ __forceinline__ void walk_stream_a(const Ctx &c, CNode4 *__restrict__ stream, uint32_t n_groups,
                                              uint32_t n_nodes, uint64_t t_static, uint64_t trace_begin,
                                              uint64_t n_traces, uint64_t base,
                                              const uint32_t *__restrict__ stream_w, CEnt *__restrict__ tab,
                                              uint32_t tab_t_hi) {
  const StreamBatch<TPL, LEAN ? kHeldLean : kHeldA, LEAN> bt(c, trace_begin, n_traces, base);
  static_assert(64 * TPL < 256, "a record's 500 count is packed into a byte");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t lane = lane_id();
  uint32_t errh[TPL];
  uint64_t root_st[TPL];
#pragma unroll
  for (int u = 0; u < TPL; ++u) errh[u] = 0;

  Node4 cur = load_group(stream);
  {  // record 0 is the entry invocation (the client request): its status is the trace's
    uint32_t x[TPL][4];
    if constexpr (LEAN) {
      // the table's t_hi is the valid lanes': an invalid lane of the last
      // batch may lie past 2^32, and its draw is masked.  (With the scalar
      // rounds here, as in the general kernel, the whole kernel was scheduled
      // differently and config 3 ran 5 % slower: DESIGN.md §5.)
      const GroupEnt e0 = load_ent(tab);
      philox_lockstep_from(bt, c.k0, c.k1, e0.uk0, e0.uk1, e0.d, x);
    } else {
      stream_draws(c, bt, bt.hi_uniform, ~0u, 0, x);
    }
#pragma unroll
    for (int u = 0; u < TPL; ++u)
      root_st[u] = (cur.n[0].meta & 0x80000000u) ? bt.all[u] : (ballot(x[u][0] < cur.n[0].thr) & bt.all[u]);
  }
  // DR: where the groups' draws come from (one instantiation of the loop
  // each, so the test stays out of it): 2 the launch's group table, 1 lockstep
  // blocks with the scalar rounds here (the batch does not straddle 2^32),
  // 0 a block per trace
  auto chunks = [&](auto DR) {
    constexpr bool TAB = decltype(DR)::value == 2;
    GroupEnt ecur{};
    if constexpr (TAB) ecur = load_ent(tab);
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kCountGroups) {
      const uint32_t ng = n_groups - g0 < kCountGroups ? n_groups - g0 : kCountGroups;
      // this lane's group of the chunk (thr, meta of its four records)
      u32x4 ra = {0u, kSlotPad, 0u, kSlotPad}, rb = ra;
      if (lane < ng) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(stream_w + 8u * (size_t)(g0 + lane));
        ra = p[0];
        rb = p[1];
      }
      uint32_t pk = 0;  // lane l: the 500 counts of group g0 + l, a byte per record
      // one group: its Philox blocks, per record and trace the compare and the
      // carried add, the four counts into the group's lane of pk
      stream_pingpong<TAB>(stream, tab, cur, ecur, g0, g0 + ng, [&](const Node4 &q, const GroupEnt &e, uint32_t g) {
        uint32_t x[TPL][4];
        bool any_always;  // the group holds an errorRate-1 record
        if constexpr (TAB) {
          stream_draws_tab(c, bt, e, x);
          any_always = (int32_t)e.flags < 0;  // kGroupAnyAlways
        } else {
          uint64_t qor = 0;  // s_or_b64: both tests of the group from three scalar ORs of its (thr, meta) pairs
#pragma unroll
          for (int j = 0; j < 4; ++j) qor |= u64of(q.n[j].thr, q.n[j].meta);
          stream_draws(c, bt, decltype(DR)::value == 1, (uint32_t)qor, g, x);
          any_always = (int64_t)qor < 0;
        }
        uint64_t own[TPL][4];
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t n = 0;
#pragma unroll
          for (int u = 0; u < TPL; ++u) {
            own[u][j] = ballot(x[u][j] < q.n[j].thr);
            if constexpr (!FULL) own[u][j] &= bt.all[u];
            add_lane(errh[u], own[u][j]);
            n += popc(own[u][j]);
          }
          w |= n << (8 * j);
        }
        // errorRate-1 records (always 500, thr 0: no lane counted above) are
        // rare: one test per group, a test per record only in the groups
        // that hold one
        if (any_always) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!(q.n[j].meta & 0x80000000u)) continue;
            uint32_t n = 0;
#pragma unroll
            for (int u = 0; u < TPL; ++u) {
              own[u][j] = FULL ? ~0ull : bt.all[u];
              add_lane(errh[u], own[u][j]);
              n += popc(own[u][j]);
            }
            w |= n << (8 * j);
          }
        }
        pk = wrl(w, g - g0, pk);
      });
      const uint32_t slot[4] = {ra.y & 0xFFFFFFu, ra.w & 0xFFFFFFu, rb.y & 0xFFFFFFu, rb.w & 0xFFFFFFu};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t n = (pk >> (8 * j)) & 0xFFu;
        if (n != 0 && slot[j] < kSlotPad) site_err_add<LDSC>(c, slot[j], n);
      }
    }
  };
  if constexpr (LEAN) {
    chunks(std::integral_constant<int, 2>{});
  } else {
    if (use_group_table(bt, tab, tab_t_hi)) chunks(std::integral_constant<int, 2>{});
    else if (bt.hi_uniform) chunks(std::integral_constant<int, 1>{});
    else chunks(std::integral_constant<int, 0>{});
  }
#pragma unroll
  for (int u = 0; u < TPL; ++u) bt.finish(c, u, t_static, n_nodes, root_st[u], errh[u]);
}

typedef const __attribute__((address_space(4))) StreamClose CClose;
typedef const __attribute__((address_space(4))) uint32_t CU32;
struct CloseBlk {
  StreamClose c[8];
};
__device__ __forceinline__ CloseBlk load_closes(CClose *p) {  // one s_load_dwordx16
  CloseBlk r;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    r.c[k].pre1 = p[k].pre1;
    r.c[k].rmask = p[k].rmask;
  }
  return r;
}

// Mode B on the draw stream without a stack (kernel kind 6).  An invocation
// responds 500 iff some invocation of its subtree drew an error (a 500 fails
// the caller's step, and the caller's step failure is its 500), and a
// subtree is the contiguous stream range [p, j] (DFS preorder).  So a lane
// only keeps, per trace, the error bits of the current chunk of 32 records
// (shifted in, one v_addc per record) and the position + 1 of its last
// erring record before the chunk; after each chunk the closes that end in it
// are tested against both (StreamClose, kernel_abi.h) and counted (a lane
// per close, one ds_add per 64 closes).  Leaves respond with their own draw
// (a lane per record, one ds_add per chunk); the entry's status is "any
// error at all".  No call-depth limit, no per-record branching
// on the stack.
template <bool LDSC, int TPL, bool FULL>
__device__ __forceinline__ void walk_stream_cl(const Ctx &c, CNode4 *__restrict__ stream, uint32_t n_groups,
                                               uint32_t n_nodes, uint64_t t_static, uint64_t trace_begin,
                                               uint64_t n_traces, uint64_t base, CClose *__restrict__ closes,
                                               const uint32_t *__restrict__ close_slot, CU32 *__restrict__ close_end,
                                               const uint32_t *__restrict__ stream_w, CEnt *__restrict__ tab,
                                               uint32_t tab_t_hi) {
  const StreamBatch<TPL, kHeldCl> bt(c, trace_begin, n_traces, base);
  const uint32_t lane = lane_id();
  uint32_t errh[TPL], le[TPL];
#pragma unroll
  for (int u = 0; u < TPL; ++u) errh[u] = le[u] = 0;

  Node4 cur = load_group(stream);
  const bool use_tab = use_group_table(bt, tab, tab_t_hi);
  GroupEnt ecur{};
  if (use_tab) ecur = load_ent(tab);
  uint32_t cp = 0;
  const uint32_t n_chunks = (n_groups + kChunkGroups - 1) / kChunkGroups;
  for (uint32_t ch = 0; ch < n_chunks; ++ch) {
    const uint32_t g0 = ch * kChunkGroups;
    const uint32_t g1 = g0 + kChunkGroups < n_groups ? g0 + kChunkGroups : n_groups;
    // the chunk's first 64 close slots (one per lane), loaded before its Philox work
    uint32_t slotv = close_slot[cp + lane];  // zero tail padding
    const uint32_t nrec = 4u * (g1 - g0);
    const uint32_t rmeta = lane < nrec ? stream_w[2u * (ch * kChunkRecords + lane) + 1u] : kSlotPad;
    uint32_t lcnt = 0;
    uint32_t mb[TPL];
#pragma unroll
    for (int u = 0; u < TPL; ++u) mb[u] = 0;
    // one group: its Philox blocks, then per record the error bits shifted
    // into mb and the record's count in lane r of lcnt
    // T: the draws come from the group table (chosen per chunk, outside the
    // group loop)
    auto groups = [&](auto T) {
      constexpr bool TAB = decltype(T)::value;
      stream_pingpong<TAB>(stream, tab, cur, ecur, g0, g1, [&](const Node4 &q, const GroupEnt &e, uint32_t g) {
        uint32_t x[TPL][4];
        if constexpr (TAB) stream_draws_tab(c, bt, e, x);
        else stream_draws(c, bt, bt.hi_uniform, thr_or(q), g, x);
        auto records = [&](bool always) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t thr = q.n[j].thr, meta = q.n[j].meta;
            uint32_t n = 0;
#pragma unroll
            for (int u = 0; u < TPL; ++u) {
              uint64_t own = ballot(x[u][j] < thr);
              if (always && (meta & 0x80000000u)) own = ~0ull;
              shift_in(mb[u], own);
              if constexpr (!FULL) own &= bt.all[u];
              n += popc(own);
            }
            lcnt = wrl(n, 4u * (g - g0) + j, lcnt);  // lane r: record r's count
          }
        };
        // errorRate-1 records (always 500) are rare: a branch per record only
        // in the groups that hold one
        bool any_always;
        if constexpr (TAB) any_always = (e.flags & kGroupAnyAlways) != 0;
        else any_always = ((q.n[0].meta | q.n[1].meta | q.n[2].meta | q.n[3].meta) & 0x80000000u) != 0;
        if (!any_always) records(false);
        else records(true);
      });
    };
    if (use_tab) groups(std::true_type{});
    else groups(std::false_type{});
    // leaves respond with their own draw: their error counts (lane r =
    // record r) go to the site table in one ds_add, their 500s to errh
    {
      const uint32_t rslot = rmeta & 0xFFFFFFu;
      const bool leaf = (rmeta & 0x7F000000u) != 0 && rslot < kSlotPad;
      const uint32_t lm = __builtin_bitreverse32((uint32_t)ballot(leaf)) >> (32u - nrec);  // mb's bit order
#pragma unroll
      for (int u = 0; u < TPL; ++u) errh[u] += (uint32_t)__builtin_popcount(mb[u] & lm);
      if (leaf && lcnt) site_err_add<LDSC>(c, rslot, lcnt);
    }
    const uint32_t ce = close_end[ch];
    CloseBlk blk = load_closes(closes + cp);  // the chunk's first 8 closes
    // calling invocations whose subtree ends in this chunk, in segments of
    // up to 64: close i of a segment keeps its count in lane i of cntv, and
    // the segment's counts go to the site table in one ds_add
    while (cp < ce) {
      const uint32_t nseg = ce - cp < 64u ? ce - cp : 64u;
      uint32_t cntv = 0;
      for (uint32_t i = 0; i < nseg; i += 8) {
        const CloseBlk nb = load_closes(closes + cp + i + 8);  // zero tail padding
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (i + k >= nseg) break;
          const uint32_t pre1 = blk.c[k].pre1, rmask = blk.c[k].rmask;
          uint32_t n = 0;
#pragma unroll
          for (int u = 0; u < TPL; ++u) {
            uint64_t st = ballot((mb[u] & rmask) != 0u) | ballot(le[u] >= pre1);
            if constexpr (!FULL) st &= bt.all[u];
            add_lane(errh[u], st);
            n += popc(st);
          }
          cntv = wrl(n, i + k, cntv);
        }
        blk = nb;
      }
      if (lane < nseg && (LDSC || cntv)) site_err_add<LDSC>(c, slotv, cntv);
      cp += nseg;
      if (cp < ce) slotv = close_slot[cp + lane];  // a chunk with more than 64 closes
    }
    const uint32_t top = ch * kChunkRecords + 4u * (g1 - g0);
#pragma unroll
    for (int u = 0; u < TPL; ++u) le[u] = mb[u] ? top - (uint32_t)__builtin_ctz(mb[u]) : le[u];
  }
#pragma unroll
  for (int u = 0; u < TPL; ++u) {
    const uint64_t root_st = ballot(le[u] != 0u) & bt.all[u];
    add_lane(errh[u], root_st);
    bt.finish(c, u, t_static, n_nodes, root_st, errh[u]);
  }
}

// Mode B on the draw stream by sparse ancestor marking (kernel kind 8, the
// default; kernel_abi.h kMarkPadKey).  The walk is mode A's — one Philox block
// per group of 4 records, one compare per record and trace — plus, per record
// and trace, one v_min of the record's key into the lane's running minimum
// since its trace's last error.  Only where some lane errs (the branch mode A
// takes for its counters anyway) the erring lanes mark: +1 at the record (one
// ds_add for the wave), -1 at the LCA that minimum names (a ds_sub per
// erring lane), and the trace's new 500s depth(e) - depth(LCA) into its error
// count.  The entry responds 500 iff its trace erred at all.  Costs against
// the close list (kind 6): no per-chunk close tests (4,389 per trace on
// config 3), no error-bit shifts, no call-depth limit.
template <int TPL, bool FULL>
__device__ __forceinline__ void walk_stream_mark(const Ctx &c, CNode4 *__restrict__ stream, uint32_t n_groups,
                                                 uint32_t n_nodes, uint64_t t_static, uint64_t trace_begin,
                                                 uint64_t n_traces, uint64_t base, CEnt *__restrict__ tab,
                                                 uint32_t tab_t_hi) {
  const StreamBatch<TPL, kHeldMark> bt(c, trace_begin, n_traces, base);
  const bool lane0 = lane_id() == 0;
  uint32_t errh[TPL], mk[TPL];
#pragma unroll
  for (int u = 0; u < TPL; ++u) {
    errh[u] = 0;
    mk[u] = 0xFFFFFFFFu;
  }
  uint32_t *marks = c.cnt;
  // T: the draws come from the group table (one instantiation of the loop
  // each, so the test stays out of it)
  auto groups = [&](auto T) {
    constexpr bool TAB = decltype(T)::value;
    stream_one_ahead<TAB>(stream, tab, n_groups, [&](const Node4 &q, const GroupEnt &e, uint32_t g) {
      uint32_t x[TPL][4];
      if constexpr (TAB) stream_draws_tab(c, bt, e, x);
      else stream_draws(c, bt, bt.hi_uniform, thr_or(q), g, x);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t kw = q.n[j].meta;
        const uint32_t key = kw & kMarkKeyMask;
        const uint64_t always = (kw & 0x80000000u) ? ~0ull : 0ull;  // errorRate 1: no draw, always 500
        uint64_t own[TPL], any = 0;
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
          own[u] = ballot(x[u][j] < q.n[j].thr) | always;
          if constexpr (!FULL) own[u] &= bt.all[u];
          mk[u] = mk[u] < key ? mk[u] : key;
          any |= own[u];
        }
        if (any) {
          uint32_t n = 0;
#pragma unroll
          for (int u = 0; u < TPL; ++u) n += popc(own[u]);
          if (lane0) atomicAdd(marks + 4u * g + (uint32_t)j, n);
          const uint32_t d1 = (key >> 24) + 1u;
#pragma unroll
          for (int u = 0; u < TPL; ++u) {
            if (lane_in(own[u])) {
              atomicSub(marks + (mk[u] & kMarkPosMask), 1u);
              errh[u] += d1 - (mk[u] >> 24);
              mk[u] = 0xFFFFFFFFu;
            }
          }
        }
      }
    });
  };
  if (use_group_table(bt, tab, tab_t_hi)) groups(std::true_type{});
  else groups(std::false_type{});
#pragma unroll
  for (int u = 0; u < TPL; ++u) bt.finish(c, u, t_static, n_nodes, ballot(errh[u] != 0u) & bt.all[u], errh[u]);
}

}  // namespace dev
}  // namespace isim
