// DES item engine, stage 6: the span tap.  A
// part of des_items.hip, included inside namespace isim::dit after
// des_items_prewalk.h (it reads the tree's nodes as the pre-walk does).
#pragma once

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
