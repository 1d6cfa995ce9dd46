// DES item engine, stages 4a, 4c and 5: a round's
// step begins, a finish group's finishes with their statistics, and the
// batch's records and latency statistics.  A part of des_items.hip, included
// inside namespace isim::dit after des_items_k.h.
#pragma once

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
