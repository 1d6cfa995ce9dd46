// The DES level engine's up pass: a thread's quad of
// finishes in 64-bit and, for narrow rows, 32-bit arithmetic, the des_up
// kernel over (position, trace-range) blocks, and des_finalize.
//
// Included by des.hip INSIDE namespace isim::dev, after des_rows.h and the
// statistics helpers (as des_draw.h: a piece of that translation unit, not a
// header of its own).

// One thread's 4 consecutive traces of the up pass (FULL: all below te, so
// every row access is one vector load).  Every load of the quad is issued
// before any arithmetic (start, arrival and step-begin rows, the status word,
// the first kUpCB children's finish rows: one memory round trip, not five);
// children past kUpCB (hubs) follow in batches.  `ch`: the child positions,
// staged in LDS by the workgroup when they fit.
template <typename T>
constexpr uint32_t kUpCB = sizeof(T) == 4 ? ISIM_DES_UP_CB : 2;  // children rows in flight with the rest
constexpr uint32_t kUpChildLds = kDesUpChildLds;  // child ids staged in LDS per workgroup
// Per-block state of the durations a caller records for its flagged callees
// (kDesFlagParentDur): per callee (index j < kDesDurKids) the histogram, the
// start sum S(caller) over the traces where the callee responded 500 and
// their count; the callee's own block adds its finish sums by status, the
// caller's subtracts the arrivals S(caller) + off (Σ over all its traces: ss).
struct UpKids {
  uint32_t nd;                // flagged callees
  const uint32_t *dch;        // [j]: the callee's position
  const uint64_t *doff;       // [j]: the callee's off
  uint32_t *dhist;            // [j][2 * ISIM_N_PROM]
  unsigned long long *ds5;    // [j]
  uint32_t *dn5;              // [j]
};

// OWN: the block records its position's durations (its arrival row is read);
// else they are 0 (the entry: des_finalize) or its caller's (PDUR sums: the
// finishes by status).  DK: the block records its flagged callees' durations.
// NS: the finish needs no start row (kDesFlagNoStart, no callee durations here)
template <typename T, bool FULL, bool OWN, bool DK, bool NS = false>
__device__ __forceinline__ void up_quad(const DesK &k, const DesPos &P, uint32_t v, uint64_t b0, uint64_t te,
                                        T *fin, const T *arow, uint64_t off, bool leaf, bool pdur,
                                        const T *mrow, uint32_t c_max_from, const uint32_t *ch,
                                        const uint32_t (&id0)[kUpCB<T>], uint32_t *hist, const uint8_t *lut,
                                        const UpKids &dk, uint64_t &ss,
                                        uint64_t &dsum0, uint64_t &dsum1, uint64_t &n500, bool &bad) {
  __asm__ volatile("" : "+v"(b0));  // opaque to loop strength reduction (down1_chunk)
  constexpr Quad Q = FULL ? Quad::whole : Quad::test;
  const uint32_t cnt = leaf ? 0u : P.child_cnt;
  T ar[kPer], mr[kPer];
  T f0[kUpCB<T>][kPer];
  // 1. the loads (no branch around the row loads: a branch that merges
  // loaded values makes the compiler wait for them inside it)
  if constexpr (OWN) load_row<T, Q>(arow, b0, te, ar);
  if constexpr (NS) {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) mr[i] = 0;
  } else {
    load_row<T, Q>(mrow, b0, te, mr);
  }
  const uint32_t stm = des_status4(k, v, b0);
#pragma unroll
  for (uint32_t j = 0; j < kUpCB<T>; ++j)
    if (j < cnt) load_row<T, Q>(row<T>(k.WF, k.ld, id0[j]), b0, te, f0[j]);
  // 2. the arithmetic
  uint64_t a[kPer], m[kPer];
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    a[i] = OWN ? (uint64_t)ar[i] + off : 0;
    m[i] = NS ? 0 : (uint64_t)mr[i] + P.floor;  // NS: max_c F(c) >= S + floor
    if constexpr (DK) ss += FULL || b0 + i < te ? (uint64_t)mr[i] : 0;  // S(caller): no step begins (plan)
  }
  uint32_t sto = 0;  // children's 500s, bit i
  if (cnt) {
    T cm[kPer] = {0, 0, 0, 0};
    auto take = [&](const T (&f)[kPer], bool in_max) {
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) {
        const T tc = f[i] & (T)Row<T>::kMask;
        if (in_max) cm[i] = tc > cm[i] ? tc : cm[i];
        sto |= (uint32_t)(f[i] >> Row<T>::kTop) << i;
      }
    };
#pragma unroll
    for (uint32_t j = 0; j < kUpCB<T>; ++j)
      if (j < cnt) take(f0[j], j >= c_max_from);
    for (uint32_t c = kUpCB<T>; c < cnt; c += kUpCB<T>) {
      T f[kUpCB<T>][kPer];
#pragma unroll
      for (uint32_t j = 0; j < kUpCB<T>; ++j)
        if (c + j < cnt) load_row<T, Q>(row<T>(k.WF, k.ld, ch[c + j]), b0, te, f[j]);
#pragma unroll
      for (uint32_t j = 0; j < kUpCB<T>; ++j)
        if (c + j < cnt) take(f[j], c + j >= c_max_from);
    }
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) m[i] = (uint64_t)cm[i] > m[i] ? (uint64_t)cm[i] : m[i];
  }
  uint64_t o[kPer];
  uint32_t bin[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin};
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    const uint64_t t = b0 + i;
    o[i] = 0;
    if (FULL || t < te) {
      const uint64_t F = leaf ? m[i] : m[i] + P.post;
      const uint32_t own = (stm >> i) & 1u;
      const uint32_t st = k.modeb ? (own | ((sto >> i) & 1u)) : own;
      // OWN: the duration; a caller-recorded position: its finish (the
      // caller subtracts the arrival); the entry: 0 (des_finalize)
      const uint64_t dur = OWN ? F - a[i] : pdur ? F : 0;
      bad |= !Row<T>::fits(F);
      o[i] = F | ((uint64_t)st << Row<T>::kTop);
      if (st && !k.quiet) atomicAdd(k.E + t, 1u);
      n500 += st;
      dsum1 += st ? dur : 0;
      dsum0 += st ? 0 : dur;
      if constexpr (OWN) bin[i] = st * ISIM_N_PROM + des_prom_bucket(lut, dur);
    }
  }
  if constexpr (OWN) hist_add4<FULL>(hist, bin);
  T ot[kPer];
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) ot[i] = (T)o[i];
  track4<T, Q>(k, fin, b0, te, ot);
  store_row<T, Q, Mem::plain>(fin, b0, te, ot);
  if constexpr (DK) {
    // the flagged callees' durations F(c) - (S + off(c)): their finish rows
    // again (just read above: cache hits), after the quad's own work so the
    // children loop keeps its registers
    for (uint32_t j = 0; j < dk.nd; ++j) {
      T f[kPer];
      load_row<T, Q>(row<T>(k.WF, k.ld, dk.dch[j]), b0, te, f);
      const uint64_t offc = dk.doff[j];
      uint32_t cb[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin};
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) {
        if (FULL || b0 + i < te) {
          const uint64_t dur = (uint64_t)(f[i] & (T)Row<T>::kMask) - ((uint64_t)mr[i] + offc);
          const uint32_t st = (uint32_t)(f[i] >> Row<T>::kTop);
          cb[i] = st * ISIM_N_PROM + des_prom_bucket(lut, dur);
          if (st) {
            atomicAdd(dk.ds5 + j, (unsigned long long)mr[i]);
            atomicAdd(dk.dn5 + j, 1u);
          }
        }
      }
      hist_add4<FULL>(dk.dhist + j * 2 * ISIM_N_PROM, cb);
    }
  }
}

// up_quad for narrow rows in 32-bit arithmetic (round 3): every value below
// 2^31 + 2^30 (row values < 2^31, the host-checked off / floor / post
// < 2^30: DesPlan::up_n32), so no 64-bit time in the quad — fewer VGPRs,
// more waves of loads in flight.  The same results as up_quad<uint32_t, ...>.
template <bool FULL, bool OWN, bool DK, bool NS>
__device__ __forceinline__ void up_quad32(const DesK &k, const DesPos &P, uint32_t v, uint64_t b0, uint64_t te,
                                          uint32_t *fin, const uint32_t *arow, uint32_t off32, bool leaf, bool pdur,
                                          const uint32_t *mrow, const uint32_t *ch, const uint32_t (&id0)[kUpCB<uint32_t>],
                                          uint32_t *hist, const uint8_t *lut, const UpKids &dk, uint64_t &ss,
                                          uint64_t &dsum0, uint64_t &dsum1, uint32_t &n500, bool &bad) {
  using T = uint32_t;
  __asm__ volatile("" : "+v"(b0));  // opaque to loop strength reduction (down1_chunk)
  constexpr Quad Q = FULL ? Quad::whole : Quad::test;
  const uint32_t cnt = leaf ? 0u : P.child_cnt;
  T ar[kPer], mr[kPer];
  T f0[kUpCB<T>][kPer];
  if constexpr (OWN) load_row<T, Q>(arow, b0, te, ar);
  if constexpr (NS) {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) mr[i] = 0;
  } else {
    load_row<T, Q>(mrow, b0, te, mr);
  }
  const uint32_t stm = des_status4(k, v, b0);
#pragma unroll
  for (uint32_t j = 0; j < kUpCB<T>; ++j)
    if (j < cnt) load_row<T, Q>(row<T>(k.WF, k.ld, id0[j]), b0, te, f0[j]);
  const uint32_t floor32 = (uint32_t)P.floor, post32 = leaf ? 0u : (uint32_t)P.post;
  uint32_t m[kPer];
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    m[i] = NS ? 0u : mr[i] + floor32;  // NS: max_c F(c) >= S + floor
    if constexpr (DK) ss += FULL || b0 + i < te ? (uint64_t)mr[i] : 0;
  }
  uint32_t sto = 0;  // children's 500s, bit i
  auto take = [&](const T (&f)[kPer]) {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      const T tc = f[i] & 0x7FFFFFFFu;
      m[i] = tc > m[i] ? tc : m[i];
      sto |= (f[i] >> 31) << i;
    }
  };
#pragma unroll
  for (uint32_t j = 0; j < kUpCB<T>; ++j)
    if (j < cnt) take(f0[j]);
  for (uint32_t c = kUpCB<T>; c < cnt; c += kUpCB<T>) {
    T f[kUpCB<T>][kPer];
#pragma unroll
    for (uint32_t j = 0; j < kUpCB<T>; ++j)
      if (c + j < cnt) load_row<T, Q>(row<T>(k.WF, k.ld, ch[c + j]), b0, te, f[j]);
#pragma unroll
    for (uint32_t j = 0; j < kUpCB<T>; ++j)
      if (c + j < cnt) take(f[j]);
  }
  T o[kPer];
  uint32_t bin[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin}, big = 0;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    const uint64_t t = b0 + i;
    o[i] = 0;
    if (FULL || t < te) {
      const uint32_t F = m[i] + post32;
      const uint32_t own = (stm >> i) & 1u;
      const uint32_t st = k.modeb ? (own | ((sto >> i) & 1u)) : own;
      // OWN: the duration; a caller-recorded position: its finish (the
      // caller subtracts the arrival); the entry: 0 (des_finalize)
      const uint32_t dur = OWN ? F - (ar[i] + off32) : pdur ? F : 0u;
      big |= F;
      o[i] = F | (st << 31);
      if (st && !k.quiet) atomicAdd(k.E + t, 1u);
      n500 += st;
      dsum1 += st ? dur : 0u;
      dsum0 += st ? 0u : dur;
      if constexpr (OWN) bin[i] = st * ISIM_N_PROM + des_prom_bucket32(lut, dur);
    }
  }
  bad |= (big >> 31) != 0u;
  if constexpr (OWN) hist_add4<FULL>(hist, bin);
  track4<T, Q>(k, fin, b0, te, o);
  store_row<T, FULL ? Quad::whole : Quad::each, Mem::nontemporal>(fin, b0, te, o);
  if constexpr (DK) {
    // the flagged callees' durations F(c) - (S + off(c)) (up_quad)
    for (uint32_t j = 0; j < dk.nd; ++j) {
      T f[kPer];
      load_row<T, Q>(row<T>(k.WF, k.ld, dk.dch[j]), b0, te, f);
      const uint32_t offc = (uint32_t)dk.doff[j];
      uint32_t cb[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin};
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) {
        if (FULL || b0 + i < te) {
          const uint32_t dur = (f[i] & 0x7FFFFFFFu) - (mr[i] + offc);
          const uint32_t st = f[i] >> 31;
          cb[i] = st * ISIM_N_PROM + des_prom_bucket32(lut, dur);
          if (st) {
            atomicAdd(dk.ds5 + j, (unsigned long long)mr[i]);
            atomicAdd(dk.dn5 + j, 1u);
          }
        }
      }
      hist_add4<FULL>(dk.dhist + j * 2 * ISIM_N_PROM, cb);
    }
  }
}

// ---- up pass: finish times, statuses, per-service durations.
// (position, trace-range) blocks; 4 consecutive traces per thread.
// N32: narrow rows and every finish constant below 2^30 (DesPlan::up_n32): up_quad32
template <typename T, bool N32>
__global__ void __launch_bounds__(kDesUpThreads, N32 ? ISIM_DES_UP32_WAVES : ISIM_DES_UP_WAVES) des_up(DesK k) {
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ uint64_t red[3 * kDesUpThreads / 64];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  __shared__ uint64_t s_doff[kDesDurKids];
  __shared__ uint32_t s_dch[kDesDurKids], s_nd;
  __shared__ uint32_t dhist[kDesDurKids * 2 * ISIM_N_PROM];
  __shared__ unsigned long long ds5[kDesDurKids];
  __shared__ uint32_t dn5[kDesDurKids];
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDesUpThreads) hist[i] = 0;
  des_bucket_lut_init(lut);
  if (threadIdx.x == 0) s_nd = 0;
  const uint32_t v = k.level_pos[k.level_begin + blockIdx.y];
  const DesPos P = k.pos[v];
  const uint64_t N = k.N;
  // trace range: split boundaries on multiples of 16 (aligned vector accesses)
  const uint64_t tb = blockIdx.x ? (N * blockIdx.x / k.splits) & ~15ull : 0;
  const uint64_t te = blockIdx.x + 1 == k.splits ? N : (N * (blockIdx.x + 1) / k.splits) & ~15ull;
  const T *mine = row<T>(k.W, k.ld, v);
  T *fin = row<T>(k.WF, k.ld, v);
  const DesPosExt X = k.ext[v];
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  const bool leaf = P.flags & kDesFlagLeaf;
  const bool pdur = (P.flags & kDesFlagParentDur) != 0;
  const bool own = par && !pdur;  // the block records the position's durations
  // several call steps: F = max(BK_last + floor, max F(last step's callees)) + post
  const T *base_t = X.bk_last == kDesNone ? nullptr : row<T>(k.BK, k.ld, X.bk_last);
  const uint32_t c_max_from = X.bk_last == kDesNone ? 0u : X.last_child;
  uint64_t dsum0 = 0, dsum1 = 0, n500 = 0, ss = 0;
  uint32_t n500_32 = 0;
  bool bad = false;
  // rows read: the arrival row when the block records the durations, and the
  // row F's floor starts from (the last step's begin, or S)
  const T *arow = par;
  const T *mrow = base_t ? base_t : mine;
  // the child positions: in LDS when they fit (read by every quad; LDS
  // addressing known to the compiler, not flat), else from global memory;
  // with them, which are flagged callees (the plan flags only callees of
  // callers with at most kUpChildLds children)
  __shared__ uint32_t s_ch[kUpChildLds];
  const uint32_t cnt = leaf ? 0u : P.child_cnt;
  const uint32_t *gch = k.child + P.child_off;
  __syncthreads();  // s_nd
  UpKids dk{0, s_dch, s_doff, dhist, ds5, dn5};
  auto run = [&](const uint32_t *ch, auto own_t, auto dk_t, auto ns_t) {
    constexpr bool OWN = decltype(own_t)::value, DK = decltype(dk_t)::value, NS = decltype(ns_t)::value;
    // the first children's positions in (uniform) registers for the whole
    // range: their row loads issue with the others, no id load in front
    uint32_t id0[kUpCB<T>];
#pragma unroll
    for (uint32_t j = 0; j < kUpCB<T>; ++j) id0[j] = j < cnt ? ch[j] : 0u;
    for (uint64_t b0 = tb + (uint64_t)threadIdx.x * kPer; b0 < te; b0 += (uint64_t)kPer * kDesUpThreads) {
      if constexpr (N32 && sizeof(T) == 4) {
        if (b0 + kPer <= te)
          up_quad32<true, OWN, DK, NS>(k, P, v, b0, te, fin, arow, (uint32_t)off, leaf, pdur, mrow, ch, id0, hist, lut,
                                       dk, ss, dsum0, dsum1, n500_32, bad);
        else
          up_quad32<false, OWN, DK, NS>(k, P, v, b0, te, fin, arow, (uint32_t)off, leaf, pdur, mrow, ch, id0, hist, lut,
                                        dk, ss, dsum0, dsum1, n500_32, bad);
      } else {
        if (b0 + kPer <= te)
          up_quad<T, true, OWN, DK, NS>(k, P, v, b0, te, fin, arow, off, leaf, pdur, mrow, c_max_from, ch, id0, hist,
                                        lut, dk, ss, dsum0, dsum1, n500, bad);
        else
          up_quad<T, false, OWN, DK, NS>(k, P, v, b0, te, fin, arow, off, leaf, pdur, mrow, c_max_from, ch, id0, hist,
                                         lut, dk, ss, dsum0, dsum1, n500, bad);
      }
    }
  };
  using tt = std::true_type;
  using ff = std::false_type;
  uint32_t nd = 0;
  if (cnt <= kUpChildLds) {
    for (uint32_t i = threadIdx.x; i < cnt; i += kDesUpThreads) {
      const uint32_t c = gch[i];
      s_ch[i] = c;
      const uint32_t f = k.pos[c].flags;
      if (f & kDesFlagParentDur) {
        const uint32_t j = (f >> kDesDurShift) & 0xFFu;
        s_doff[j] = k.pos[c].off;
        s_dch[j] = c;
        atomicMax(&s_nd, j + 1);
      }
    }
    __syncthreads();
    nd = s_nd;
    dk.nd = nd;
    for (uint32_t i = threadIdx.x; i < nd * 2 * ISIM_N_PROM; i += kDesUpThreads) dhist[i] = 0;
    if (threadIdx.x < nd) {
      ds5[threadIdx.x] = 0;
      dn5[threadIdx.x] = 0;
    }
    __syncthreads();
    const bool ns = (P.flags & kDesFlagNoStart) != 0;
    if (nd) {
      if (own) run(s_ch, tt{}, tt{}, ff{});
      else run(s_ch, ff{}, tt{}, ff{});
    } else if (ns) {
      if (own) run(s_ch, tt{}, ff{}, tt{});
      else run(s_ch, ff{}, ff{}, tt{});
    } else {
      if (own) run(s_ch, tt{}, ff{}, ff{});
      else run(s_ch, ff{}, ff{}, ff{});
    }
  } else {
    if (own) run(gch, tt{}, ff{}, ff{});
    else run(gch, ff{}, ff{}, ff{});
  }
  n500 += n500_32;
  flag_overflow(k, bad);
  if (k.quiet) return;
  if (nd) {
    // the flagged callees' histograms, and their duration sums less the
    // arrivals: Σ (S + off) over this block's traces, by the callee's status
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) ss += __shfl_xor(ss, d, 64);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    uint64_t sall = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDesUpThreads / 64; ++w) sall += red[w];
    for (uint32_t i = threadIdx.x; i < nd * 2 * ISIM_N_PROM; i += kDesUpThreads) {
      const uint32_t j = i / (2 * ISIM_N_PROM), b = i - j * (2 * ISIM_N_PROM);
      if (dhist[i])
        atomicAdd((unsigned long long *)(k.table + (uint64_t)k.pos[s_dch[j]].row * ISIM_DES_ROW_WORDS + b),
                  (unsigned long long)dhist[i]);
    }
    if (threadIdx.x < nd) {
      const uint32_t j = threadIdx.x;
      const uint64_t s5 = ds5[j], n5 = dn5[j], offc = s_doff[j];
      const uint64_t a1 = s5 + n5 * offc, a0 = (sall - s5) + ((te - tb) - n5) * offc;
      unsigned long long *trow =
          (unsigned long long *)(k.table + (uint64_t)k.pos[s_dch[j]].row * ISIM_DES_ROW_WORDS);
      if (a0) atomicAdd(trow + 2 * ISIM_N_PROM, (unsigned long long)(0 - a0));
      if (a1) atomicAdd(trow + 2 * ISIM_N_PROM + 1, (unsigned long long)(0 - a1));
    }
    __syncthreads();  // red is reused below
  }
  des_flush_durations<kDesUpThreads>(k, P, hist, dsum0, dsum1, n500, red);
}

// ---- finalize: records and the latency statistics
template <typename T>
__global__ void __launch_bounds__(kDesUpThreads) des_finalize(DesK k) {
  __shared__ uint32_t hp[2 * ISIM_N_PROM], hl[2 * ISIM_N_LOG2];
  __shared__ uint64_t red[6 * kDesUpThreads / 64];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDesUpThreads) hp[i] = 0;
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_LOG2; i += kDesUpThreads) hl[i] = 0;
  des_bucket_lut_init(lut);
  __syncthreads();
  const uint64_t N = k.N;
  // an overflowed narrow batch is dropped (des_commit): records untouched
  const bool keep = *k.ovf == 0;
  const T *F0 = row<T>(k.WF, k.ld, 0);  // position 0: the entry
  uint64_t sl = 0, s5 = 0, se = 0, n5 = 0, mn = ~0ull, mx = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * kDesUpThreads + threadIdx.x; t < N;
       t += (uint64_t)gridDim.x * kDesUpThreads) {
    const uint64_t F = F0[t];
    const uint32_t st = (uint32_t)(F >> Row<T>::kTop);
    const uint64_t L = (F & Row<T>::kMask) - (k.A[t] - des_gbase(k, t));  // the latency
    const uint32_t e = k.E[t];
    if (k.records && keep) {
      isim_trace_rec r;
      r.latency_ns = L;
      r.hops = k.n_pos;
      r.status_err = (st << 31) | e;
      k.records[t] = r;
    }
    sl += L;
    s5 += st ? L : 0;
    se += e;
    n5 += st;
    mn = L < mn ? L : mn;
    mx = L > mx ? L : mx;
    atomicAdd(&hp[st * ISIM_N_PROM + des_prom_bucket(lut, L)], 1u);
    atomicAdd(&hl[st * ISIM_N_LOG2 + (L ? 64u - (uint32_t)__builtin_clzll(L) : 0u)], 1u);
  }
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) {
    sl += __shfl_xor(sl, d, 64);
    s5 += __shfl_xor(s5, d, 64);
    se += __shfl_xor(se, d, 64);
    n5 += __shfl_xor(n5, d, 64);
    const uint64_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  constexpr uint32_t W = kDesUpThreads / 64;
  if ((threadIdx.x & 63u) == 0) {
    const uint32_t w = threadIdx.x >> 6;
    red[w] = sl;
    red[W + w] = se;
    red[2 * W + w] = n5;
    red[3 * W + w] = mn;
    red[4 * W + w] = mx;
    red[5 * W + w] = s5;
  }
  __syncthreads();
  unsigned long long *st = (unsigned long long *)k.stats;
  // the entry's invocation durations (RecordResponseSent) are the latencies;
  // des_up leaves them here unless the entry finished in its queue pass
  const bool entry_dur = !(k.pos[0].flags & kDesFlagFused);
  unsigned long long *trow = (unsigned long long *)(k.table + (uint64_t)k.pos[0].row * ISIM_DES_ROW_WORDS);
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDesUpThreads)
    if (hp[i]) {
      atomicAdd(st + ISIM_ST_PROM + i, (unsigned long long)hp[i]);
      if (entry_dur) atomicAdd(trow + i, (unsigned long long)hp[i]);
    }
  for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_LOG2; i += kDesUpThreads)
    if (hl[i]) atomicAdd(st + ISIM_ST_LOG2 + i, (unsigned long long)hl[i]);
  if (threadIdx.x == 0) {
    for (uint32_t i = 1; i < W; ++i) {
      red[0] += red[i];
      red[W] += red[W + i];
      red[2 * W] += red[2 * W + i];
      red[3 * W] = red[3 * W + i] < red[3 * W] ? red[3 * W + i] : red[3 * W];
      red[4 * W] = red[4 * W + i] > red[4 * W] ? red[4 * W + i] : red[4 * W];
      red[5 * W] += red[5 * W + i];
    }
    if (entry_dur) {
      if (red[0] - red[5 * W]) atomicAdd(trow + 2 * ISIM_N_PROM, (unsigned long long)(red[0] - red[5 * W]));
      if (red[5 * W]) atomicAdd(trow + 2 * ISIM_N_PROM + 1, (unsigned long long)red[5 * W]);
    }
    if (blockIdx.x == 0) {
      atomicAdd(st + ISIM_ST_N_TRACES, (unsigned long long)N);
      atomicAdd(st + ISIM_ST_SUM_HOPS, (unsigned long long)(N * k.n_pos));
    }
    atomicAdd(st + ISIM_ST_SUM_LATENCY, (unsigned long long)red[0]);
    atomicAdd(st + ISIM_ST_SUM_ERR_HOPS, (unsigned long long)red[W]);
    atomicAdd(st + ISIM_ST_N_500, (unsigned long long)red[2 * W]);
    if (red[3 * W] != ~0ull) atomicMax(st + ISIM_ST_NOT_MIN_LATENCY, (unsigned long long)~red[3 * W]);
    atomicMax(st + ISIM_ST_MAX_LATENCY, (unsigned long long)red[4 * W]);
  }
}
