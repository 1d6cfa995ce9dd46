// The DES level engine's queue (down) pass, DESIGN.md §10.3: the finish of a
// thread's traces once its prefix is known, the 64-bit and 32-bit chunks of
// the closed-form single-replica queue, and the three launch shapes — one
// workgroup per position (des_down_mix; replicated services: des_down),
// chunks chained by a look-back (des_down_chain_mix) and consecutive rounds
// pipelined in one launch (des_down_pipe).
//
// Included by des.hip INSIDE namespace isim::dev, after des_rows.h,
// des_scan.h and the statistics helpers (as des_draw.h: a piece of that
// translation unit, not a header of its own).

constexpr uint32_t kN32 = kDesN32Per;  // consecutive traces per thread in the 32-bit-key queue chunks
// pipe_body's callers and callees hand chunks off by chunk INDEX (st_flag /
// the wait on a chunk), and the 32-bit and 64-bit branches step through
// chunks of kN32 and kPer traces per thread: the indices only name the same
// traces while both sizes agree.
static_assert(kN32 == kPer, "32-bit and 64-bit queue chunks must cover the same traces");
constexpr uint64_t kN32HoldMax = kDesN32HoldMax;  // (t - t_g) h < 2^31

// the keys a_t - t h of this thread's (up to) 4 traces from `base`
// (kKeyMin past N) and their largest
template <bool FULL>
__device__ __forceinline__ int64_t queue_keys(const uint64_t (&a)[kPer], uint64_t base, uint64_t N, uint64_t hold,
                                              int64_t (&key)[kPer]) {
  int64_t kt = kKeyMin;
  uint64_t th = base * hold;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    key[i] = FULL || base + i < N ? (int64_t)(a[i] - th) : kKeyMin;
    kt = max_i64(kt, key[i]);
    th += hold;
  }
  return kt;
}

// The queue of one chunk of 4 traces per thread, once the carry into the
// thread is known: S = max(x, a) per trace (absolute), the stored value
// (S or, fused, F | status, relative to A_t), waits and durations.
template <typename T, bool FUSED>
__device__ __forceinline__ void queue_finish(const DesK &k, const DesPos &P, uint64_t base, uint64_t N,
                                             uint64_t x, const uint64_t (&a)[kPer], const T (&r)[kPer],
                                             uint64_t off, uint32_t mask, uint32_t stm, T (&out)[kPer], uint32_t *hist,
                                             const uint8_t *lut,
                                             uint64_t &wsum, uint64_t &wmax, uint64_t &d0, uint64_t &d1,
                                             uint64_t &n5, bool &bad) {
  uint32_t bin[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin};
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    if (base + i < N && ((mask >> i) & 1u)) {
      const uint64_t S = x > a[i] ? x : a[i];
      const uint64_t w = S - a[i];
      wsum += w;
      wmax = w > wmax ? w : wmax;
      x = S + P.hold;
      uint64_t val = w + (uint64_t)r[i] + off;  // S - A_t (off is 0 for the entry: r = 0)
      if constexpr (FUSED) {
        const uint64_t F = val + P.floor;
        const uint32_t st = (stm >> i) & 1u;
        const uint64_t dur = w + P.floor;  // F - a
        if (st && !k.quiet) atomicAdd(k.E + base + i, 1u);
        n5 += st;
        d1 += st ? dur : 0;  // selects, not a branch: keeps d0/d1 in registers
        d0 += st ? 0 : dur;
        bin[i] = st * ISIM_N_PROM + des_prom_bucket(lut, dur);
        bad |= !Row<T>::fits(F);
        val = F | ((uint64_t)st << Row<T>::kTop);
      } else {
        bad |= !Row<T>::fits(val);
      }
      out[i] = (T)val;
    }
  }
  if constexpr (FUSED) hist_add4(hist, bin);
}

// agent-scope relaxed accesses: sc1 loads and stores (L1 bypassed)
__device__ __forceinline__ uint64_t ld_relaxed(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(uint64_t *p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_flag(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_flag(uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Single-replica queues (closed form): from the thread's exclusive prefix p
// the running max of the keys gives the wait of each trace, S_t - a_t =
// p_t - key_t; the stored value (S or, fused, F | status, relative to A_t),
// waits and durations as queue_finish.
struct QAcc {
  uint64_t wsum = 0, wmax = 0, dsum = 0, d1 = 0, n5 = 0;  // d0 = dsum - d1
  uint32_t wmax32 = 0;  // 32-bit rows: the largest wait (< 2^31 unless `bad`), folded into wmax by max_wait()
  bool bad = false;
  __device__ uint64_t max_wait() const { return wmax > wmax32 ? wmax : wmax32; }
};
template <typename T, bool FUSED, bool FULL>
__device__ __forceinline__ void queue_finish1(const DesK &k, const DesPos &P, uint64_t base, uint64_t N, int64_t p,
                                              const int64_t (&key)[kPer], const T (&r)[kPer], uint64_t off,
                                              uint32_t stm, T (&out)[kPer], uint32_t *hist, const uint8_t *lut,
                                              QAcc &q) {
  uint32_t bin[kPer] = {kNoBin, kNoBin, kNoBin, kNoBin};
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    if (FULL || base + i < N) {
      p = max_i64(p, key[i]);
      if constexpr (sizeof(T) == 4) {
        // 32-bit rows: a stored value below 2^31 needs a wait below 2^31, so
        // the wait, the duration and their maxima are 32-bit (a larger wait
        // marks the batch bad: it is rerun with 64-bit rows)
        const uint64_t w64 = (uint64_t)(p - key[i]);
        const uint32_t w = (uint32_t)w64;
        q.bad |= w64 >= Row<T>::kSt;
        q.wsum += w;
        q.wmax32 = w > q.wmax32 ? w : q.wmax32;
        uint64_t val = (uint64_t)w + (uint64_t)r[i] + off;  // S - A_t (off is 0 for the entry: r = 0)
        if constexpr (FUSED) {
          const uint64_t F = val + P.floor;
          const uint32_t st = (stm >> i) & 1u;
          const uint32_t dur = w + (uint32_t)P.floor;  // F - a; exact whenever F fits
          if (st && !k.quiet) atomicAdd(k.E + base + i, 1u);
          q.n5 += st;
          q.dsum += dur;
          q.d1 += st ? dur : 0u;
          bin[i] = st * ISIM_N_PROM + des_prom_bucket32(lut, dur);
          q.bad |= !Row<T>::fits(F);
          val = F | ((uint64_t)st << Row<T>::kTop);
        } else {
          q.bad |= !Row<T>::fits(val);
        }
        out[i] = (T)val;
        continue;
      }
      const uint64_t w = (uint64_t)(p - key[i]);
      q.wsum += w;
      q.wmax = w > q.wmax ? w : q.wmax;
      uint64_t val = w + (uint64_t)r[i] + off;  // S - A_t (off is 0 for the entry: r = 0)
      if constexpr (FUSED) {
        const uint64_t F = val + P.floor;
        const uint32_t st = (stm >> i) & 1u;
        const uint64_t dur = w + P.floor;  // F - a
        // (per trace: hoisting the atomics under one wave-uniform test was
        // measured no faster)
        if (st && !k.quiet) atomicAdd(k.E + base + i, 1u);
        q.n5 += st;
        q.dsum += dur;
        q.d1 += st ? dur : 0;  // a select, not a branch
        bin[i] = st * ISIM_N_PROM + des_prom_bucket(lut, dur);
        q.bad |= !Row<T>::fits(F);
        val = F | ((uint64_t)st << Row<T>::kTop);
      } else {
        q.bad |= !Row<T>::fits(val);
      }
      out[i] = (T)val;
    }
  }
  if constexpr (FUSED) hist_add4<FULL>(hist, bin);
}

// this thread's 4 traces (one group: base % 4 == 0): absolute arrivals a =
// G + relative arrival, and the relative arrivals' row values r (S relative
// = wait + r + off); the entry's relative arrival is A_t - G.  Returns true
// when an entry value does not fit the row type (the batch is redone wide).
template <typename T, bool FULL = false>
__device__ __forceinline__ bool load_arrivals(const DesK &k, const T *par, uint64_t off, uint64_t base,
                                              uint64_t N, uint64_t (&a)[kPer], T (&r)[kPer]) {
  constexpr Quad Q = FULL ? Quad::whole : Quad::test;
  const uint64_t g = FULL || base < N ? des_gbase(k, base) : 0;
  if (par) {
    load_row<T, Q>(par, base, N, r);
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) a[i] = g + (uint64_t)r[i] + off;
    return false;
  }
  load_row<uint64_t, Q>(k.A, base, N, a);
  bool bad = false;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    const uint64_t d = FULL || base + i < N ? a[i] - g : 0;
    r[i] = (T)d;
    bad |= !Row<T>::fits(d);
  }
  return bad;
}

// ---- queue pass, one workgroup per position (wide groups; replicated
// services: per-replica scans, the routing draw per trace)
// single-replica services: the closed form, one barrier per chunk (the wave
// totals double-buffered; every thread folds them into its prefix and into the
// carry itself)
// One chunk of kPer x kDownThreads traces from c0 (FULL: all below N).
// Pipelined pass (des_down_pipe): HAND_IN, the caller's start row is written
// in this launch, read with sc1 loads; HAND_OUT, this start row is read in
// this launch: sc1 stores, and at the chunk's barrier (every wave drained its
// previous chunk's stores first) one lane publishes the chunks done so far.
template <typename T, bool FUSED, bool FULL, bool HAND_IN = false, bool HAND_OUT = false>
__device__ __forceinline__ void down1_chunk(const DesK &k, const DesPos &P, uint32_t v, const T *par, uint64_t off,
                                            T *out, uint64_t c0, int64_t *wtot, int64_t &carry, uint32_t *hist,
                                            const uint8_t *lut, QAcc &q, uint32_t chunk = 0) {
  constexpr uint32_t NW = kDownThreads / 64;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t N = k.N;
  uint64_t base = c0 + (uint64_t)threadIdx.x * kPer;
  // opaque to loop strength reduction, which otherwise keeps a dozen 64-bit
  // induction variables ((base + i) * hold, ...) live across the chunk loop
  __asm__ volatile("" : "+v"(base));
  uint64_t a[kPer];
  T ar[kPer];
  if constexpr (HAND_IN) {
    const uint64_t g = FULL || base < N ? des_gbase(k, base) : 0;
    load_row<T, FULL ? Quad::whole : Quad::each, Mem::sc1>(par, base, N, ar, c0);
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) a[i] = g + (uint64_t)ar[i] + off;
  } else {
    q.bad |= load_arrivals<T, FULL>(k, par, off, base, N, a, ar);
  }
  const uint32_t stm = FUSED ? des_status4(k, v, base) : 0u;
  int64_t key[kPer];
  const int64_t inc = wave_max_scan(queue_keys<FULL>(a, base, N, P.hold, key));
  const int64_t exc = wave_shr1(inc);
  if (lane == 63) wtot[wave] = inc;
  if constexpr (HAND_OUT) __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the previous chunk's stores
  __syncthreads();
  if constexpr (HAND_OUT)
    if (threadIdx.x == 0 && chunk > 0) st_flag(k.prog + v, chunk);
  // lanes 0..NW-1 scan the wave totals: the waves before this one and all
  int64_t pre;
  fold_totals<NW>(wtot, wave, carry, pre);
  T o[kPer] = {0, 0, 0, 0};
  queue_finish1<T, FUSED, FULL>(k, P, base, N, max_i64(pre, exc), key, ar, off, stm, o, hist, lut, q);
  if constexpr (FUSED) track4<T>(k, out, base, N, o);  // a fused leaf's row is final (F)
  if constexpr (HAND_OUT) store_row<T, FULL ? Quad::whole : Quad::each, Mem::sc1>(out, base, N, o, c0);
  else store_row<T, FULL ? Quad::whole : Quad::test, kRowStore<T>>(out, base, N, o);
}

// ---- 32-bit queue keys (round 3; narrow rows, whole chunks, every position
// but the entry).  A wave's 256 traces are 4 groups of 64, one DPP row (16
// lanes x 4 traces) each.  With x_t = row + off the group-relative arrival
// and the group's base kb = G - t_g h (G its first arrival, t_g its first
// trace), the keys relative to kb,
//   key_t - kb = x_t - (t - t_g) h,
// lie in (-64 h, x_t]: 32-bit whenever x_t < 2^31 (a larger one overflows
// the start row anyway: the batch is redone wide) and 64 h < 2^31 (the
// caller's check).  A row scan by DPP gives each trace its prefix within the
// group; the group totals (64-bit absolute) combine across the wave's rows
// by two row broadcasts, across the waves through LDS (fold_totals) and
// across chunks in the carry.  A prefix below every key is clamped to
// INT32_MIN (exact: keys exceed -2^31); one at or above 2^31 puts the
// group's first start at or above 2^31 (a row overflow: the batch is redone).
//
// the finish of one thread's kN32 traces with 32-bit keys from the prefix p
// (FULL: all below N; else the traces past N are left out)
template <bool FUSED, bool FULL>
__device__ __forceinline__ void queue_finish_n32(const DesK &k, uint64_t base, int32_t p, const int32_t (&key)[kN32],
                                                 const uint32_t (&x)[kN32], uint32_t floor32, uint32_t stm,
                                                 uint32_t (&out)[kN32], uint32_t *hist, const uint8_t *lut, QAcc &q) {
  static_assert(kN32 % 2 == 0, "waits are summed in pairs");
  uint32_t bin[kN32], wv[kN32], big = 0, cnt = 0;
#pragma unroll
  for (uint32_t i = 0; i < kN32; ++i) {
    out[i] = 0;
    bin[i] = kNoBin;
    wv[i] = 0;
    if (!FULL && base + i >= k.N) continue;
    if constexpr (!FULL) ++cnt;
    p = max_i32(p, key[i]);
    const uint32_t w = (uint32_t)p - (uint32_t)key[i];  // the wait S - a (< 2^32: exact)
    wv[i] = w;
    q.wmax32 = w > q.wmax32 ? w : q.wmax32;
    uint32_t val = w + x[i];  // S - G (no wrap unless the batch is redone)
    big |= w | val;           // a wait or start at or above 2^31: redone with 64-bit rows
    if constexpr (FUSED) {
      const uint32_t F = val + floor32;
      const uint32_t st = (stm >> i) & 1u;
      const uint32_t dur = w + floor32;  // F - a
      bin[i] = st * ISIM_N_PROM + des_prom_bucket32(lut, dur);
      big |= F;
      val = F | (st << 31);
    }
    out[i] = val;
  }
  // the sums once per call: a pair of waits fits 32 bits (each is below 2^31,
  // or `big` redoes the batch with 64-bit rows and these statistics are not
  // committed); the durations' sum is the waits' plus n x floor; the 500s
  // (rare: stm is almost always 0 wave-wide) under one branch
  uint64_t ws = 0;
#pragma unroll
  for (uint32_t h = 0; h < kN32; h += 2) ws += (uint64_t)(wv[h] + wv[h + 1]);
  q.wsum += ws;
  if constexpr (FUSED) {
    q.dsum += ws + (uint64_t)(FULL ? kN32 : cnt) * floor32;
    if (stm) {
#pragma unroll
      for (uint32_t i = 0; i < kN32; ++i)
        if ((stm >> i) & 1u) {
          if (!k.quiet) atomicAdd(k.E + base + i, 1u);
          q.n5 += 1;
          q.d1 += wv[i] + floor32;
        }
    }
  }
  q.bad |= (big >> 31) != 0u;
  if constexpr (FUSED) hist_add4<FULL>(hist, bin);
}

// down1_chunk for narrow rows (FULL: a whole chunk; ENTRY: the entry, whose
// group-relative arrival is A_t - G; else the caller's row `par`), kN32
// consecutive traces per thread: a DPP row (16 lanes) holds one trace group;
// `jh0` = (t - t_g) h of the thread's first trace (the caller's per-position
// constant).  The same results as down1_chunk<uint32_t, FUSED, FULL, ...>.
template <bool FUSED, bool HAND_IN, bool HAND_OUT, bool FULL = true, bool ENTRY = false>
__device__ __forceinline__ void down1_chunk_n32(const DesK &k, const DesPos &P, uint32_t v, const uint32_t *par,
                                                uint32_t *out, uint64_t c0, int64_t *wtot, int64_t &carry,
                                                uint32_t *hist, const uint8_t *lut, QAcc &q, uint32_t chunk,
                                                uint32_t jh0) {
  constexpr uint32_t NW = kDownThreads / 64;
  constexpr Quad Q = FULL ? Quad::whole : Quad::each;  // a chunk's tail goes value by value
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t N = k.N;
  uint64_t base = c0 + (uint64_t)threadIdx.x * kN32;
  __asm__ volatile("" : "+v"(base));  // (down1_chunk)
  const uint64_t tg = base & ~(kDesGrp - 1);
  const uint64_t g = FULL || tg < N ? k.A[tg] : 0;  // every lane of a group with a trace below N
  uint32_t x[kN32], xo = 0;
  if constexpr (ENTRY) {
    uint64_t d = 0;
#pragma unroll
    for (uint32_t i = 0; i < kN32; ++i) {
      const uint64_t r = FULL || base + i < N ? k.A[base + i] - g : 0;
      d |= r;
      x[i] = (uint32_t)r;
    }
    q.bad |= (d >> 31) != 0;
  } else {
    uint32_t ar[kN32];
    load_row<uint32_t, Q, HAND_IN ? Mem::sc1 : Mem::plain>(par, base, N, ar, c0);
    const uint32_t off32 = (uint32_t)P.off;
#pragma unroll
    for (uint32_t i = 0; i < kN32; ++i) x[i] = ar[i] + off32;
  }
  // own error statuses, bit i (base % kN32 == 0: one status word, nothing past N)
  const uint32_t stm = FUSED && base < N ? (k.stbits[(uint64_t)v * k.st_wpr + (base >> 5)] >> (base & 31u)) &
                                               ((1u << kN32) - 1u)
                                         : 0u;
  const uint32_t hold32 = (uint32_t)P.hold;
  int32_t key[kN32], kt = INT32_MIN;
#pragma unroll
  for (uint32_t i = 0; i < kN32; ++i) {
    xo |= x[i];
    key[i] = FULL || base + i < N ? (int32_t)(x[i] - (jh0 + i * hold32)) : INT32_MIN;
    kt = max_i32(kt, key[i]);
  }
  q.bad |= (xo >> 31) != 0u;  // an arrival at or above 2^31: its start row overflows
  const int32_t inc = row_max_scan32(kt);
  const int32_t exc = __builtin_amdgcn_update_dpp((int)INT32_MIN, inc, 0x111, 0xF, 0xF, false);  // row_shr:1
  // the group totals, absolute, at lane 15 of each row; their inclusive prefix
  // over the wave's rows at lanes 15/31/47/63, and each row's exclusive one
  // (a group past N: kb = -t_g h, its total INT32_MIN relative — below any key)
  const int64_t kb = (int64_t)(g - tg * P.hold);
  int64_t s = kb + (int64_t)inc;
  s = max_i64(s, dpp_i64<0x142, 0xA>(s, s));  // row_bcast:15 into rows 1, 3
  s = max_i64(s, dpp_i64<0x143, 0xC>(s, s));  // row_bcast:31 into rows 2, 3
  int64_t e = dpp_i64<0x142, 0xA>(kKeyMin, s);  // rows 1, 3: lane 15 / 47
  e = dpp_i64<0x143, 0x4>(e, s);                // row 2: lane 31
  if (lane == 63) wtot[wave] = max_i64(0, s);
  if constexpr (HAND_OUT) __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the previous chunk's stores
  __syncthreads();
  if constexpr (HAND_OUT)
    if (threadIdx.x == 0 && chunk > 0) st_flag(k.prog + v, chunk);
  int64_t pre;
  fold_totals<NW>(wtot, wave, carry, pre);
  const int64_t pr = max_i64(pre, e) - kb;  // the group's prefix, relative
  q.bad |= (FULL || base < N) && pr > (int64_t)INT32_MAX;
  const int32_t p0 = pr < (int64_t)INT32_MIN ? INT32_MIN : pr > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)pr;
  uint32_t o[kN32];
  queue_finish_n32<FUSED, FULL>(k, base, max_i32(p0, exc), key, x, (uint32_t)P.floor, stm, o, hist, lut, q);
  if constexpr (FUSED) track4<uint32_t>(k, out, base, N, o);  // a fused leaf's row is final (F)
  store_row<uint32_t, Q, HAND_OUT ? Mem::sc1 : Mem::nontemporal>(out, base, N, o, c0);
}

// whether a position's whole chunks take the 32-bit keys, and the thread's (t - t_g) h
template <typename T, bool FUSED>
__device__ __forceinline__ bool n32_ok(const DesPos &P, const void *par, uint32_t &jh0) {
  jh0 = (threadIdx.x & 15u) * kN32 * (uint32_t)P.hold;
  return sizeof(T) == 4 && par != nullptr && P.hold < kN32HoldMax && P.off < (1ull << 30) &&
         (!FUSED || P.floor < (1ull << 30));
}

template <typename T, bool FUSED>
__device__ __forceinline__ void down1_body(const DesK &k, uint32_t v) {
  constexpr uint32_t NW = kDownThreads / 64;
  __shared__ int64_t wtot[2][NW];
  __shared__ uint64_t red[3 * NW];
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  const DesPos P = k.pos[v];
  if constexpr (FUSED) {
    for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDownThreads) hist[i] = 0;
    des_bucket_lut_init(lut);
    __syncthreads();
  }
  const uint64_t N = k.N;
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  T *out = row<T>(FUSED ? k.WF : k.W, k.ld, v);  // a fused leaf stores its finish
  QAcc q;
  int64_t carry = 0;  // max key of the chunks before (0: the idle start)
  uint32_t buf = 0;
  constexpr uint64_t CH = (uint64_t)kPer * kDownThreads;
  uint64_t c0 = 0;
  uint32_t jh0;
  if (n32_ok<T, FUSED>(P, par, jh0)) {
    if constexpr (sizeof(T) == 4) {
      constexpr uint64_t CH32 = (uint64_t)kN32 * kDownThreads;
#pragma unroll 1
      for (; c0 + CH32 <= N; c0 += CH32) {
        down1_chunk_n32<FUSED, false, false>(k, P, v, par, out, c0, wtot[buf], carry, hist, lut, q, 0, jh0);
        buf ^= 1u;
      }
    }
  }
#pragma unroll 1
  for (; c0 + CH <= N; c0 += CH) {
    down1_chunk<T, FUSED, true>(k, P, v, par, off, out, c0, wtot[buf], carry, hist, lut, q);
    buf ^= 1u;
  }
  if (c0 < N) down1_chunk<T, FUSED, false>(k, P, v, par, off, out, c0, wtot[buf], carry, hist, lut, q);
  flag_overflow(k, q.bad);
  if (k.quiet) return;
  des_flush_waits<kDownThreads>(k, P.row, q.wsum, q.max_wait(), N, N * P.hold, red);
  if constexpr (FUSED) {
    __syncthreads();
    des_flush_durations<kDownThreads>(k, P, hist, q.dsum - q.d1, q.d1, q.n5, red);
  }
}

// replicated services: per-replica max-plus scans, the routing draw per trace
template <typename T, bool FUSED>
__device__ __forceinline__ void downr_body(const DesK &k, uint32_t v) {
  __shared__ MaxPlus wtot[kDownThreads / 64];
  __shared__ uint64_t carry[kDesMaxReplicas];
  __shared__ uint64_t red[3 * kDownThreads / 64];
  __shared__ MaxPlus xs[kDownThreads];
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  const DesPos P = k.pos[v];
  const uint32_t reps = P.reps;
  if (threadIdx.x < reps) carry[threadIdx.x] = 0;
  if constexpr (FUSED) {
    for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDownThreads) hist[i] = 0;
    des_bucket_lut_init(lut);
  }
  __syncthreads();
  const uint64_t N = k.N;
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  T *out = row<T>(FUSED ? k.WF : k.W, k.ld, v);  // a fused leaf stores its finish
  uint64_t wsum = 0, wmax = 0, d0 = 0, d1 = 0, n5 = 0;
  bool bad = false;
  for (uint64_t c0 = 0; c0 < N; c0 += (uint64_t)kPer * kDownThreads) {
    const uint64_t base = c0 + (uint64_t)threadIdx.x * kPer;
    uint64_t a[kPer];
    T o[kPer] = {0, 0, 0, 0};
    T ar[kPer];
    bad |= load_arrivals<T>(k, par, off, base, N, a, ar);
    uint32_t rr[kPer];
    const uint32_t stm = FUSED ? des_status4(k, v, base) : 0u;  // fused leaves: own error statuses, bit i
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i)
      rr[i] = base + i < N ? des_draw(k.trace_begin + base + i, v, 0x80000002u, 0, k.k0, k.k1) % reps : 0u;
    for (uint32_t r = 0; r < reps; ++r) {
      MaxPlus f{0, 0};
      uint32_t mask = 0;
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i)
        if (base + i < N && rr[i] == r) {
          f = mp_then(f, MaxPlus{P.hold, a[i] + P.hold});
          mask |= 1u << i;
        }
      const MaxPlus inc = mp_block_scan<kDownThreads>(f, wtot);
      // exclusive prefix = the previous thread's inclusive one
      xs[threadIdx.x] = inc;
      __syncthreads();
      const MaxPlus pre = threadIdx.x ? xs[threadIdx.x - 1] : MaxPlus{0, 0};
      const uint64_t cin = carry[r];
      const uint64_t x = cin + pre.B > pre.C ? cin + pre.B : pre.C;
      queue_finish<T, FUSED>(k, P, base, N, x, a, ar, off, mask, stm, o, hist, lut, wsum, wmax, d0, d1, n5, bad);
      __syncthreads();  // every thread has read carry[r]
      if (threadIdx.x == kDownThreads - 1) {
        uint64_t xe = x;
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i)
          if ((mask >> i) & 1u) xe = (xe > a[i] ? xe : a[i]) + P.hold;
        carry[r] = xe;
      }
      __syncthreads();
    }
    if constexpr (FUSED) track4<T>(k, out, base, N, o);  // a fused leaf's row is final (F)
    store_row<T, Quad::test, kRowStore<T>>(out, base, N, o);
  }
  flag_overflow(k, bad);
  if (k.quiet) return;
  des_flush_waits<kDownThreads>(k, P.row, wsum, wmax, N, N * P.hold, red);
  if constexpr (FUSED) {
    __syncthreads();
    des_flush_durations<kDownThreads>(k, P, hist, d0, d1, n5, red);
  }
}

// replicated positions of a round: the fused leaves in one launch, the others in another
template <typename T, bool FUSED>
__global__ void __launch_bounds__(kDownThreads, ISIM_DES_DOWN_WAVES) des_down(DesK k) {
  downr_body<T, FUSED>(k, k.level_pos[k.level_begin + blockIdx.x]);
}

// single-replica positions of a round, fused leaves and others in ONE launch
// (better packing of the last wave of workgroups than two launches)
template <typename T>
__global__ void __launch_bounds__(kDownThreads, ISIM_DES_DOWN_WAVES) des_down_mix(DesK k) {
  const uint32_t v = k.level_pos[k.level_begin + blockIdx.x];
  if (k.pos[v].flags & kDesFlagFused) down1_body<T, true>(k, v);
  else down1_body<T, false>(k, v);
}

// ---- queue pass, single-replica services of narrow groups: one workgroup
// per (position, chunk of kDownChunk traces), chunks of a position chained by
// a decoupled look-back over their max-plus maps.  Workgroups take tickets in
// launch order (position-major, chunk-minor), so every chunk they wait on
// has started.
// (ChainState, one per (position, chunk): des_layout.h)

// the ticket of a chained-scan workgroup: (position, chunk) in launch order
__device__ __forceinline__ uint32_t chain_ticket(const DesK &k) {
  __shared__ uint32_t s_ticket;
  if (threadIdx.x == 0) s_ticket = atomicAdd(k.chain_ticket, 1u);
  __syncthreads();
  return s_ticket;
}

template <typename T, bool FUSED>
__device__ __forceinline__ void chain_body(const DesK &k, uint32_t v, uint32_t chunk) {
  constexpr uint32_t NW = kDesThreads / 64;
  __shared__ int64_t wtot[NW];
  __shared__ uint64_t red[3 * kDesThreads / 64];
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  __shared__ int64_t s_carry;
  if constexpr (FUSED) {
    for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDesThreads) hist[i] = 0;
    des_bucket_lut_init(lut);
  }
  const DesPos P = k.pos[v];
  const uint64_t N = k.N;
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  T *out = row<T>(FUSED ? k.WF : k.W, k.ld, v);  // a fused leaf stores its finish
  ChainState *cs = k.chain + (uint64_t)v * k.n_chunks;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)chunk * kDownChunk + (uint64_t)threadIdx.x * kPer;
  uint64_t a[kPer];
  T ar[kPer];
  const bool in_bad = load_arrivals<T>(k, par, off, base, N, a, ar);
  const uint32_t stm = FUSED && base < N ? des_status4(k, v, base) : 0u;
  int64_t key[kPer];
  const int64_t inc = wave_max_scan(queue_keys<false>(a, base, N, P.hold, key));
  const int64_t exc = wave_shr1(inc);
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  if (threadIdx.x < 64) {
    // wave 0: publish this chunk's largest key, then look back (64 chunks
    // per step) for the largest key before it.  Hand-offs between workgroups
    // (other XCDs included) use sc1 stores drained before the flag store and
    // sc1 loads (no L2 writeback / invalidate).
    int64_t agg = kKeyMin, unused;
    fold_totals<NW>(wtot, 0, agg, unused);
    if (chunk > 0 && lane == 0) {
      st_relaxed(&cs[chunk].B, (uint64_t)agg);
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st_flag(&cs[chunk].flag, 1u);
    }
    int64_t cin = 0;  // chunk 0 starts from an idle worker
    if (chunk > 0) {
      int64_t run = kKeyMin;  // the windows already passed
      int64_t top = (int64_t)chunk - 1;
      uint32_t spins = 0;
      for (;;) {
        if (spins >= k.spin_limit) {  // never expected (tickets order the chunks): fail the batch
          if (lane == 0) atomicOr(k.ovf, kDesOvfFault);
          break;
        }
        const int64_t j = top - (int64_t)lane;  // lane 0 = the nearest chunk
        const uint32_t fl = j >= 0 ? ld_flag(&cs[j].flag) : 2u;  // j < 0: the idle start, prefix 0
        const uint64_t m0 = __ballot(fl == 0), m2 = __ballot(fl == 2);
        const uint32_t f2 = m2 ? (uint32_t)__builtin_ctzll(m2) : 64u;
        const uint64_t below = f2 >= 64 ? ~0ull : ((1ull << f2) - 1);
        if (m0 & below) {  // a chunk this one needs has not published yet
          __builtin_amdgcn_s_sleep(1);
          ++spins;
          continue;
        }
        // chunks nearer than the first inclusive prefix give their own key,
        // that chunk its prefix (the order does not matter for a max)
        int64_t m = kKeyMin;
        if (lane < f2 && j >= 0) m = (int64_t)ld_relaxed(&cs[j].B);
        if (lane == f2) m = j >= 0 ? (int64_t)ld_relaxed(&cs[j].P) : 0;
        run = max_i64(run, read_lane(wave_max_scan(m), 63));
        if (f2 < 64) {
          cin = run;
          break;
        }
        top -= 64;
      }
    }
    if (lane == 0) {
      st_relaxed(&cs[chunk].P, (uint64_t)max_i64(cin, agg));
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
      st_flag(&cs[chunk].flag, 2u);
      s_carry = cin;
    }
  }
  __syncthreads();
  int64_t cin = s_carry, pre;
  fold_totals<NW>(wtot, wave, cin, pre);
  T o[kPer] = {0, 0, 0, 0};
  QAcc q;
  q.bad = in_bad;
  queue_finish1<T, FUSED, false>(k, P, base, N, max_i64(pre, exc), key, ar, off, stm, o, hist, lut, q);
  if constexpr (FUSED) track4<T>(k, out, base, N, o);  // a fused leaf's row is final (F)
  store_row<T, Quad::test, kRowStore<T>>(out, base, N, o);
  flag_overflow(k, q.bad);
  if (k.quiet) return;
  des_flush_waits<kDesThreads>(k, P.row, q.wsum, q.max_wait(), chunk == 0 ? N : 0, chunk == 0 ? N * P.hold : 0, red);
  if constexpr (FUSED) {
    __syncthreads();
    des_flush_durations<kDesThreads>(k, P, hist, q.dsum - q.d1, q.d1, q.n5, red);
  }
}

// fused leaves and other positions in one launch (as des_down_mix)
template <typename T>
__global__ void __launch_bounds__(kDesThreads, 8) des_down_chain_mix(DesK k) {
  const uint32_t ticket = chain_ticket(k);
  const uint32_t v = k.level_pos[k.level_begin + ticket / k.n_chunks];
  if (k.pos[v].flags & kDesFlagFused) chain_body<T, true>(k, v, ticket % k.n_chunks);
  else chain_body<T, false>(k, v, ticket % k.n_chunks);
}

// ---- pipelined queue pass: the single-replica positions of
// consecutive rounds in ONE launch, one workgroup per position, tickets in the
// plan's round order.  A position whose arrivals are its caller's start row
// waits chunk by chunk for the caller to publish them (the caller's ticket is
// earlier, so it is resident and progressing): no level boundaries, no tail
// of one level in front of the next.
// N32: every chunk takes the 32-bit keys (narrow rows; the host checked the
// segment's holds and offsets, DesPlan::pipe_n32): the launch holds no 64-bit
// key code, so it runs at more waves per SIMD
template <typename T, bool FUSED, bool HAND_IN, bool N32 = false>
__device__ __forceinline__ void pipe_body(const DesK &k, uint32_t v, uint32_t dep) {
  constexpr uint32_t NW = kDownThreads / 64;
  constexpr bool HAND_OUT = !FUSED;  // non-leaves: their callees may read the start row in this launch
  __shared__ int64_t wtot[2][NW];
  __shared__ uint64_t red[3 * NW];
  __shared__ uint32_t hist[2 * ISIM_N_PROM];
  __shared__ __attribute__((aligned(4))) uint8_t lut[4 * kBucketLutWords];
  __shared__ uint32_t s_known;
  const DesPos P = k.pos[v];
  if constexpr (FUSED) {
    for (uint32_t i = threadIdx.x; i < 2 * ISIM_N_PROM; i += kDownThreads) hist[i] = 0;
    des_bucket_lut_init(lut);
    __syncthreads();
  }
  const uint64_t N = k.N;
  const T *par = arrival_row<T>(k, v, P);
  const uint64_t off = par ? P.off : 0;
  T *out = row<T>(FUSED ? k.WF : k.W, k.ld, v);  // a fused leaf stores its finish
  QAcc q;
  int64_t carry = 0;
  uint32_t buf = 0, known = 0, chunk = 0;
  // the caller's chunks [0, chunk] published (one lane polls, the barrier
  // shares the count; bounded: a timeout drops the batch, never expected)
  auto wait = [&]() {
    if constexpr (HAND_IN) {
      if (known <= chunk) {
        if (threadIdx.x == 0) {
          uint32_t pv, spins = 0;
          while ((pv = ld_flag(k.prog + dep)) <= chunk) {
            if (spins++ >= k.spin_limit) {  // never expected: fail the batch
              atomicOr(k.ovf, kDesOvfFault);
              pv = 0xFFFFFFFFu;
              break;
            }
            __builtin_amdgcn_s_sleep(2);
          }
          s_known = pv;
        }
        __syncthreads();
        known = s_known;
      }
    }
  };
  constexpr uint64_t CH = (uint64_t)kPer * kDownThreads;
  uint64_t c0 = 0;
  if constexpr (N32 && sizeof(T) == 4) {
    const uint32_t jh0 = (threadIdx.x & 15u) * kN32 * (uint32_t)P.hold;
    constexpr uint64_t CH32 = (uint64_t)kN32 * kDownThreads;
    auto chunks = [&](auto entry_t) {
      constexpr bool ENTRY = decltype(entry_t)::value;
#pragma unroll 1
      for (; c0 + CH32 <= N; c0 += CH32, ++chunk) {
        wait();
        down1_chunk_n32<FUSED, HAND_IN, HAND_OUT, true, ENTRY>(k, P, v, par, out, c0, wtot[buf], carry, hist, lut, q,
                                                               chunk, jh0);
        buf ^= 1u;
      }
      if (c0 < N) {
        wait();
        down1_chunk_n32<FUSED, HAND_IN, HAND_OUT, false, ENTRY>(k, P, v, par, out, c0, wtot[buf], carry, hist, lut, q,
                                                                chunk, jh0);
        ++chunk;
      }
    };
    if (par) chunks(std::false_type{});
    else chunks(std::true_type{});
  } else {
    // (no 32-bit chunks here: a caller and its callees must count chunks of
    // one size, and this launch has positions the 32-bit keys do not fit)
#pragma unroll 1
    for (; c0 + CH <= N; c0 += CH, ++chunk) {
      wait();
      down1_chunk<T, FUSED, true, HAND_IN, HAND_OUT>(k, P, v, par, off, out, c0, wtot[buf], carry, hist, lut, q, chunk);
      buf ^= 1u;
    }
    if (c0 < N) {
      wait();
      down1_chunk<T, FUSED, false, HAND_IN, HAND_OUT>(k, P, v, par, off, out, c0, wtot[buf], carry, hist, lut, q, chunk);
      ++chunk;
    }
  }
  if constexpr (HAND_OUT) {
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's last stores
    __syncthreads();
    if (threadIdx.x == 0) st_flag(k.prog + v, chunk);
  }
  flag_overflow(k, q.bad);
  if (k.quiet) return;
  des_flush_waits<kDownThreads>(k, P.row, q.wsum, q.max_wait(), N, N * P.hold, red);
  if constexpr (FUSED) {
    __syncthreads();
    des_flush_durations<kDownThreads>(k, P, hist, q.dsum - q.d1, q.d1, q.n5, red);
  }
}

template <typename T, bool N32>
__global__ void __launch_bounds__(kDownThreads, N32 ? ISIM_DES_PIPE32_WAVES : ISIM_DES_DOWN_WAVES)
    des_down_pipe(DesK k) {
  const uint32_t t = chain_ticket(k);
  const uint32_t v = k.level_pos[k.level_begin + t], dep = k.pipe_dep[k.level_begin + t];
  if (k.pos[v].flags & kDesFlagFused) {
    if (dep != kDesNone) pipe_body<T, true, true, N32>(k, v, dep);
    else pipe_body<T, true, false, N32>(k, v, dep);
  } else {
    if (dep != kDesNone) pipe_body<T, false, true, N32>(k, v, dep);
    else pipe_body<T, false, false, N32>(k, v, dep);
  }
}
