// DES item engine, stage 4b: the queues of a round —
// arrivals, the FIFO order (sort keys, ties, kept orders), the order's
// sources and the one kernel that writes it out as arrays (k_pairs), the
// queue-figure fold (QFold), and the two scans' kernels (k_qout after
// rocPRIM's scan by key; k_qscan, one pass).  Worker pools (des_workers.h)
// follow at the end.  A part of des_items.hip, included inside namespace
// isim::dit after des_items_k.h.
#pragma once

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

// Where a round's queue order comes from.  k_qscan reads it at its source;
// the scan by key and a pooled round's refinement read it as arrays, which
// k_pairs materialises (kQArrays: the two-sort path writes them itself):
//   kQArrays  the arrays (segment key, row, item, (hold, a + hold)): k_pairs',
//             k_pairs2's or a pooled round's refined ones (des_workers.h)
//   kQList    a round that needs no sort (DesPlan::round_nosort): its list in
//             (position, trace) order is each position's FIFO already;
//             segment = the position (a zero-hold item alone: qalone)
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

// A zero-hold position of a sort-free round (its arrivals need not come in
// trace order) starts each item at its own arrival (des_oracle.c: an
// invocation holding its worker for 0 starts when it arrives): every such
// item is a segment of its own, whatever its neighbours' keys
template <int SRC>
__device__ __forceinline__ bool qalone(uint64_t hold) {
  return SRC == kQList && hold == 0;
}

// item j of the order: its segment key (hold-free: qalone is the caller's),
// and with FULL its item, row, hold and arrival.  kQList computes the arrival
// as k_qarr would (k_qscan on the list: no k_qarr launched), or with STORED
// reads the one k_qarr left in IA
template <int SRC, bool FULL, bool STORED = false>
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
      if (SRC == kQKept || STORED || !live(k, i)) {
        a = k.IA[i];  // (kQList: an item a quiet pass does not recompute keeps its own)
      } else {
        a = item_arrival(k, i, v, P.off);
        k.IA[i] = a;
      }
    }
  }
  return sk;
}

// The order as arrays, for the scan by key and des_workers.h: the segment key
// (the position, or row | replica), row, map (hold, a + hold) and item of
// each place of the order; k_qarr has run, so a list's arrivals are the
// stored ones.  An item alone takes a key above any position that alternates
// by index, so it differs from both neighbours' (they compare adjacent keys)
template <int SRC>
__global__ void __launch_bounds__(kT) k_pairs(K k, uint64_t m, QSrc q, uint32_t *segk, uint32_t *rowk, MP *mp,
                                              uint32_t *sid) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    uint32_t i, row;
    uint64_t hold, a;
    const uint64_t sk = qitem<SRC, true, true>(k, q, j, i, row, hold, a);
    segk[j] = qalone<SRC>(hold) ? 0x80000000u | (uint32_t)(j & 1u) : (uint32_t)sk;
    rowk[j] = row;
    mp[j] = MP{hold, a + hold};
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

// The queue figures of a recording pass, per table row: invocations, summed
// and longest wait, summed hold — four consecutive words of the row.  A lane
// sums its run of one row before any atomic; a workgroup's items are mostly
// one row (its first item's: the head row), whose figures the lanes sum in
// LDS, laid out as the table's, and thread 0 sends on: one global atomic per
// figure and workgroup, not per lane run.  k_qout and k_qscan both fold so
static_assert(ISIM_DES_SUM_WAIT == ISIM_DES_COUNT + 1 && ISIM_DES_MAX_WAIT == ISIM_DES_COUNT + 2 &&
                  ISIM_DES_SUM_HOLD == ISIM_DES_COUNT + 3,
              "the queue figures are four consecutive words");
__device__ __forceinline__ void qfig_add(unsigned long long *w, unsigned long long n, unsigned long long sw,
                                         unsigned long long mw, unsigned long long sh) {
  atomicAdd(w, n);
  if (sw) atomicAdd(w + 1, sw);
  if (mw) atomicMax(w + 2, mw);
  if (sh) atomicAdd(w + 3, sh);
}
struct QHead {  // __shared__ in the kernel
  unsigned long long w[4];
  uint32_t row;
};
struct QFold {
  QHead *hd;
  unsigned long long *table;
  uint32_t hrow, row = kNone;  // the head row; the lane's run
  unsigned long long n = 0, sw = 0, mw = 0, sh = 0;

  // one thread empties the head row; a barrier, then every thread's QFold
  static __device__ __forceinline__ void open(QHead *hd, uint32_t row) {
    hd->w[0] = hd->w[1] = hd->w[2] = hd->w[3] = 0;
    hd->row = row;
  }
  // (a quiet pass records nothing: it opens no head row and adds no item)
  __device__ __forceinline__ QFold(const K &k, QHead *hd_)
      : hd(hd_), table(k.table), hrow(k.quiet ? kNone : hd_->row) {}
  __device__ __forceinline__ unsigned long long *words(uint32_t r) const {
    return table + (uint64_t)r * ISIM_DES_ROW_WORDS + ISIM_DES_COUNT;
  }
  __device__ __forceinline__ void flush() {
    if (row == kNone || !n) return;
    if (row == hrow) qfig_add(hd->w, n, sw, mw, sh);
    else qfig_add(words(row), n, sw, mw, sh);
  }
  __device__ __forceinline__ void add(uint32_t r, uint64_t wait, uint64_t hold) {
    if (r != row) {
      flush();
      row = r;
      n = sw = mw = sh = 0;
    }
    n += 1;
    sw += wait;
    mw = wait > mw ? wait : mw;
    sh += hold;
  }
  // the lanes' last runs, then the head row: every thread of the workgroup calls it
  __device__ __forceinline__ void close() {
    flush();
    __syncthreads();
    if (threadIdx.x == 0 && hd->w[0]) qfig_add(words(hrow), hd->w[0], hd->w[1], hd->w[2], hd->w[3]);
  }
};

// start times and the queue figures from the scan by key's maps
constexpr uint32_t kQSpan = 16;
__global__ void __launch_bounds__(kT) k_qout(K k, uint64_t m, const uint32_t *rkb, const uint32_t *sid,
                                             const MP *in, const MP *inc, uint32_t span) {
  __shared__ QHead s_q;  // (the chunk's first row: a chunk of 4,096 items is mostly one row)
  // a workgroup takes kT x span consecutive sorted items (uniform trip
  // count: its barriers), a wave 64 x span, lane l the items l, l + 64, ...
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t kChunk = (uint64_t)kT * span;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kChunk; c0 < m; c0 += (uint64_t)gridDim.x * kChunk) {
    if (!k.quiet) {
      if (threadIdx.x == 0) QFold::open(&s_q, rkb[c0]);
      __syncthreads();
    }
    QFold fold(k, &s_q);
    const uint64_t j0 = c0 + (uint64_t)wave * 64 * span;
    for (uint64_t j = j0 + lane; j < j0 + 64 * span && j < m; j += 64) {
      const uint32_t i = sid[j];
      const uint32_t r = rkb[j];
      const uint64_t hold = k.row_hold[r];
      const uint64_t S = inc[j].C - hold;
      const uint64_t a = in[j].C - hold;
      store_tracked(k, k.IS + i, S, i);
      if (!k.quiet) fold.add(r, S - a, hold);
    }
    if (!k.quiet) {
      fold.close();
      __syncthreads();  // the head row is emptied for the next chunk
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

// (the order's sources and qitem: above; the queue figures: QFold)
template <uint32_t IPT, int SRC>
__global__ void __launch_bounds__(kT) k_qscan(K k, uint64_t m, QSrc q, QState *qs, uint32_t *ticket, uint32_t tbase,
                                              uint32_t epoch) {
  constexpr uint32_t NW = kT / 64;
  __shared__ uint32_t s_tile;
  __shared__ int64_t w_v[NW], s_cin;
  __shared__ uint32_t w_f[NW];
  __shared__ QHead s_q;  // (the tile's first row)
  if (threadIdx.x == 0) {
    const uint32_t t = atomicAdd(ticket, 1u) - tbase;
    s_tile = t;
    const uint64_t j0 = (uint64_t)t * kT * IPT;
    uint32_t row0;
    if constexpr (SRC == kQArrays) row0 = q.rowk[j0];
    else if constexpr (SRC == kQSorted) row0 = (uint32_t)(q.key[j0] >> (q.ab + q.rb));
    else row0 = k.pos[k.ipos[q.list[SRC == kQKept ? q.ord[j0] : (uint32_t)j0]]].row;
    QFold::open(&s_q, row0);
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
      s = j == 0 || ps != sk || qalone<SRC>(h[r]);
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
  // starts, and the queue figures
  QFold fold(k, &s_q);
#pragma unroll
  for (uint32_t r = 0; r < IPT; ++r) {
    const uint64_t j = w0 + r * 64 + lane;
    if (j >= m) break;
    const uint64_t S = (uint64_t)(f[r] ? v[r] : qmax(c, v[r])) + j * h[r];
    const uint32_t i = it[r];
    store_tracked(k, k.IS + i, S, i);
    if (!k.quiet) fold.add(rw[r], S - a[r], h[r]);
  }
  if (!k.quiet) fold.close();  // (k.quiet is uniform: every thread reaches the barrier or none)
}

// ---- 4b''. worker pools: a pooled round's order refined into rank classes
#include "des_workers.h"
