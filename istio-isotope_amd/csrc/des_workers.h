// DES worker pools: W workers per replica behind one
// FIFO queue, on the item engine.  A part of des_items.hip, included inside
// namespace isim::dit where des_items_queue.h ends (it uses kT, gid, nthreads
// and MP).
//
// With a constant hold h the request of FIFO rank p of a replica starts at
//   S_p = max(a_p, S_{p-W} + h),
// so the replica is W one-worker queues fed cyclically: rank p goes to
// sub-queue p mod W, where it is request p div W.  k_qscan and the scan by key
// solve a one-worker queue over any contiguous run in FIFO order with one
// hold, so all a pooled round needs is its order REFINED: every (row, replica)
// segment of the round's FIFO order (k_pairs<SRC>'s or k_pairs2's arrays)
// laid out as its min(W, L) rank classes, each contiguous and in FIFO order,
// each a segment of its own.
//
//   1. k_wk_tile, k_wk_carry, k_wk_rank: a head-flag scan in three launches
//      (reduce per tile, one workgroup over the tiles, scan per tile with the
//      carry): start[j] = the index of j's segment's first item; the last item
//      of a segment writes the segment's length at len[start].  No workgroup
//      waits for another: the launches order them.
//   2. k_wk_scatter: item of rank p = j - start[j] of a segment of L items and
//      W workers goes to
//        start + c floor(L / W) + min(c, L mod W) + p div W,   c = p mod W,
//      the classes 0 .. L mod W - 1 holding one item more.  The class's first
//      index is its segment key: unique in the round, constant over the class.
#pragma once

constexpr uint32_t kWkPer = kWkTile / kT;  // consecutive items per thread
static_assert(kWkTile % kT == 0, "a tile is a whole number of items per thread");

// item j starts a segment
__device__ __forceinline__ bool wk_head(const uint32_t *segk, uint64_t j) { return j == 0 || segk[j] != segk[j - 1]; }

// the workgroup's inclusive prefix maximum over its threads' values, thread order
__device__ __forceinline__ uint32_t wk_block_scan(uint32_t v, uint32_t *s_w) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v = o > v ? o : v;
  }
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  for (uint32_t w = 0; w < wave; ++w) v = s_w[w] > v ? s_w[w] : v;
  __syncthreads();  // s_w is free again
  return v;
}

// 1a. per tile the index of its last segment start (0: none, or item 0)
__global__ void __launch_bounds__(kT) k_wk_tile(const uint32_t *segk, uint64_t m, uint32_t *tile) {
  __shared__ uint32_t s_w[kT / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * kWkTile + (uint64_t)threadIdx.x * kWkPer;
  uint32_t v = 0;
  for (uint32_t q = 0; q < kWkPer; ++q) {
    const uint64_t j = j0 + q;
    if (j < m && wk_head(segk, j)) v = (uint32_t)j;
  }
  v = wk_block_scan(v, s_w);
  if (threadIdx.x == kT - 1) tile[blockIdx.x] = v;
}

// 1b. the tiles' values into their inclusive prefix maxima, one workgroup
__global__ void __launch_bounds__(kT) k_wk_carry(uint32_t *tile, uint32_t n_tiles) {
  __shared__ uint32_t s_w[kT / 64];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kT) {
    const uint32_t t = t0 + threadIdx.x;
    uint32_t v = t < n_tiles ? tile[t] : 0u;
    v = wk_block_scan(v, s_w);
    const uint32_t c = s_carry;
    v = c > v ? c : v;
    if (t < n_tiles) tile[t] = v;
    __syncthreads();  // every thread has read the carry
    if (threadIdx.x == kT - 1) s_carry = v;
    __syncthreads();
  }
}

// 1c. each item's segment start; a segment's last item writes its length at the start
__global__ void __launch_bounds__(kT) k_wk_rank(const uint32_t *segk, uint64_t m, const uint32_t *tile,
                                                uint32_t *start, uint32_t *len) {
  __shared__ uint32_t s_w[kT / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * kWkTile + (uint64_t)threadIdx.x * kWkPer;
  uint32_t h[kWkPer], v = 0;
  for (uint32_t q = 0; q < kWkPer; ++q) {
    const uint64_t j = j0 + q;
    if (j < m && wk_head(segk, j)) v = (uint32_t)j;
    h[q] = v;  // the thread's last start up to its item q
  }
  const uint32_t incl = wk_block_scan(v, s_w);
  // the last start before this thread's items: the threads below (the exclusive prefix) and the tiles before
  __shared__ uint32_t s_incl[kT];
  s_incl[threadIdx.x] = incl;
  __syncthreads();
  uint32_t ex = threadIdx.x ? s_incl[threadIdx.x - 1] : 0u;
  const uint32_t carry = blockIdx.x ? tile[blockIdx.x - 1] : 0u;
  ex = carry > ex ? carry : ex;
  for (uint32_t q = 0; q < kWkPer; ++q) {
    const uint64_t j = j0 + q;
    if (j >= m) break;
    const uint32_t st = h[q] > ex ? h[q] : ex;
    start[j] = st;
    if (j + 1 == m || segk[j + 1] != segk[j]) len[st] = (uint32_t)(j + 1) - st;
  }
}

// 2. the refined order: each segment as its rank classes
struct WkArrays {
  const uint32_t *segk, *rowk, *sid;  // the round's FIFO order (k_pairs*)
  const MP *mp;
  const uint32_t *start, *len;        // k_wk_rank
  const uint32_t *row_workers;        // per duration-table row
  uint32_t *o_segk, *o_rowk, *o_sid;  // the refined order
  MP *o_mp;
};
__global__ void __launch_bounds__(kT) k_wk_scatter(WkArrays w, uint64_t m) {
  for (uint64_t j = gid(); j < m; j += nthreads()) {
    const uint32_t st = w.start[j], L = w.len[st], row = w.rowk[j];
    const uint32_t W = w.row_workers[row];
    const uint32_t p = (uint32_t)j - st;
    const uint32_t c = p % W, base = L / W, rem = L % W;
    const uint32_t cs = st + c * base + (c < rem ? c : rem);  // the class's first index
    const uint32_t dst = cs + p / W;
    if (dst >= m) continue;  // never: dst < st + L <= m (a guard against a torn segment table)
    w.o_segk[dst] = cs;
    w.o_rowk[dst] = row;
    w.o_sid[dst] = w.sid[j];
    w.o_mp[dst] = w.mp[j];
  }
}
