// The DES level engine's wave and block scans: max-plus maps (replicated
// services), sums (arrivals) and the running maxima of the closed-form queues
// by DPP, 64-bit and 32-bit.
//
// Included by des.hip INSIDE namespace isim::dev (as des_draw.h: a piece of
// that translation unit, not a header of its own).

// (B, C) represents x -> max(x + B, C); `then` composes a after b.
struct MaxPlus {
  uint64_t B, C;
};
__device__ __forceinline__ MaxPlus mp_then(MaxPlus first, MaxPlus second) {
  const uint64_t c = first.C + second.B;
  return {first.B + second.B, c > second.C ? c : second.C};
}

// Inclusive block scan of MaxPlus over kDesThreads threads (wave shuffles +
// one LDS pass over the 16 wave totals).
template <uint32_t NT = kDesThreads>
__device__ __forceinline__ MaxPlus mp_block_scan(MaxPlus v, MaxPlus *wtot) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    MaxPlus o;
    o.B = __shfl_up(v.B, d, 64);
    o.C = __shfl_up(v.C, d, 64);
    if (lane >= d) v = mp_then(o, v);
  }
  if (lane == 63) wtot[wave] = v;
  __syncthreads();
  if (wave == 0) {
    MaxPlus w = lane < NT / 64 ? wtot[lane] : MaxPlus{0, 0};
#pragma unroll
    for (uint32_t d = 1; d < NT / 64; d <<= 1) {
      MaxPlus o;
      o.B = __shfl_up(w.B, d, 64);
      o.C = __shfl_up(w.C, d, 64);
      if (lane >= d) w = mp_then(o, w);
    }
    if (lane < NT / 64) wtot[lane] = w;
  }
  __syncthreads();
  if (wave > 0) v = mp_then(wtot[wave - 1], v);
  __syncthreads();  // wtot is reused by the next call
  return v;
}

__device__ __forceinline__ uint64_t block_scan_add(uint64_t v, uint64_t *wtot, uint64_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) wtot[wave] = v;
  __syncthreads();
  if (wave == 0) {
    uint64_t w = lane < kDesThreads / 64 ? wtot[lane] : 0;
#pragma unroll
    for (uint32_t d = 1; d < kDesThreads / 64; d <<= 1) {
      const uint64_t o = __shfl_up(w, d, 64);
      if (lane >= d) w += o;
    }
    if (lane < kDesThreads / 64) wtot[lane] = w;
  }
  __syncthreads();
  if (wave > 0) v += wtot[wave - 1];
  total = wtot[kDesThreads / 64 - 1];
  __syncthreads();
  return v;  // inclusive
}

// ---- single-replica queues in closed form.  A FIFO worker with hold h fed
// arrivals a_t in trace order starts trace t at
//   S_t = max(S_{t-1} + h, a_t) = t h + max_{s <= t} (a_s - s h)
// (an idle worker at time 0 contributes 0), so the queue is ONE running max
// of the signed keys a_t - t h: a wave max-scan by DPP row shifts and row
// broadcasts, wave totals through LDS, the carry across chunks a running max
// (the host bounds n_traces x hold below 2^62, des_host.hip).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int64_t dpp_i64(int64_t old, int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)old, (int)(uint32_t)v, CTRL, ROW_MASK,
                                                           0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)((uint64_t)old >> 32),
                                                           (int)(uint32_t)((uint64_t)v >> 32), CTRL, ROW_MASK, 0xF,
                                                           false);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t max_i64(int64_t a, int64_t b) { return a > b ? a : b; }
constexpr int64_t kKeyMin = INT64_MIN;
// a lane's value moved by a full-mask DPP control, 0 where the source lane
// does not exist (bound_ctrl: no register to preset)
template <int CTRL>
__device__ __forceinline__ int64_t dpp0_i64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)v, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)((uint64_t)v >> 32), CTRL, 0xF, 0xF, true);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// inclusive max-scan over the wave's 64 lanes of max(0, v): every prefix the
// queues need is at least 0 (the idle start), so lanes past an edge read 0
__device__ __forceinline__ int64_t wave_max_scan(int64_t v) {
  v = max_i64(v, dpp0_i64<0x111>(v));              // row_shr:1
  v = max_i64(v, dpp0_i64<0x112>(v));              // row_shr:2
  v = max_i64(v, dpp0_i64<0x114>(v));              // row_shr:4
  v = max_i64(v, dpp0_i64<0x118>(v));              // row_shr:8
  v = max_i64(v, dpp_i64<0x142, 0xA>(v, v));       // row_bcast:15 into rows 1, 3 (rows 0, 2 keep v)
  v = max_i64(v, dpp_i64<0x143, 0xC>(v, v));       // row_bcast:31 into rows 2, 3
  return v;
}
// the previous lane's value (lane 0: 0)
__device__ __forceinline__ int64_t wave_shr1(int64_t v) { return dpp0_i64<0x138>(v); }
__device__ __forceinline__ int64_t read_lane(int64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), (int)l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the block's wave totals (LDS, NW <= 16): pre = max(carry, totals of the
// waves before `wave`), carry = max(carry, all totals); both wave-uniform
template <uint32_t NW>
__device__ __forceinline__ void fold_totals(const int64_t *wtot, uint32_t wave, int64_t &carry, int64_t &pre) {
  static_assert(NW >= 2 && NW <= 16, "one DPP row of wave totals");
  const uint32_t lane = threadIdx.x & 63u;
  int64_t v = lane < NW ? wtot[lane] : 0;  // totals are >= 0 (wave_max_scan)
  v = max_i64(v, dpp0_i64<0x111>(v));
  v = max_i64(v, dpp0_i64<0x112>(v));
  v = max_i64(v, dpp0_i64<0x114>(v));
  if constexpr (NW > 8) v = max_i64(v, dpp0_i64<0x118>(v));
  const int64_t before = wave ? read_lane(v, wave - 1) : kKeyMin;
  pre = max_i64(carry, before);
  carry = max_i64(carry, read_lane(v, NW - 1));
}

// ---- the 32-bit keys of narrow rows (des_queue.h, down1_chunk_n32): a trace
// group is one DPP row
__device__ __forceinline__ int32_t max_i32(int32_t a, int32_t b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ int32_t dpp_max32(int32_t v) {
  return max_i32(v, __builtin_amdgcn_update_dpp((int)INT32_MIN, v, CTRL, 0xF, 0xF, false));
}
// inclusive max-scan within each DPP row (INT32_MIN where a source lane does not exist)
__device__ __forceinline__ int32_t row_max_scan32(int32_t v) {
  v = dpp_max32<0x111>(v);  // row_shr:1
  v = dpp_max32<0x112>(v);  // row_shr:2
  v = dpp_max32<0x114>(v);  // row_shr:4
  v = dpp_max32<0x118>(v);  // row_shr:8
  return v;
}
