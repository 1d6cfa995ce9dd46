// Arrival times under a load profile on gfx950 (load_profile.h, DESIGN.md
// §17): A[i] = t(u_i), u_i the running work of the batch's traces.
//
//   lp_work_chunks  per chunk of 8192 traces: the draw, its Q24 exponential,
//                   the chunk's inclusive prefix of work into A, its sum into blk
//   lp_scan_blocks  exclusive scan of the chunk sums (one workgroup)
//   lp_map_chunks   u = prefix + chunk offset, then t(u) through the table.
//                   The u of a chunk do not decrease, so its first and last u
//                   bound the segments it can meet: only those go to LDS (24 B
//                   each, 24 KB at 1024 segments), and a chunk inside one
//                   segment searches nothing.
//
// Paced profiles have u_i = (i + 1) 2^24 in closed form: the map kernel alone.
// No workgroup waits for another; the launches are ordered by the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "des.h"
#include "des_layout.h"
#include "load_profile.h"

namespace isim {
namespace lp {
namespace dev {

#include "des_draw.h"

constexpr uint32_t kPer = 8;  // traces per thread, as des.hip's arrivals
constexpr uint32_t kThreads = 1024;
constexpr uint32_t kChunk = kPer * kThreads;
// des_launch hands these kernels the static engine's chunk sums (DesBufs::blk), which des_layout.h sizes
static_assert(kChunk == kDesArrChunk, "the profile arrivals' chunks are the ones des_layout.h sizes blk for");
constexpr uint32_t kPack = 128;  // segments per upload launch: 3 KB of kernel arguments
constexpr uint64_t kUnit = 1ull << 24;

struct LpK {
  uint64_t *A;        // [N] work prefixes in, arrival times out
  uint64_t *blk;      // [n_blk + 1] chunk sums, then chunk offsets (null: A holds the whole prefix)
  const Seg *seg;     // [n_seg]
  uint64_t N, trace_begin;
  uint32_t k0, k1;
  uint32_t n_blk, n_seg;
};

struct SegPack {
  Seg s[kPack];
};

__global__ void __launch_bounds__(kPack) lp_upload(SegPack p, Seg *dst, uint32_t count) {
  if (threadIdx.x < count) dst[threadIdx.x] = p.s[threadIdx.x];
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
    uint64_t w = lane < kThreads / 64 ? wtot[lane] : 0;
#pragma unroll
    for (uint32_t d = 1; d < kThreads / 64; d <<= 1) {
      const uint64_t o = __shfl_up(w, d, 64);
      if (lane >= d) w += o;
    }
    if (lane < kThreads / 64) wtot[lane] = w;
  }
  __syncthreads();
  if (wave > 0) v += wtot[wave - 1];
  total = wtot[kThreads / 64 - 1];
  __syncthreads();
  return v;  // inclusive
}

__device__ __forceinline__ uint64_t trace_work(const LpK &k, uint64_t t) {
  return des_exp_q24(des_draw(k.trace_begin + t, 0u, 0x80000001u, 0, k.k0, k.k1));
}

// the work of every trace alone (the item engine scans it itself)
__global__ void __launch_bounds__(256) lp_work(LpK k, uint32_t paced) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < k.N; t += stride)
    k.A[t] = paced ? kUnit : trace_work(k, t);
}

__global__ void __launch_bounds__(kThreads) lp_work_chunks(LpK k) {
  __shared__ uint64_t wtot[kThreads / 64];
  const uint64_t base = (uint64_t)blockIdx.x * kChunk + (uint64_t)threadIdx.x * kPer;
  uint64_t x[kPer], s = 0;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    x[i] = base + i < k.N ? trace_work(k, base + i) : 0;
    s += x[i];
  }
  uint64_t total;
  uint64_t run = block_scan_add(s, wtot, total) - s;
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    run += x[i];
    if (base + i < k.N) k.A[base + i] = run;
  }
  if (threadIdx.x == 0) k.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) lp_scan_blocks(LpK k) {
  __shared__ uint64_t wtot[kThreads / 64];
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < k.n_blk; b0 += kThreads) {
    const uint32_t b = b0 + threadIdx.x;
    const uint64_t v = b < k.n_blk ? k.blk[b] : 0;
    uint64_t total;
    const uint64_t inc = block_scan_add(v, wtot, total);
    if (b < k.n_blk) k.blk[b] = carry + inc - v;
    carry += total;
  }
}

// A[i] = t(u_i) for one chunk; PACED: u_i = (i + 1) 2^24, else A[i] + the chunk's offset
template <bool PACED>
__global__ void __launch_bounds__(kThreads) lp_map_chunks(LpK k) {
  __shared__ Seg s_seg[kMaxSegments];
  const uint64_t c0 = (uint64_t)blockIdx.x * kChunk;  // c0 < N: one workgroup per chunk of the batch
  const uint64_t c1 = c0 + kChunk < k.N ? c0 + kChunk : k.N;
  const uint64_t off = PACED || !k.blk ? 0 : k.blk[blockIdx.x];
  auto work = [&](uint64_t i) { return PACED ? (i + 1) * kUnit : k.A[i] + off; };
  // the chunk's segments [jlo, jhi] (workgroup-uniform)
  const uint32_t jlo = find_seg(k.seg, k.n_seg, work(c0));
  const uint32_t jhi = jlo + find_seg(k.seg + jlo, k.n_seg - jlo, work(c1 - 1));
  const uint32_t nj = jhi - jlo + 1;
  for (uint32_t j = threadIdx.x; j < nj; j += kThreads) s_seg[j] = k.seg[jlo + j];
  __syncthreads();
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += kThreads) {
    const uint64_t u = work(i);
    uint64_t t;
    (void)seg_time(s_seg[nj > 1 ? find_seg(s_seg, nj, u) : 0], u, t);  // below 2^62: the host checked the horizon
    k.A[i] = t;
  }
}

}  // namespace dev

uint64_t arrival_blocks(uint64_t n) { return (n + dev::kChunk - 1) / dev::kChunk; }

int upload(const Compiled &c, Seg *d_seg, void *stream) {
  const uint32_t n = (uint32_t)c.seg.size();
  for (uint32_t j0 = 0; j0 < n; j0 += dev::kPack) {
    dev::SegPack p{};
    const uint32_t cnt = n - j0 < dev::kPack ? n - j0 : dev::kPack;
    for (uint32_t j = 0; j < cnt; ++j) p.s[j] = c.seg[j0 + j];
    hipLaunchKernelGGL(dev::lp_upload, dim3(1), dim3(dev::kPack), 0, (hipStream_t)stream, p, d_seg + j0, cnt);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

static dev::LpK make_k(uint64_t seed, const DeviceProfile &p, uint64_t trace_begin, uint64_t n, uint64_t *d_a,
                       uint64_t *d_blk) {
  dev::LpK k{};
  k.A = d_a;
  k.blk = d_blk;
  k.seg = p.d_seg;
  k.N = n;
  k.trace_begin = trace_begin;
  k.k0 = (uint32_t)seed;
  k.k1 = (uint32_t)(seed >> 32);
  k.n_blk = (uint32_t)arrival_blocks(n);
  k.n_seg = p.n_seg;
  return k;
}

int arrivals_launch(uint64_t seed, const DeviceProfile &p, uint64_t trace_begin, uint64_t n, uint64_t *d_arrivals,
                    uint64_t *d_blk, void *stream_) {
  using namespace dev;
  hipStream_t stream = (hipStream_t)stream_;
  const LpK k = make_k(seed, p, trace_begin, n, d_arrivals, d_blk);
  if (p.paced) {
    hipLaunchKernelGGL(lp_map_chunks<true>, dim3(k.n_blk), dim3(kThreads), 0, stream, k);
  } else {
    hipLaunchKernelGGL(lp_work_chunks, dim3(k.n_blk), dim3(kThreads), 0, stream, k);
    hipLaunchKernelGGL(lp_scan_blocks, dim3(1), dim3(kThreads), 0, stream, k);
    hipLaunchKernelGGL(lp_map_chunks<false>, dim3(k.n_blk), dim3(kThreads), 0, stream, k);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int work_launch(uint64_t seed, const DeviceProfile &p, uint64_t trace_begin, uint64_t n, uint64_t *d_work,
                void *stream) {
  const dev::LpK k = make_k(seed, p, trace_begin, n, d_work, nullptr);
  uint64_t g = (n + 255) / 256;
  g = g < 65536 ? g : 65536;
  hipLaunchKernelGGL(dev::lp_work, dim3((uint32_t)g), dim3(256), 0, (hipStream_t)stream, k, p.paced);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int map_launch(const DeviceProfile &p, uint64_t n, uint64_t *d_arrivals, void *stream) {
  const dev::LpK k = make_k(0, p, 0, n, d_arrivals, nullptr);
  hipLaunchKernelGGL(dev::lp_map_chunks<false>, dim3(k.n_blk), dim3(dev::kThreads), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace lp
}  // namespace isim
