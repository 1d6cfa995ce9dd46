// Closed-loop arrivals on gfx950 (closed_loop.h): A_j = max(F_c, s_j),
// F_c <- A_j + L_j along each of C connections, a max-plus scan at stride C over the batch.
//
// The batch is a matrix of rows k by C columns in record order.  A row block is R rows; the
// workspace holds one Map per (row block, connection).
//
//   cl_init_info    info = {0, ~0, 0, 0} (the totals below arrive by vector atomics)
//   cl_compose      per row block and connection: the composite of its requests' maps
//   cl_scan_states  per connection: the composites scanned over the row blocks from free_at,
//                   each overwritten by the state at its block's start; free_at, makespan, min
//   cl_apply        per row block: from that state the arrivals, and the late totals
//
// Two regimes (closed_loop.h shape_of).  C >= 64, direct: a workgroup's thread (g, c) owns
// column c of row block blockIdx.x * G + g and steps down its M rows, so a wave reads and
// writes 64 consecutive records per step.  C < 64, staged: a workgroup takes G x 16 rows of
// all C columns, at most 4096 consecutive records, loads their latencies into LDS along the
// record index, thread (g, c) walks 16 rows of column c there, the G sub-blocks of a column
// are scanned through LDS (Hillis-Steele at stride C in the thread index), and the arrivals
// leave through the same LDS words along the record index.  The records are read twice
// (compose, apply), the arrivals written once.  No workgroup waits for another: the launches
// are ordered by the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "closed_loop.h"
#include "hip_check.h"
#include "host_stage.h"

namespace isim {
namespace cl {
namespace dev {

constexpr uint32_t kLoads = 8;                              // records in flight per lane (direct regime)
constexpr uint32_t kStageWords = kThreads * kStageRows;     // 4096 latencies
__device__ __forceinline__ Map identity() { return Map{0, 0}; }

struct ClK {
  const isim_trace_rec *rec;
  uint64_t *arr;
  uint64_t *free_at;          // null: zeros in, nothing out
  unsigned long long *info;
  Map *ws;                    // [n_blocks][C]
  uint64_t n, first, k0, period, n_blocks, R;
  uint32_t C, Cw, G, M, flags;
  uint32_t scan_Cw, scan_G;   // cl_scan_states' own tile width and threads per column
};

// one LDS word per 32 keeps the sub-blocks of a column (16 C words apart) off each other's banks
__device__ __forceinline__ uint32_t pad(uint32_t l) { return l + (l >> 5); }

// Inclusive scan of v over the G threads of a column (thread index g * stride + column); threads
// with g >= G idle.  `excl` is the composite of the threads before this one.
template <uint32_t T>
__device__ __forceinline__ Map group_scan(Map v, uint32_t g, uint32_t G, uint32_t stride, Map *s, Map &excl) {
  const uint32_t tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < G; d <<= 1) {
    const bool on = g < G && g >= d;
    const Map o = on ? s[tid - d * stride] : identity();
    __syncthreads();
    if (on) {
      v = compose(o, v);
      s[tid] = v;
    }
    __syncthreads();
  }
  excl = g < G && g > 0 ? s[tid - stride] : identity();
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(64) cl_init_info(unsigned long long *info) {
  if (threadIdx.x < ISIM_CL_INFO_WORDS) info[threadIdx.x] = threadIdx.x == ISIM_CL_MIN_FREE ? ~0ull : 0ull;
}

// thread (g, cc) of a workgroup: its column, its first row and that row's record and start
struct Lane {
  bool on;
  uint32_t g, c;
  uint64_t block;   // the row block whose workspace entry this thread reads or writes
  int64_t i;        // record index of its first row (below 0 or at or above n: not of the batch)
  uint64_t s;       // scheduled start of its first row
};

template <bool STAGE>
__device__ __forceinline__ Lane lane_of(const ClK &k) {
  Lane t;
  t.g = threadIdx.x / k.Cw;
  t.c = blockIdx.y * k.Cw + (threadIdx.x - t.g * k.Cw);
  t.block = STAGE ? blockIdx.x : (uint64_t)blockIdx.x * k.G + t.g;
  t.on = t.g < k.G && t.c < k.C && t.block < k.n_blocks;
  const uint64_t row = k.k0 + t.block * k.R + (STAGE ? (uint64_t)t.g * k.M : 0);
  t.i = (int64_t)(row * k.C + t.c) - (int64_t)k.first;
  t.s = start_of(t.c, row, k.C, k.period, k.flags);
  return t;
}

// the staged regime's LDS block: latencies in, arrivals out, by l = record index - i_lo
__device__ __forceinline__ void stage_in(const ClK &k, uint64_t *lat, int64_t &i_lo, uint32_t &count) {
  i_lo = (int64_t)((k.k0 + (uint64_t)blockIdx.x * k.R) * k.C) - (int64_t)k.first;
  count = (uint32_t)k.R * k.C;   // G x 16 x C <= 4096
  for (uint32_t l = threadIdx.x; l < count; l += kThreads) {
    const int64_t i = i_lo + l;
    if (i >= 0 && i < (int64_t)k.n) lat[pad(l)] = k.rec[i].latency_ns;
  }
  __syncthreads();
}

// the composite of a lane's M rows
template <bool STAGE>
__device__ __forceinline__ Map fold_rows(const ClK &k, const Lane &t, const uint64_t *lat, int64_t i_lo) {
  Map v = identity();
  if (!t.on) return v;
  uint64_t s = t.s;
  int64_t i = t.i;
  if (STAGE) {
    for (uint32_t m = 0; m < k.M; ++m, i += k.C, s += k.period)
      if (i >= 0 && i < (int64_t)k.n) v = compose(v, request_map(lat[pad((uint32_t)(i - i_lo))], s));
  } else {
    for (uint32_t m0 = 0; m0 < k.M; m0 += kLoads) {
      uint64_t L[kLoads];
      bool ok[kLoads];
#pragma unroll
      for (uint32_t u = 0; u < kLoads; ++u) {
        const int64_t iu = i + (int64_t)u * k.C;
        ok[u] = m0 + u < k.M && iu >= 0 && iu < (int64_t)k.n;
        L[u] = ok[u] ? k.rec[iu].latency_ns : 0;
      }
#pragma unroll
      for (uint32_t u = 0; u < kLoads; ++u, s += k.period)
        if (ok[u]) v = compose(v, request_map(L[u], s));
      i += (int64_t)kLoads * k.C;
    }
  }
  return v;
}

template <bool STAGE>
__global__ void __launch_bounds__(kThreads) cl_compose(ClK k) {
  __shared__ uint64_t lat[STAGE ? kStageWords + kStageWords / 32 : 1];
  __shared__ Map s_scan[STAGE ? kThreads : 1];
  const Lane t = lane_of<STAGE>(k);
  int64_t i_lo = 0;
  uint32_t count = 0;
  if (STAGE) stage_in(k, lat, i_lo, count);
  Map v = fold_rows<STAGE>(k, t, lat, i_lo);
  if (STAGE) {
    Map excl;
    v = group_scan<kThreads>(v, t.g, k.G, k.Cw, s_scan, excl);
    if (t.on && t.g == k.G - 1) k.ws[t.block * k.C + t.c] = v;
  } else if (t.on) {
    k.ws[t.block * k.C + t.c] = v;
  }
}

// One column per thread, or, where C is below the workgroup, scan_G threads per column, each with
// a run of consecutive row blocks, scanned through LDS.
template <uint32_t T>
__global__ void __launch_bounds__(T) cl_scan_states(ClK k) {
  __shared__ Map s_scan[T];
  const uint32_t g = threadIdx.x / k.scan_Cw;
  const uint32_t c = blockIdx.x * k.scan_Cw + (threadIdx.x - g * k.scan_Cw);
  const bool on = g < k.scan_G && c < k.C;
  const uint64_t per = (k.n_blocks + k.scan_G - 1) / k.scan_G;
  const uint64_t b0 = on ? (g * per < k.n_blocks ? g * per : k.n_blocks) : 0;
  const uint64_t b1 = on ? (b0 + per < k.n_blocks ? b0 + per : k.n_blocks) : 0;
  Map v = identity();
#pragma unroll 4
  for (uint64_t b = b0; b < b1; ++b) v = compose(v, k.ws[b * k.C + c]);
  Map excl;
  (void)group_scan<T>(v, on ? g : k.scan_G, k.scan_G, k.scan_Cw, s_scan, excl);
  uint64_t x = on && k.free_at ? k.free_at[c] : 0;
  x = apply(excl, x);
#pragma unroll 4
  for (uint64_t b = b0; b < b1; ++b) {
    const Map m = k.ws[b * k.C + c];
    k.ws[b * k.C + c].a = x;   // the state at the start of row block b
    x = apply(m, x);
  }
  const bool last = on && g == k.scan_G - 1;
  if (last && k.free_at && k.n_blocks) k.free_at[c] = x;
  // makespan and minimum over the connections: per wave, then one atomic each
  uint64_t hi = last ? x : 0, lo = last ? x : ~0ull;
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    const uint64_t oh = __shfl_down(hi, d, 64), ol = __shfl_down(lo, d, 64);
    hi = oh > hi ? oh : hi;
    lo = ol < lo ? ol : lo;
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMax(&k.info[ISIM_CL_MAKESPAN], (unsigned long long)hi);
    atomicMin(&k.info[ISIM_CL_MIN_FREE], (unsigned long long)lo);
  }
}

template <bool STAGE>
__global__ void __launch_bounds__(kThreads) cl_apply(ClK k) {
  __shared__ uint64_t lat[STAGE ? kStageWords + kStageWords / 32 : 1];
  __shared__ Map s_scan[STAGE ? kThreads : 1];
  const Lane t = lane_of<STAGE>(k);
  int64_t i_lo = 0;
  uint32_t count = 0;
  uint64_t x = t.on ? k.ws[t.block * k.C + t.c].a : 0;
  uint64_t late = 0, sum_late = 0;
  if (STAGE) {
    stage_in(k, lat, i_lo, count);
    const Map v = fold_rows<STAGE>(k, t, lat, i_lo);
    Map excl;
    (void)group_scan<kThreads>(v, t.g, k.G, k.Cw, s_scan, excl);
    x = apply(excl, x);
    if (t.on) {
      uint64_t s = t.s;
      int64_t i = t.i;
      for (uint32_t m = 0; m < k.M; ++m, i += k.C, s += k.period) {
        if (i < 0 || i >= (int64_t)k.n) continue;
        uint64_t &w = lat[pad((uint32_t)(i - i_lo))];
        const uint64_t a = x > s ? x : s;
        x = sat_add(a, w);
        w = a;
        late += a > s;
        sum_late += a - s;
      }
    }
    __syncthreads();
    for (uint32_t l = threadIdx.x; l < count; l += kThreads) {
      const int64_t i = i_lo + l;
      if (i >= 0 && i < (int64_t)k.n) k.arr[i] = lat[pad(l)];
    }
  } else if (t.on) {
    uint64_t s = t.s;
    int64_t i = t.i;
    for (uint32_t m0 = 0; m0 < k.M; m0 += kLoads) {
      uint64_t L[kLoads];
      bool ok[kLoads];
#pragma unroll
      for (uint32_t u = 0; u < kLoads; ++u) {
        const int64_t iu = i + (int64_t)u * k.C;
        ok[u] = m0 + u < k.M && iu >= 0 && iu < (int64_t)k.n;
        L[u] = ok[u] ? k.rec[iu].latency_ns : 0;
      }
#pragma unroll
      for (uint32_t u = 0; u < kLoads; ++u, s += k.period) {
        if (!ok[u]) continue;
        const uint64_t a = x > s ? x : s;
        x = sat_add(a, L[u]);
        k.arr[i + (int64_t)u * k.C] = a;
        late += a > s;
        sum_late += a - s;
      }
      i += (int64_t)kLoads * k.C;
    }
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    late += __shfl_down(late, d, 64);
    sum_late += __shfl_down(sum_late, d, 64);
  }
  if ((threadIdx.x & 63u) == 0 && late) {   // late 0: a - s was 0 for every request of the wave
    atomicAdd(&k.info[ISIM_CL_LATE], (unsigned long long)late);
    atomicAdd(&k.info[ISIM_CL_SUM_LATE], (unsigned long long)sum_late);
  }
}

}  // namespace dev

int launch(const Client &c, const isim_trace_rec *d_records, uint64_t n, uint64_t *d_free_at,
           uint64_t *d_arrivals, uint64_t *d_info, void *d_workspace, void *stream_) {
  using namespace dev;
  hipStream_t stream = (hipStream_t)stream_;
  ClK k{};
  k.rec = d_records;
  k.arr = d_arrivals;
  k.free_at = d_free_at;
  k.info = (unsigned long long *)d_info;
  k.ws = (Map *)d_workspace;
  k.n = n;
  k.first = c.first_index;
  k.period = c.period_ns;
  k.C = c.connections;
  k.flags = c.flags;
  const bool wide = k.C >= kScanThreads;   // a column per thread fills many workgroups
  k.scan_Cw = wide ? kThreads : k.C;
  k.scan_G = wide ? 1 : kScanThreads / k.C;
  Shape s{};
  dim3 grid;
  hipLaunchKernelGGL(cl_init_info, dim3(1), dim3(64), 0, stream, k.info);
  if (n) {
    s = shape_of(n, k.C);
    k.Cw = s.Cw;
    k.G = s.G;
    k.M = s.M;
    k.R = s.R;
    k.k0 = c.first_index / k.C;
    const uint64_t rows = (c.first_index + n - 1) / k.C - k.k0 + 1;
    k.n_blocks = (rows + s.R - 1) / s.R;   // <= s.max_blocks, which sized the workspace
    grid = dim3((uint32_t)(s.stage ? k.n_blocks : (k.n_blocks + s.G - 1) / s.G), s.tiles);
    if (s.stage) hipLaunchKernelGGL(cl_compose<true>, grid, dim3(kThreads), 0, stream, k);
    else hipLaunchKernelGGL(cl_compose<false>, grid, dim3(kThreads), 0, stream, k);
  }
  // n 0: no row blocks, the totals of the incoming state
  if (wide) hipLaunchKernelGGL(cl_scan_states<kThreads>, dim3((k.C + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, k);
  else hipLaunchKernelGGL(cl_scan_states<kScanThreads>, dim3(1), dim3(kScanThreads), 0, stream, k);
  if (n) {
    if (s.stage) hipLaunchKernelGGL(cl_apply<true>, grid, dim3(kThreads), 0, stream, k);
    else hipLaunchKernelGGL(cl_apply<false>, grid, dim3(kThreads), 0, stream, k);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace cl
}  // namespace isim

namespace {
namespace cl = isim::cl;
int cfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "closed loop: " + msg); }
}  // namespace

extern "C" {

int isim_closed_loop_device(const cl::Client *p, const isim_trace_rec *d_records, uint64_t n,
                            uint64_t *d_free_at, uint64_t *d_arrivals, uint64_t *d_info, void *d_workspace,
                            uint64_t workspace_bytes, void *hip_stream) {
  if (const char *m = cl::batch_error(p, n); *m) return cfail(m);
  if (!d_info) return cfail("null d_info");
  if (n && (!d_records || !d_arrivals)) return cfail("null d_records or d_arrivals");
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_arrivals & 7u) || ((uintptr_t)d_free_at & 7u) ||
      ((uintptr_t)d_info & 7u) || ((uintptr_t)d_workspace & 7u))
    return cfail("d_records must be 16-byte aligned, d_free_at, d_arrivals, d_info and d_workspace 8-byte aligned");
  const uint64_t need = cl::workspace_bytes(n, p->connections);
  if (n && (!d_workspace || workspace_bytes < need))
    return cfail("workspace too small: " + std::to_string(d_workspace ? workspace_bytes : 0) + " bytes, need " +
                 std::to_string(need) + " (isim_closed_loop_workspace_bytes)");
  if (cl::launch(*p, d_records, n, d_free_at, d_arrivals, d_info, d_workspace, hip_stream))
    return isim::set_error(ISIM_EHIP, "closed loop: kernel launch failed");
  return ISIM_OK;
}

int isim_closed_loop(int device, const cl::Client *p, const isim_trace_rec *h_records, uint64_t n,
                     uint64_t *h_free_at, uint64_t *h_arrivals, uint64_t *h_info) {
  if (const char *m = cl::batch_error(p, n); *m) return cfail(m);
  if (!h_info) return cfail("null h_info");
  if (n && (!h_records || !h_arrivals)) return cfail("null h_records or h_arrivals");
  const uint64_t state_bytes = h_free_at ? (uint64_t)p->connections * 8 : 0, wsb = cl::workspace_bytes(n, p->connections);
  isim::HostStage stage(device);
  void *d_arr = stage.alloc(n * 8), *d_info = stage.alloc(ISIM_CL_INFO_WORDS * 8), *d_ws = stage.alloc(wsb);
  void *d_free = stage.upload(h_free_at, state_bytes), *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_closed_loop_device(p, (const isim_trace_rec *)d_rec, n, (uint64_t *)d_free, (uint64_t *)d_arr,
                                             (uint64_t *)d_info, d_ws, wsb, stage.stream()))
    return rc;
  if (const int rc = stage.download(h_info, d_info, ISIM_CL_INFO_WORDS * 8)) return rc;
  if (const int rc = stage.download(h_free_at, d_free, state_bytes)) return rc;
  return stage.download(h_arrivals, d_arr, n * 8);
}

}  // extern "C"
