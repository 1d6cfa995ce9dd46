// Exact latency percentiles on the device (include/isim.h isim_latency_quantiles*,
// DESIGN.md §13): MSD radix select over the latency_ns of the 16-byte trace
// records, every class (all / 200 / 500) and every quantile in one sweep per
// 8-bit digit.  A fixed sequence of launches on the caller's stream: no host
// synchronisation, no allocation, no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/isim.h"
#include "host_stage.h"
#include "quantile_rank.h"
#include "segmented_select.h"
#include "trace_rec_dev.h"

namespace {

namespace rs = isim::rs;
using isim::dev::rec4;
using rs::kBins;
using rs::kClasses;
using rs::kMaxQ;

using rs::kHistThreads;
using rs::kResolveThreads;
using rs::kUnroll;
constexpr uint32_t kHistMaxGrid = 768;  // 3 per CU; a workgroup's u32 LDS bins hold 2^40 / 768 < 2^32 records
constexpr uint64_t kMaxRecords = 1ull << 40;

int qfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, msg); }

// The select's state (radix_select.h), at the start of the workspace; the u64
// histogram [3][n_q][256] follows it.
struct QState {
  uint64_t cnt[kClasses];  // records per class (cnt[0] = n)
  uint64_t any;            // OR of every latency: the bytes above its top bit are zero
  int32_t top_byte;        // most significant byte with a set bit; -1: every latency is 0
  rs::State<uint64_t> sel;
};

constexpr uint64_t kStateBytes = (sizeof(QState) + 255) & ~255ull;
static_assert(kStateBytes == 1536, "isim_quantiles_workspace_bytes is pinned");

uint64_t workspace_bytes(uint32_t n_q) { return kStateBytes + (uint64_t)kClasses * n_q * kBins * 8; }

using isim::q::nearest_rank;  // quantile_rank.h

// Zeroes the workspace the select uses (the caller may hand over a dirty one),
// or the output of an empty batch.  A kernel like the rest of the sequence, so
// a captured call is a chain of kernel nodes only.
__global__ __launch_bounds__(1024) void k_quantile_clear(unsigned long long *words, uint32_t n_words) {
  rs::clear_words<1024>(words, n_words);
}

// Pass 0: per class the record count, and the OR of the latencies.
__global__ __launch_bounds__(256) void k_quantile_count(const rec4 *__restrict__ rec, uint64_t n, QState *st) {
  __shared__ unsigned long long s_any[4];
  __shared__ unsigned long long s_500[4];
  unsigned long long any = 0, n500 = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const rec4 r = isim::dev::load_rec(rec, i);
    any |= isim::dev::latency(r);
    n500 += isim::dev::code(r);
  }
  for (int d = 32; d; d >>= 1) {
    any |= __shfl_xor(any, d, 64);
    n500 += __shfl_xor(n500, d, 64);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_any[wave] = any;
    s_500[wave] = n500;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    any = s_any[0] | s_any[1] | s_any[2] | s_any[3];
    n500 = s_500[0] + s_500[1] + s_500[2] + s_500[3];
    if (any) atomicOr((unsigned long long *)&st->any, any);
    if (n500) atomicAdd((unsigned long long *)&st->cnt[ISIM_Q_500], n500);
  }
}

// After pass 0: the ranks from the counts (on the device: the host never sees
// the class counts), one group per non-empty class, the first digit pass.
__global__ __launch_bounds__(64) void k_quantile_setup(QState *st, uint64_t n, rs::Ppm q, uint32_t n_q, uint64_t *out) {
  const uint32_t t = threadIdx.x;
  const uint64_t n500 = st->cnt[ISIM_Q_500];
  const uint64_t any = st->any;
  __syncthreads();  // every thread has read cnt[500] before thread 0 rewrites the counts
  rs::setup(st->sel, t, n_q, n, n - n500, n500, q, (unsigned long long *)out);
  if (t == 0) {
    st->cnt[ISIM_Q_ALL] = n;
    st->cnt[ISIM_Q_200] = n - n500;
    st->top_byte = rs::top_byte(any);
  }
}

// Digit pass `byte`: rs::hist_pass over a grid-stride share of the records,
// into the global u64 histogram.
__global__ __launch_bounds__(kHistThreads) void k_quantile_hist(const rec4 *__restrict__ rec, uint64_t n,
                                                               const QState *__restrict__ st,
                                                               unsigned long long *__restrict__ ghist, uint32_t n_q,
                                                               int byte) {
  __shared__ rs::HistLds lds;
  if (byte > st->top_byte) return;  // every latency is zero in this byte: the prefixes keep a zero digit
  // a wave takes 64 * kUnroll consecutive records per step
  const uint64_t wave = (uint64_t)blockIdx.x * (kHistThreads / 64) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (kHistThreads / 64) * (64 * kUnroll);
  const auto keys = [&] {
    return [=](uint64_t i, bool live) {
      const rec4 r = isim::dev::load_rec(rec, i, live);
      return rs::Key{isim::dev::latency(r), 1u + isim::dev::code(r)};
    };
  };
  rs::hist_pass(lds, st->sel, n_q, byte, wave * (64 * kUnroll), n, step, keys, ghist);
}

// After digit pass `byte`, one workgroup: rs::resolve_pass.
__global__ __launch_bounds__(kResolveThreads) void k_quantile_resolve(QState *st, unsigned long long *ghist,
                                                                     uint32_t n_q, int byte, uint64_t *out) {
  rs::resolve_pass(st->sel, ghist, n_q, byte, st->top_byte, (unsigned long long *)out);
}

int check_q(const uint32_t *q_ppm, uint32_t n_q, uint64_t n_records) {
  if (const std::string m = isim::q::list_error(q_ppm, n_q); !m.empty()) return qfail(m);
  if (n_records > kMaxRecords) return qfail("n_records is above 2^40");
  return ISIM_OK;
}

}  // namespace

extern "C" {

int isim_quantile_rank(uint64_t n, uint32_t q_ppm, uint64_t *k) {
  if (!k) return qfail("null argument");
  if (n == 0 || n > kMaxRecords) return qfail("n must be 1..2^40");
  if (q_ppm > 1000000u) return qfail("q_ppm is above 1000000");
  *k = nearest_rank(n, q_ppm);
  return ISIM_OK;
}

int isim_quantiles_workspace_bytes(uint32_t n_q, uint64_t *bytes) {
  if (!bytes) return qfail("null argument");
  if (n_q == 0 || n_q > kMaxQ) return qfail("n_q must be 1.." + std::to_string(kMaxQ));
  *bytes = workspace_bytes(n_q);
  return ISIM_OK;
}

int isim_latency_quantiles_device(const isim_trace_rec *d_records, uint64_t n_records, const uint32_t *q_ppm,
                                  uint32_t n_q, uint64_t *d_out, void *d_workspace, uint64_t workspace_bytes_,
                                  void *hip_stream) {
  if (const int rc = check_q(q_ppm, n_q, n_records)) return rc;
  if (!d_out || !d_workspace) return qfail("null d_out or d_workspace");
  if (workspace_bytes_ < workspace_bytes(n_q))
    return qfail("workspace too small: " + std::to_string(workspace_bytes_) + " bytes, need " +
                 std::to_string(workspace_bytes(n_q)) + " (isim_quantiles_workspace_bytes)");
  if (n_records && !d_records) return qfail("null d_records");
  if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_workspace & 7u) || ((uintptr_t)d_out & 7u))
    return qfail("d_records must be 16-byte aligned, d_out and d_workspace 8-byte aligned");
  const hipStream_t s = (hipStream_t)hip_stream;
  if (n_records == 0) {
    hipLaunchKernelGGL(k_quantile_clear, dim3(1), dim3(1024), 0, s, (unsigned long long *)d_out,
                       (uint32_t)ISIM_Q_OUT_WORDS(n_q));
    ISIM_HIPCHK(hipGetLastError());
    return ISIM_OK;
  }
  QState *st = (QState *)d_workspace;
  unsigned long long *ghist = (unsigned long long *)((char *)d_workspace + kStateBytes);
  const rec4 *rec = (const rec4 *)d_records;
  hipLaunchKernelGGL(k_quantile_clear, dim3(1), dim3(1024), 0, s, (unsigned long long *)d_workspace,
                     (uint32_t)(workspace_bytes(n_q) / 8));
  const uint32_t count_grid = (uint32_t)std::min<uint64_t>((n_records + 1023) / 1024, 2048);
  hipLaunchKernelGGL(k_quantile_count, dim3(count_grid), dim3(256), 0, s, rec, n_records, st);
  hipLaunchKernelGGL(k_quantile_setup, dim3(1), dim3(64), 0, s, st, n_records, rs::ppm_of(q_ppm, n_q), n_q, d_out);
  const uint64_t per_wg = kHistThreads * kUnroll;
  const uint32_t hist_grid = (uint32_t)std::min<uint64_t>((n_records + per_wg - 1) / per_wg, kHistMaxGrid);
  for (int byte = 7; byte >= 0; --byte) {
    hipLaunchKernelGGL(k_quantile_hist, dim3(hist_grid), dim3(kHistThreads), 0, s, rec, n_records,
                       (const QState *)st, ghist, n_q, byte);
    hipLaunchKernelGGL(k_quantile_resolve, dim3(1), dim3(kResolveThreads), 0, s, st, ghist, n_q, byte, d_out);
  }
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int isim_latency_quantiles(int device, const isim_trace_rec *h_records, uint64_t n_records, const uint32_t *q_ppm,
                           uint32_t n_q, uint64_t *h_out) {
  if (const int rc = check_q(q_ppm, n_q, n_records)) return rc;
  if (!h_out || (n_records && !h_records)) return qfail("null argument");
  const uint64_t wsb = workspace_bytes(n_q), out_bytes = ISIM_Q_OUT_WORDS(n_q) * 8;
  isim::HostStage stage(device);
  void *d_ws = stage.alloc(wsb), *d_out = stage.alloc(out_bytes);
  void *d_rec = stage.upload(h_records, n_records * sizeof(isim_trace_rec));
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_latency_quantiles_device((const isim_trace_rec *)d_rec, n_records, q_ppm, n_q,
                                                   (uint64_t *)d_out, d_ws, wsb, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, out_bytes);
}

}  // extern "C"
