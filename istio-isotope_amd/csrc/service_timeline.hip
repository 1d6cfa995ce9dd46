// Service timeline on the device (service_timeline.h).
//
// isim_service_timeline_device: three kernels on the caller's stream, no host
// synchronisation.  k_svt_zero clears the two cover-difference planes of the
// workspace.  k_svt_fold takes one span per lane, grid-stride over a grid sized
// from cap_spans; the span count is read on the device from what the tap wrote.
// svt::span_updates turns the span into cells and values; spans come in trace
// order and arrivals in id order, so the lanes of a wave mostly hit one
// (service, row) cell: equal cells add up in the wave first (wave_peel.h, keyed
// on the cell) and one lane issues the atomic; the lanes left alone issue their
// own.  An interval's interior rows are never walked: +1 and -1 in the cover
// differences.  k_svt_finish, one workgroup per (service, plane), turns the
// differences into covers with a prefix sum along the rows (wave scans, the wave
// totals through LDS, a carry from tile to tile) and adds cover x window.
#include <hip/hip_runtime.h>

#include <string>

#include "hip_check.h"
#include "host_stage.h"
#include "service_timeline.h"
#include "spans.h"
#include "wave_peel.h"

namespace isim {
namespace svt {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 2048;  // 8 workgroups on each of 256 CUs
constexpr uint32_t kPeel = 4;          // shared cells a wave adds up per update before the rest go singly
constexpr uint32_t kScan = 1024;       // threads, and rows per tile, of the finish

struct FK {
  const uint64_t *off, *info;
  const isim_des_span *spans;
  uint64_t cap;
  unsigned long long *table, *cover;  // cover: [2][cells]
  const uint64_t *hold;
  uint64_t cells;
  uint32_t n_services;
  // the row fields of timeline_row.h
  uint64_t t0, window, recip;
  uint32_t n_windows, shift, pow2;
};

__device__ __forceinline__ bool is_lead(int lead) { return (int)(threadIdx.x & 63u) == lead; }

// word[addr(key)] += v per lane (kNone: no update), equal keys added up in the wave first
template <typename Addr>
__device__ __forceinline__ void wave_add(uint32_t key, uint64_t v, Addr addr) {
  dev::wave_peel<kPeel>(
      key, kNone,
      [&](uint32_t k0, unsigned long long, int lead) {
        const uint64_t sum = dev::wave_reduce<dev::OpAdd>(key == k0 ? v : 0);
        if (is_lead(lead) && sum) atomicAdd(addr(k0), (unsigned long long)sum);
      },
      [&](uint32_t k) {
        if (v) atomicAdd(addr(k), (unsigned long long)v);
      });
}

// word[addr(key)] += 1 per lane
template <typename Addr>
__device__ __forceinline__ void wave_count(uint32_t key, Addr addr) {
  dev::wave_peel<kPeel>(
      key, kNone,
      [&](uint32_t k0, unsigned long long m, int lead) {
        if (is_lead(lead)) atomicAdd(addr(k0), (unsigned long long)__popcll(m));
      },
      [&](uint32_t k) { atomicAdd(addr(k), 1ull); });
}

__global__ void __launch_bounds__(kThreads) k_svt_zero(unsigned long long *cover, uint64_t words) {
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += (uint64_t)gridDim.x * kThreads)
    cover[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_svt_fold(FK k) {
  const uint64_t end = k.off[k.info[ISIM_SPAN_WRITTEN]];
  const uint64_t n = end < k.cap ? end : k.cap;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  unsigned long long *const table = k.table;
  const auto word = [table](uint32_t w) {
    return [table, w](uint32_t cell) { return table + (uint64_t)cell * kW + w; };
  };
  uint64_t folded = 0, refused = 0;
  // every wave takes 64 consecutive spans per step; the bound is the same for all its lanes
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t i = base + lane;
    Upd u;
    if (i < n) {
      const isim_des_span &s = k.spans[i];
      u = span_updates(k, k.n_services, k.hold, s.arrival_ns, s.start_ns, s.finish_ns, s.service, s.status);
      if (u.ka == kNone) ++refused;
      else ++folded;
    }
    wave_count(u.ka, word(ISIM_SVT_ARRIVED));
    // STARTED, SUM_WAIT and MAX_WAIT of the start's cell in one peel
    dev::wave_peel<kPeel>(
        u.ks, kNone,
        [&](uint32_t k0, unsigned long long m, int lead) {
          const bool mine = u.ks == k0;
          const uint64_t sum = dev::wave_reduce<dev::OpAdd>(mine ? u.wait : 0);
          const uint64_t mx = dev::wave_reduce<dev::OpMax>(mine ? u.wait : 0);
          if (is_lead(lead)) {
            unsigned long long *row = table + (uint64_t)k0 * kW;
            atomicAdd(row + ISIM_SVT_STARTED, (unsigned long long)__popcll(m));
            if (sum) atomicAdd(row + ISIM_SVT_SUM_WAIT, (unsigned long long)sum);
            if (mx) atomicMax(row + ISIM_SVT_MAX_WAIT, (unsigned long long)mx);
          }
        },
        [&](uint32_t c) {
          unsigned long long *row = table + (uint64_t)c * kW;
          atomicAdd(row + ISIM_SVT_STARTED, 1ull);
          if (u.wait) {
            atomicAdd(row + ISIM_SVT_SUM_WAIT, (unsigned long long)u.wait);
            atomicMax(row + ISIM_SVT_MAX_WAIT, (unsigned long long)u.wait);
          }
        });
    // FINISHED by code: the key is cell * 2 + code
    wave_count(u.kf == kNone ? kNone : u.kf * 2u + u.code,
               [table](uint32_t key) { return table + (uint64_t)(key >> 1) * kW + ISIM_SVT_FINISHED + (key & 1u); });
    // the two intervals: head, tail, and the cover differences of the interior
    const Interval *iv[2] = {&u.q, &u.b};
#pragma unroll
    for (uint32_t p = 0; p < 2; ++p) {
      const Interval &v = *iv[p];
      unsigned long long *cover = k.cover + p * k.cells;
      const auto cov = [cover](uint32_t cell) { return cover + cell; };
      wave_add(v.k0, v.head, word(p ? ISIM_SVT_BUSY_NS : ISIM_SVT_QUEUED_NS));
      wave_add(v.k1, v.tail, word(p ? ISIM_SVT_BUSY_NS : ISIM_SVT_QUEUED_NS));
      wave_add(v.c0, 1ull, cov);
      wave_add(v.c1, ~0ull, cov);  // -1 mod 2^64
    }
  }
  // the header: one add per wave and word
  folded = dev::wave_reduce<dev::OpAdd>(folded);
  refused = dev::wave_reduce<dev::OpAdd>(refused);
  if (lane == 0) {
    if (folded) atomicAdd(table + k.cells * kW + ISIM_SVT_H_FOLDED, (unsigned long long)folded);
    if (refused) atomicAdd(table + k.cells * kW + ISIM_SVT_H_REFUSED, (unsigned long long)refused);
  }
}

// One workgroup per (service, plane): cover[r] = the sum of the differences of the rows <= r.
__global__ void __launch_bounds__(kScan) k_svt_finish(const unsigned long long *cover, unsigned long long *table,
                                                      uint64_t cells, uint32_t rows, uint64_t window) {
  __shared__ uint64_t s_wave[kScan / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t plane = blockIdx.y, w = plane ? ISIM_SVT_BUSY_NS : ISIM_SVT_QUEUED_NS;
  const uint64_t base = (uint64_t)blockIdx.x * rows;
  const unsigned long long *diff = cover + plane * cells + base;
  uint64_t carry = 0;
  for (uint32_t r0 = 0; r0 < rows; r0 += kScan) {  // the same for every thread
    const uint32_t r = r0 + t;
    uint64_t v = r < rows ? diff[r] : 0;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t o = __shfl_up((unsigned long long)v, d, 64);
      if (lane >= d) v += o;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint64_t before = carry, total = 0;
#pragma unroll
    for (uint32_t x = 0; x < kScan / 64; ++x) {
      const uint64_t sx = s_wave[x];
      total += sx;
      if (x < wave) before += sx;
    }
    const uint64_t c = before + v;
    if (r < rows && c) atomicAdd(table + (base + r) * kW + w, (unsigned long long)(c * window));
    carry += total;
    __syncthreads();
  }
}

}  // namespace

int launch(const isim_handler *h, const isim_timeline_params &p, const uint64_t *d_off, const isim_des_span *d_spans,
           uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_table, void *d_workspace, void *stream) {
  if (cap_spans == 0) return ISIM_OK;  // no span, no add
  hipStream_t s = (hipStream_t)stream;
  const spans::HandlerView v = spans::handler_view(h);
  spans::DevTables t;
  if (const int rc = spans::device_tables(v, t)) return rc;
  FK k{};
  k.off = d_off;
  k.info = d_info;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.table = (unsigned long long *)d_table;
  k.cover = (unsigned long long *)d_workspace;
  k.hold = t.svc_hold;
  k.n_services = (uint32_t)v.graph->services.size();
  k.cells = cells_of(k.n_services, p.n_windows);
  tl::set_row_args(k, p);
  const uint64_t words = 2 * k.cells;
  const uint64_t zb = (words + kThreads - 1) / kThreads, fb = (cap_spans + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_svt_zero, dim3((uint32_t)(zb < kMaxBlocks ? zb : kMaxBlocks)), dim3(kThreads), 0, s, k.cover,
                     words);
  hipLaunchKernelGGL(k_svt_fold, dim3((uint32_t)(fb < kMaxBlocks ? fb : kMaxBlocks)), dim3(kThreads), 0, s, k);
  hipLaunchKernelGGL(k_svt_finish, dim3(k.n_services, 2), dim3(kScan), 0, s, k.cover, k.table, k.cells,
                     p.n_windows + 2u, p.window_ns);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace svt
}  // namespace isim

namespace {
namespace svt = isim::svt;
namespace sp = isim::spans;
int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service timeline: " + msg); }

}  // namespace

extern "C" {

int isim_service_timeline_device(const isim_handler *h, const isim_timeline_params *p, const uint64_t *d_off,
                                 const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
                                 uint64_t *d_table, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (cap_spans > svt::kMaxSpans) return sfail("cap_spans is above 2^40");
  if (!d_off || !d_info || !d_table) return sfail("null offsets, info or table");
  if (cap_spans && !d_spans) return sfail("null spans with cap_spans > 0");
  if ((((uintptr_t)d_off | (uintptr_t)d_info | (uintptr_t)d_table | (uintptr_t)d_workspace) & 7u) ||
      ((uintptr_t)d_spans & 15u))
    return sfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (cap_spans && (!d_workspace || workspace_bytes < svt::ws_bytes(cells)))
    return sfail("the workspace is smaller than isim_service_timeline_workspace_bytes()");
  return svt::launch(h, *p, d_off, d_spans, cap_spans, d_info, d_table, d_workspace, hip_stream);
}

int isim_service_timeline(int device, const isim_handler *h, const isim_timeline_params *p,
                          const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_table) {
  uint64_t cells = 0;
  if (const int rc = svt::check(h, p, cells)) return rc;
  if (n_spans > svt::kMaxSpans) return sfail("n_spans is above 2^40");
  if (!h_table) return sfail("null table");
  if (n_spans && !h_spans) return sfail("null spans");
  if (n_spans == 0) return ISIM_OK;
  // the tap's offsets and info of one list entry that holds every span
  const uint64_t off[2] = {0, n_spans};
  const uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {n_spans, 1, 1, 1, 1};
  const uint64_t bytes = svt::table_words(cells) * 8, ws_bytes = svt::ws_bytes(cells);
  isim::HostStage stage(device);
  void *d_table = stage.upload(h_table, bytes);  // added into: it goes up first
  void *d_off = stage.upload(off, sizeof off), *d_info = stage.upload(info, sizeof info);
  void *d_spans = stage.upload(h_spans, n_spans * sizeof(isim_des_span)), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_service_timeline_device(h, p, (const uint64_t *)d_off, (const isim_des_span *)d_spans,
                                                  n_spans, (const uint64_t *)d_info, (uint64_t *)d_table, d_ws,
                                                  ws_bytes, stage.stream()))
    return rc;
  return stage.download(h_table, d_table, bytes);
}

}  // extern "C"
