// Per-service percentiles over time on the device (service_window_quantiles.h,
// DESIGN.md §29): a segmented select over the three measures of the tapped
// spans, a segment per cell (service, timeline row of the finish time).
//
// isim_service_window_quantiles_device: a fixed sequence of kernels on the
// caller's stream, no host synchronisation, no workgroup waits for another.
//   k_svq_clear    the head, the counts and the table's header
//   k_svq_count    spans per (cell, code), wave-aggregated; folded / refused
//   k_swq_scan     one workgroup, kScanPer cells per thread and tile: segment
//                  offsets and cursors; the cells of the LDS tier listed, the
//                  long ones numbered into slots (span_segments.h)
//   k_svq_scatter  the three measures of a span to its segment, three arrays
//   k_swq_wave     a wave per cell, striding: an empty cell gets its zeros, a
//                  segment of at most kWave spans is ranked in registers
//   k_swq_lds      a workgroup claims a listed cell by ticket and selects it
//                  in LDS, once per measure (segmented_select.h)
//   k_svq_long_*   the long segments' launches (span_segments.h)
// Most cells of a million are empty or hold a few dozen spans: the wave tier
// takes them without bins, digit passes or LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hip_check.h"
#include "host_stage.h"
#include "service_window_quantiles.h"
#include "span_segments.h"

namespace isim {
namespace swq {
namespace {

namespace rs = isim::rs;
using rs::kBins;
using rs::kMaxQ;
using rs::kSelThreads;
using rs::kUnroll;
using svq::Head;
using svq::kThreads;
using svq::SelArgs;
using svq::SK;
using svq::Slot;

constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanPer = 8;  // cells per thread and tile: 2^20 cells are 128 tiles
constexpr uint32_t kKpl = kWave / 64;  // keys per lane of the wave tier
constexpr uint32_t kWaveMaxGrid = 4096;  // workgroups of four waves
constexpr uint32_t kMidWord = 16;  // the u32 word of the head that counts the listed cells
static_assert(sizeof(Head) <= kMidWord * 4 && (kMidWord + 1) * 4 <= svq::kHeadBytes, "the head's words do not meet");
static_assert(2 * kMaxCells < kNone, "a key is not kNone");

// the key of a span that is not refused: 2 * cell + code, the row being that of the finish time
struct CellKey {
  RowArgs row;
  __device__ __forceinline__ uint32_t operator()(uint32_t svc, uint32_t status, uint64_t finish) const {
    return cell_at(row, svc, finish) * 2u + (status & 1u);
  }
};

// One workgroup: the exclusive scan of the counts into the segment offsets and the scatter cursors, kScanPer
// consecutive cells per thread and tile.  The cells of the LDS tier go to the list, the long ones get a slot
// each, in cell order, and the first of their chunks.  The counts are of at most cap spans, so no more than
// n_mid_max cells are listed and no more than n_slots are long.
__global__ __launch_bounds__(kScanThreads) void k_swq_scan(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off,
                                                          uint32_t *__restrict__ cur, uint32_t n_cells, Slot *slots,
                                                          uint32_t n_slots, uint32_t *__restrict__ mid,
                                                          uint32_t n_mid_max, Head *head) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t c_elem = 0, c_long = 0, c_chunk = 0, c_mid = 0;
  for (uint32_t tile = 0; tile < n_cells; tile += kScanThreads * kScanPer) {
    const uint32_t first = tile + t * kScanPer;
    uint32_t n200[kScanPer], n500[kScanPer];
    uint32_t elem = 0, longs = 0, chunks = 0, mids = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
      const bool live = first + j < n_cells;
      n200[j] = live ? cnt[2 * (first + j)] : 0u;
      n500[j] = live ? cnt[2 * (first + j) + 1] : 0u;
      const uint32_t n = n200[j] + n500[j];
      elem += n;
      longs += n > kStage ? 1u : 0u;
      chunks += n > kStage ? (n - 1) / svq::kChunk + 1 : 0u;
      mids += n > kWave && n <= kStage ? 1u : 0u;
    }
    uint32_t t_elem, t_long, t_chunk, t_mid;
    uint32_t e = c_elem + rs::block_scan<kScanThreads>(elem, s_wave, lane, wave, t_elem);
    uint32_t l = c_long + rs::block_scan<kScanThreads>(longs, s_wave, lane, wave, t_long);
    uint32_t c = c_chunk + rs::block_scan<kScanThreads>(chunks, s_wave, lane, wave, t_chunk);
    uint32_t m = c_mid + rs::block_scan<kScanThreads>(mids, s_wave, lane, wave, t_mid);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
      const uint32_t s = first + j;
      if (s >= n_cells) break;
      const uint32_t n = n200[j] + n500[j];
      off[2 * s] = cur[2 * s] = e;
      off[2 * s + 1] = cur[2 * s + 1] = e + n200[j];
      if (n > kStage) {
        if (l < n_slots) {
          Slot &x = slots[l];
          x.svc = s;
          x.chunk0 = c;
          x.n200 = n200[j];
          x.n500 = n500[j];
          x.off = e;
          for (uint32_t k = 0; k < kMeasures; ++k) x.any[k] = 0;
        }
        l += 1;
        c += (n - 1) / svq::kChunk + 1;
      } else if (n > kWave) {
        if (m < n_mid_max) mid[m] = s;
        m += 1;
      }
      e += n;
    }
    c_elem += t_elem;
    c_long += t_long;
    c_chunk += t_chunk;
    c_mid += t_mid;
  }
  if (t == 0) {
    const bool fits = c_long <= n_slots;  // always, for counts of at most cap spans
    head->n_long = fits ? c_long : 0u;
    head->n_chunks = fits ? c_chunk : 0u;
    ((uint32_t *)head)[kMidWord] = c_mid <= n_mid_max ? c_mid : 0u;  // likewise
  }
}

struct WArgs {
  SelArgs a;
  const uint32_t *mid;  // the listed cells
};

__device__ __forceinline__ uint64_t read_lane(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void zero_cell(unsigned long long *out, uint32_t words, uint32_t lane) {
  for (uint32_t w = lane; w < words; w += 64) out[w] = 0;
}

// The wave tier.  A wave takes cells, striding; everything below is wave-uniform but the keys and their ranks.
// An empty cell gets its zeros; a cell of more than kWave spans is another kernel's, unless its counts are not
// of these spans (the spans changed under the call) and have left that kernel nothing: zeros then, so that
// every word of the table is written.  Otherwise element p = j * 64 + lane of the segment sits in lane's
// register j, all three measures of it, and every element q is read across the wave once: p's rank among all
// and among its class counts the elements below it, ties broken by position, so the ranks are a permutation
// and the lane whose rank is a wanted k - 1 holds the k-th smallest value.
__global__ __launch_bounds__(kThreads) void k_swq_wave(WArgs w) {
  const SelArgs &a = w.a;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n_waves = gridDim.x * (kThreads / 64), ow = 1u + a.n_q, cw = kMeasures * kClasses * ow;
  const uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6));
  for (uint32_t cell = first; cell < a.n_services; cell += n_waves) {
    const uint32_t n200 = __builtin_amdgcn_readfirstlane(a.cnt[2 * cell]);
    const uint32_t n500 = __builtin_amdgcn_readfirstlane(a.cnt[2 * cell + 1]);
    const uint32_t n = n200 + n500;
    unsigned long long *out = a.out + (uint64_t)cell * cw;
    if (n == 0) {
      zero_cell(out, cw, lane);
      continue;
    }
    const uint64_t off = __builtin_amdgcn_readfirstlane(a.off[2 * cell]);
    const bool astray = n > kStage  ? a.head->n_long == 0
                        : n > kWave ? ((const uint32_t *)a.head)[kMidWord] == 0
                                    : off + n > a.cap;
    if (astray) zero_cell(out, cw, lane);
    if (n > kWave || astray) continue;

    uint64_t v[kMeasures][kKpl];
    uint32_t r[kMeasures][kKpl];  // the rank among all, and << 16 the rank among the class
#pragma unroll
    for (uint32_t j = 0; j < kKpl; ++j) {
      const uint32_t p = j * 64 + lane;
#pragma unroll
      for (uint32_t m = 0; m < kMeasures; ++m) {
        v[m][j] = p < n ? a.seg[m * a.cap + off + p] : 0;
        r[m][j] = 0;
      }
    }
#pragma unroll
    for (uint32_t jq = 0; jq < kKpl; ++jq) {
      if (jq * 64 >= n) break;
      const int n_l = (int)min(64u, n - jq * 64);
      for (int l = 0; l < n_l; ++l) {
        const uint32_t q = jq * 64 + (uint32_t)l;
        const bool q200 = q < n200;
        uint64_t x[kMeasures];
#pragma unroll
        for (uint32_t m = 0; m < kMeasures; ++m) x[m] = read_lane(v[m][jq], l);
#pragma unroll
        for (uint32_t j = 0; j < kKpl; ++j) {
          if (j * 64 >= n) break;
          const uint32_t p = j * 64 + lane;
          const uint32_t one = (p < n200) == q200 ? 0x10001u : 1u;
#pragma unroll
          for (uint32_t m = 0; m < kMeasures; ++m) {
            const bool below = q < p ? x[m] <= v[m][j] : x[m] < v[m][j];
            r[m][j] += below ? one : 0u;
          }
        }
      }
    }
    // the counts, and the zeros of an empty class
    for (uint32_t i = lane; i < cw; i += 64) {
      const uint32_t c = (i / ow) % kClasses, word = i % ow;
      const uint32_t n_c = c == ISIM_Q_ALL ? n : c == ISIM_Q_200 ? n200 : n500;
      if (word == 0) out[i] = n_c;
      else if (n_c == 0) out[i] = 0;
    }
    for (uint32_t c = 0; c < kClasses; ++c) {
      const uint32_t n_c = c == ISIM_Q_ALL ? n : c == ISIM_Q_200 ? n200 : n500;
      if (n_c == 0) continue;
      for (uint32_t i = 0; i < a.n_q; ++i) {
        const uint32_t k = (uint32_t)isim::q::nearest_rank(n_c, a.ppm.v[i]) - 1u;
#pragma unroll
        for (uint32_t j = 0; j < kKpl; ++j) {
          if (j * 64 >= n) break;
          const uint32_t p = j * 64 + lane;
          const bool mine = p < n && (c == ISIM_Q_ALL || (p < n200) == (c == ISIM_Q_200));
#pragma unroll
          for (uint32_t m = 0; m < kMeasures; ++m) {
            const uint32_t rank = c == ISIM_Q_ALL ? r[m][j] & 0xFFFFu : r[m][j] >> 16;
            if (mine && rank == k) out[(m * kClasses + c) * ow + 1 + i] = v[m][j];
          }
        }
      }
    }
  }
}

// The LDS tier.  A workgroup claims entries of the list through the ticket until none is left; per measure
// the segment is staged in LDS and selected there (segmented_select.h); the ticket is s.sel.owner_word.  A
// listed cell whose segment is not inside the arrays (counts not of these spans) gets zeros.
__global__ __launch_bounds__(kSelThreads) void k_swq_lds(WArgs w) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[kClasses * kMaxQ * kBins];
  __shared__ unsigned long long s_stage[kStage];
  __shared__ rs::SelState s;
  const SelArgs &a = w.a;
  const uint32_t t = threadIdx.x, ow = 1u + a.n_q;
  const uint32_t n_mid = ((const uint32_t *)a.head)[kMidWord];
  for (;;) {
    __syncthreads();  // the previous segment's state has been read
    if (t == 0) s.sel.owner_word = atomicAdd(&a.head->ticket, 1u);
    __syncthreads();
    const uint32_t at = s.sel.owner_word;
    if (at >= n_mid) return;  // workgroup-uniform
    const uint32_t cell = w.mid[at];
    if (cell >= a.n_services) continue;
    const uint32_t n200 = a.cnt[2 * cell], n500 = a.cnt[2 * cell + 1];
    const uint32_t n_seg = n200 + n500;
    const uint64_t off = a.off[2 * cell];
    unsigned long long *out = a.out + (uint64_t)cell * kMeasures * kClasses * ow;
    if (n_seg <= kWave || n_seg > kStage) continue;  // never for a listed cell
    if (off + n_seg > a.cap) {
      for (uint32_t i = t; i < kMeasures * kClasses * ow; i += kSelThreads) out[i] = 0;
      continue;
    }
    for (uint32_t m = 0; m < kMeasures; ++m) {
      __syncthreads();  // the previous measure's state has been read
      rs::select_segment<true>(hist, s_stage, s, a.seg + m * a.cap + off, n_seg, n200, true, a.n_q, a.ppm,
                               out + (uint64_t)m * kClasses * ow);
    }
  }
}

}  // namespace

int launch(uint32_t n_services, const isim_timeline_params &p, const uint32_t *q_ppm, uint32_t n_q,
           const uint64_t *d_off, const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
           uint64_t *d_out, void *d_workspace, void *stream) {
  const hipStream_t s = (hipStream_t)stream;
  const uint64_t cells = cells_of(n_services, p.n_windows);
  const uint64_t words = table_words(cells, n_q);
  if (cap_spans == 0) {  // no span: zeros
    hipLaunchKernelGGL(svq::k_svq_clear, dim3(rs::grid_for(2 * words, kThreads * 4, svq::kMaxGrid)), dim3(kThreads), 0,
                       s, (uint32_t *)d_out, 2 * words, (uint32_t *)nullptr, (uint64_t)0);
    ISIM_HIPCHK(hipGetLastError());
    return ISIM_OK;
  }
  const Layout l = layout(cells, cap_spans, n_q);
  char *ws = (char *)d_workspace;
  SK k{};
  k.off = d_off;
  k.info = d_info;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.n_services = n_services;
  k.cnt = (uint32_t *)(ws + l.cnt);
  k.cur = (uint32_t *)(ws + l.cur);
  k.seg = (unsigned long long *)(ws + l.seg);
  k.hdr = (unsigned long long *)d_out + (words - ISIM_SVQ_HEADER_WORDS);
  CellKey key{};
  tl::set_row_args(key.row, p);
  WArgs w{};
  SelArgs &a = w.a;
  a.cnt = k.cnt;
  a.off = (const uint32_t *)(ws + l.off);
  a.seg = k.seg;
  a.cap = cap_spans;
  a.head = (Head *)ws;
  a.slots = (Slot *)(ws + l.slots);
  a.bins = (uint32_t *)(ws + l.bins);
  a.out = (unsigned long long *)d_out;
  a.n_services = (uint32_t)cells;
  a.n_q = n_q;
  a.n_slots = (uint32_t)l.n_slots;
  a.ppm = rs::ppm_of(q_ppm, n_q);
  w.mid = (const uint32_t *)(ws + l.mid);

  // the head and the counts, contiguous from the workspace's start, and the table's header (every clear is a kernel)
  const uint64_t clear_words = l.cnt / 4 + l.counters;
  hipLaunchKernelGGL(svq::k_svq_clear, dim3(rs::grid_for(clear_words, kThreads * 4, svq::kMaxGrid)), dim3(kThreads), 0,
                     s, (uint32_t *)ws, clear_words, (uint32_t *)k.hdr, (uint64_t)2 * ISIM_SVQ_HEADER_WORDS);
  const uint32_t grid = rs::grid_for(cap_spans, kThreads * kUnroll, svq::kMaxGrid);
  hipLaunchKernelGGL(svq::k_svq_count<CellKey>, dim3(grid), dim3(kThreads), 0, s, k, key);
  hipLaunchKernelGGL(k_swq_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)k.cnt, (uint32_t *)(ws + l.off),
                     k.cur, (uint32_t)cells, a.slots, a.n_slots, (uint32_t *)(ws + l.mid), (uint32_t)l.n_mid, a.head);
  hipLaunchKernelGGL(svq::k_svq_scatter<CellKey>, dim3(grid), dim3(kThreads), 0, s, k, key);
  hipLaunchKernelGGL(k_swq_wave, dim3(rs::grid_for(cells, kThreads / 64, kWaveMaxGrid)), dim3(kThreads), 0, s, w);
  if (l.n_mid)  // cap_spans allows a segment of the LDS tier: the launch is issued whatever the spans are
    hipLaunchKernelGGL(k_swq_lds, dim3((uint32_t)std::min<uint64_t>(l.n_mid, svq::kSelMaxGrid)), dim3(kSelThreads), 0, s,
                       w);
  svq::launch_long(a, cap_spans, s);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace swq
}  // namespace isim

namespace {
namespace swq = isim::swq;
int wfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "service window quantiles: " + msg); }

}  // namespace

extern "C" {

int isim_service_window_quantiles_device(const isim_handler *h, const isim_timeline_params *p, const uint32_t *q_ppm,
                                         uint32_t n_q, const uint64_t *d_off, const isim_des_span *d_spans,
                                         uint64_t cap_spans, const uint64_t *d_info, uint64_t *d_out,
                                         void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  uint64_t ns = 0, cells = 0;
  if (const int rc = swq::check(h, p, q_ppm, n_q, true, cap_spans, ns, cells)) return rc;
  if (!d_off || !d_info || !d_out) return wfail("null offsets, info or table");
  if (cap_spans && !d_spans) return wfail("null spans with cap_spans > 0");
  if ((((uintptr_t)d_off | (uintptr_t)d_info | (uintptr_t)d_out | (uintptr_t)d_workspace) & 7u) ||
      ((uintptr_t)d_spans & 15u))
    return wfail("the buffers must be 8-byte aligned, the spans 16-byte aligned");
  if (cap_spans && (!d_workspace || workspace_bytes < swq::layout(cells, cap_spans, n_q).total))
    return wfail("the workspace is smaller than isim_service_window_quantiles_workspace_bytes()");
  return swq::launch((uint32_t)ns, *p, q_ppm, n_q, d_off, d_spans, cap_spans, d_info, d_out, d_workspace, hip_stream);
}

int isim_service_window_quantiles(int device, const isim_handler *h, const isim_timeline_params *p,
                                  const uint32_t *q_ppm, uint32_t n_q, const isim_des_span *h_spans, uint64_t n_spans,
                                  uint64_t *h_out) {
  uint64_t ns = 0, cells = 0;
  if (const int rc = swq::check(h, p, q_ppm, n_q, true, n_spans, ns, cells)) return rc;
  if (!h_out) return wfail("null table");
  if (n_spans && !h_spans) return wfail("null spans");
  // the tap's offsets and info of one list entry that holds every span
  const uint64_t off[2] = {0, n_spans};
  const uint64_t info[ISIM_DES_SPAN_INFO_WORDS] = {n_spans, 1, 1, 1, 1};
  const uint64_t bytes = swq::table_words(cells, n_q) * 8;
  const uint64_t ws_bytes = n_spans ? swq::layout(cells, n_spans, n_q).total : 0;
  isim::HostStage stage(device);
  void *d_out = stage.alloc(bytes);
  void *d_off = stage.upload(off, sizeof off), *d_info = stage.upload(info, sizeof info);
  void *d_spans = stage.upload(h_spans, n_spans * sizeof(isim_des_span)), *d_ws = stage.alloc(ws_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_service_window_quantiles_device(
          h, p, q_ppm, n_q, (const uint64_t *)d_off, (const isim_des_span *)d_spans, n_spans, (const uint64_t *)d_info,
          (uint64_t *)d_out, d_ws, ws_bytes, stage.stream()))
    return rc;
  return stage.download(h_out, d_out, bytes);
}

}  // extern "C"
