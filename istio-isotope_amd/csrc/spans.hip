// Trace spans on the device (spans.h).
//
// isim_trace_spans_device: three steps ordered by the stream, no workgroup ever
// waits for another.
//   1. count   one trace per lane (tw::Lane, a sink that records nothing); a
//              lane whose trace has responded takes the next entry of its
//              wave's batch of 64 LIST ENTRIES, the wave claiming batches from
//              a counter as it runs dry (the pre-walk's refill, des_items.hip);
//              cnt[i] = hops
//   2. scan    cnt -> d_off (exclusive): tile sums, one workgroup over the tile
//              sums (it also writes d_info), the tiles again
//   3. emit    the same walks with the SpanSink: one isim_span per close at
//              d_spans[d_off[i] + hop], the entry's once the trace has
//              responded; a trace whose range ends past cap_spans is not walked
// The walks draw the errors in both modes (the spans carry statuses); mode A's
// counting pass alone drops them, since no error changes which calls run.
// Nodes are read from global memory; the spill columns of a deep tree lie in
// the caller's workspace, so two streams never share frames.
//
// isim_select_traces_device: count per tile, the same scan, scatter.  A tile is
// 1024 records, thread t taking records t, t + 256, ...: the rank of a match in
// its tile follows from 16 wave ballots, so the ids come out in ascending order.
#include <hip/hip_runtime.h>

#include <map>
#include <type_traits>

#include "hip_check.h"
#include "host_stage.h"
#include "critical_path.h"
#include "des.h"
#include "spans.h"
#include "trace_rec_dev.h"

namespace isim {
namespace spans {
namespace {

struct GNodes {
  const unsigned long long *__restrict__ p;
  __device__ __forceinline__ tw::NodeW load(uint32_t i) const {
    const unsigned long long v = p[i];
    return tw::NodeW{(uint32_t)v, (uint32_t)(v >> 32)};
  }
};
struct GNodesW {
  const uint4 *__restrict__ p;
  __device__ __forceinline__ tw::NodeW4 load(uint32_t i) const {
    const uint4 v = p[i];
    return tw::NodeW4{v.x, v.y, v.z, v.w};
  }
};

struct WK {
  const uint64_t *ids;
  uint64_t n;
  const void *nodes;
  const TreeExt *ext;
  const TreeStep *step;
  const uint32_t *slot_callee;
  uint32_t *cnt;        // count: hops per list entry
  const uint64_t *off;  // emit: [n + 1]
  isim_span *spans;
  uint64_t cap;
  uint32_t *spill;
  uint32_t entry, k0, k1;
};

template <int FR, bool SPILL, bool EMIT, bool T64, bool MB, bool W>
__global__ void __launch_bounds__(kT) k_span_walk(WK k, unsigned long long *work) {
  using Nodes = std::conditional_t<W, GNodesW, GNodes>;
  const Nodes nodes{(decltype(Nodes::p))k.nodes};
  tw::Lane<FR, MB, true, SPILL, EMIT || MB, std::conditional_t<T64, uint64_t, uint32_t>, W> L;
  if constexpr (SPILL) {
    L.sp = k.spill + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    L.sp_stride = gridDim.x * blockDim.x;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint64_t nxt = 0, lim = 0;
  bool dry = false, active = false;
  uint64_t i = 0;
  SpanSink<MB, Nodes> s;
  s.nodes = nodes;
  s.ext = k.ext;
  s.slot_callee = k.slot_callee;
  s.entry = k.entry;
  s.k0 = k.k0;
  s.k1 = k.k1;
  NoStats cs;
  while (true) {
    if (active && L.done) {
      if constexpr (EMIT) s.entry_span((uint64_t)L.lat, L.root500);
      else k.cnt[i] = L.hops();
      active = false;
    }
    unsigned long long idle = __ballot(!active);
    while (idle && !dry) {
      if (nxt >= lim) {
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(work, 1ull);
        b = __shfl(b, 0, 64);
        if (b * 64 >= k.n) {
          dry = true;
          break;
        }
        nxt = b * 64;
        lim = nxt + 64 < k.n ? nxt + 64 : k.n;
      }
      const uint32_t rank = (uint32_t)__popcll(idle & lt);
      const bool take = ((idle >> lane) & 1ull) && rank < lim - nxt;
      if (take) {
        i = nxt + rank;
        bool walk = true;
        if constexpr (EMIT) walk = k.off[i + 1] <= k.cap;  // a trace that does not fit writes nothing
        if (walk) {
          const uint64_t id = k.ids[i];
          active = true;
          L.start(id);
          if constexpr (EMIT) s.begin(id, k.spans + k.off[i]);
        }
      }
      const unsigned long long took = __ballot(take);
      nxt += (uint64_t)__popcll(took);
      idle &= ~took;
    }
    if (!__ballot(active)) break;
    if (active && !L.done) {
      if constexpr (EMIT) L.step(nodes, k.ext, k.step, s, k.k0, k.k1);
      else L.step(nodes, k.ext, k.step, cs, k.k0, k.k1);
    }
  }
}

// the two batch counters of a call, by a kernel like every other step (a captured call is kernel nodes only)
__global__ void k_zero_work(unsigned long long *work) {
  if (threadIdx.x < 2) work[threadIdx.x] = 0;
}

// ---- the scan
__device__ __forceinline__ uint64_t wave_incl(uint64_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// exclusive prefix of v over the workgroup's threads (at most 16 waves) and the workgroup's total
__device__ __forceinline__ uint64_t block_excl(uint64_t v, uint64_t *wsum, uint64_t &total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t inc = wave_incl(v);
  __syncthreads();  // wsum may still be read from the previous use
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t base = 0, t = 0;
  for (uint32_t j = 0; j < nw; ++j) {
    const uint64_t x = wsum[j];
    base += j < w ? x : 0;
    t += x;
  }
  total = t;
  return base + inc - v;
}

__global__ void __launch_bounds__(kT) k_tile_sums(const uint32_t *__restrict__ cnt, uint64_t n, uint64_t *tile) {
  __shared__ uint64_t wsum[16];
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x * 4u;
  uint64_t v = 0;
  for (uint32_t j = 0; j < 4; ++j) v += base + j < n ? cnt[base + j] : 0u;
  uint64_t total;
  (void)block_excl(v, wsum, total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// one workgroup: tile[0 .. nt) to its exclusive scan, tile[nt] = the total; and what follows from the total:
// spans (end != nullptr): *end = total (d_off[n]), info = {total, n, n, n} (k_offsets corrects the last two
// where a trace does not fit); select: info = {total, min(total, a)}
__global__ void __launch_bounds__(1024) k_scan_tiles(uint64_t *tile, uint64_t nt, uint64_t *end, uint64_t *info,
                                                     uint64_t a) {
  __shared__ uint64_t wsum[16];
  uint64_t carry = 0;
  for (uint64_t c = 0; c < nt; c += 1024) {
    const uint64_t i = c + threadIdx.x;
    const uint64_t v = i < nt ? tile[i] : 0;
    uint64_t total;
    const uint64_t ex = block_excl(v, wsum, total);
    if (i < nt) tile[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    tile[nt] = carry;
    if (end) {
      *end = carry;
      info[ISIM_SPAN_TOTAL] = carry;
      info[ISIM_SPAN_WRITTEN] = a;
      info[ISIM_SPAN_N_IDS] = a;
      info[ISIM_SPAN_FIRST_UNFIT] = a;
    } else {
      info[0] = carry;
      info[1] = carry < a ? carry : a;
    }
  }
}

// off[i] = the exclusive scan of cnt; every trace has at least one hop, so the offsets ascend strictly and
// exactly one entry (if any) starts within cap and ends past it: the first that does not fit
__global__ void __launch_bounds__(kT) k_offsets(const uint32_t *__restrict__ cnt, uint64_t n,
                                                const uint64_t *__restrict__ tile, uint64_t *off, uint64_t cap,
                                                uint64_t *info) {
  __shared__ uint64_t wsum[16];
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x * 4u;
  uint32_t c[4];
  uint64_t v = 0;
  for (uint32_t j = 0; j < 4; ++j) {
    c[j] = base + j < n ? cnt[base + j] : 0u;
    v += c[j];
  }
  uint64_t total;
  uint64_t o = tile[blockIdx.x] + block_excl(v, wsum, total);
  for (uint32_t j = 0; j < 4; ++j) {
    if (base + j < n) {
      off[base + j] = o;
      if (o <= cap && o + c[j] > cap) {
        info[ISIM_SPAN_WRITTEN] = base + j;
        info[ISIM_SPAN_FIRST_UNFIT] = base + j;
      }
    }
    o += c[j];
  }
}

// ---- the selection
__device__ __forceinline__ bool sel_match(const dev::rec4 *rec, uint64_t i, uint64_t n, uint64_t min_latency,
                                          uint32_t cls) {
  const dev::rec4 r = dev::load_rec(rec, i, i < n);
  return i < n && selected(dev::latency(r), r.w, min_latency, cls);
}

__global__ void __launch_bounds__(kT) k_sel_count(const dev::rec4 *__restrict__ rec, uint64_t n, uint64_t min_latency,
                                                  uint32_t cls, uint64_t *tile) {
  __shared__ uint32_t wc[kT / 64];
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t c = 0;
  for (uint32_t j = 0; j < 4; ++j) c += (uint32_t)__popcll(__ballot(sel_match(rec, base + j * kT, n, min_latency, cls)));
  if ((threadIdx.x & 63u) == 0) wc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile[blockIdx.x] = (uint64_t)wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ void __launch_bounds__(kT) k_sel_scatter(const dev::rec4 *__restrict__ rec, uint64_t n, uint64_t trace_begin,
                                                    uint64_t min_latency, uint32_t cls, uint64_t max_ids,
                                                    const uint64_t *__restrict__ tile, uint64_t *ids) {
  __shared__ uint32_t wc[4][kT / 64];  // matches of row j (256 records) in wave w
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  unsigned long long m[4];
  for (uint32_t j = 0; j < 4; ++j) {
    m[j] = __ballot(sel_match(rec, base + j * kT, n, min_latency, cls));
    if (lane == 0) wc[j][w] = (uint32_t)__popcll(m[j]);
  }
  __syncthreads();
  uint64_t rank = tile[blockIdx.x];
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t before = 0, row = 0;
    for (uint32_t x = 0; x < kT / 64; ++x) {
      before += x < w ? wc[j][x] : 0u;
      row += wc[j][x];
    }
    if ((m[j] >> lane) & 1ull) {
      const uint64_t r = rank + before + (uint32_t)__popcll(m[j] & ((1ull << lane) - 1ull));
      if (r < max_ids) ids[r] = trace_begin + base + j * kT;
    }
    rank += row;
  }
}

// ---- the walk variant of a tree: register frames (8 + spill, 16, 8), time width, error mode, node width
using WalkFn = void (*)(WK, unsigned long long *);
template <int FR, bool SP, bool T6, bool MB>
WalkFn walk_variant(bool wide, bool emit) {
  static const WalkFn v[2][2] = {{k_span_walk<FR, SP, false, T6, MB, false>, k_span_walk<FR, SP, true, T6, MB, false>},
                                 {k_span_walk<FR, SP, false, T6, MB, true>, k_span_walk<FR, SP, true, T6, MB, true>}};
  return v[wide][emit];
}
WalkFn walk_kernel(Frames fr, bool t64, bool modeb, bool wide, bool emit) {
  static WalkFn (*const pick[3][2][2])(bool, bool) = {
      {{walk_variant<8, true, false, false>, walk_variant<8, true, false, true>},
       {walk_variant<8, true, true, false>, walk_variant<8, true, true, true>}},
      {{walk_variant<16, false, false, false>, walk_variant<16, false, false, true>},
       {walk_variant<16, false, true, false>, walk_variant<16, false, true, true>}},
      {{walk_variant<8, false, false, false>, walk_variant<8, false, false, true>},
       {walk_variant<8, false, true, false>, walk_variant<8, false, true, true>}}};
  return pick[fr][t64][modeb](wide, emit);
}

// ---- the handler's tables on a device (spans.h DevTables), kept in the handler (HandlerView::state) and freed
// with it
void free_tables(const DevTables &t) {
  for (void *q : {t.nodes, (void *)t.ext, (void *)t.step, (void *)t.slot_callee, (void *)t.cmd_off, (void *)t.cmds,
                  (void *)t.svc_hold})
    if (q) (void)hipFree(q);
}
struct State {
  std::map<int, DevTables> dev;
  ~State() {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto &kv : dev)
      if (hipSetDevice(kv.first) == hipSuccess) free_tables(kv.second);
    if (have) (void)hipSetDevice(cur);
  }
};

// An upload inside a stream capture is legal once the thread's capture mode is relaxed for its duration (the
// allocation and the copy are not part of the captured work): so the first call may be a captured one.
struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
  ~RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
};

int upload(void **dst, const void *src, size_t bytes, hipStream_t s) {
  ISIM_HIPCHK(hipMalloc(dst, bytes ? bytes : 1));
  if (bytes) ISIM_HIPCHK(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s));
  return ISIM_OK;
}

}  // namespace

int device_tables(const HandlerView &v, DevTables &out) {
  int device = 0;
  ISIM_HIPCHK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lk(*v.mu);
  if (!*v.state) *v.state = std::shared_ptr<void>(new State(), [](void *p) { delete (State *)p; });
  State &st = *(State *)v.state->get();
  auto it = st.dev.find(device);
  if (it != st.dev.end()) {
    out = it->second;
    return ISIM_OK;
  }
  const Program &p = *v.prog;
  const std::vector<uint32_t> callee(p.slot_callee.begin(), p.slot_callee.end());
  const cp::FlatScripts scripts = cp::flat_scripts(*v.graph);
  const std::vector<uint64_t> hold = des_service_holds(*v.graph);
  RelaxedCapture relaxed;
  hipStream_t s = nullptr;
  ISIM_HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  DevTables t;
  int rc = p.tree_wide ? upload(&t.nodes, p.tree_nodes_w.data(), p.tree_nodes_w.size() * sizeof(TreeNodeW), s)
                       : upload(&t.nodes, p.tree_nodes.data(), p.tree_nodes.size() * sizeof(TreeNode), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.ext, p.tree_ext.data(), p.tree_ext.size() * sizeof(TreeExt), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.step, p.tree_step.data(), p.tree_step.size() * sizeof(TreeStep), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.slot_callee, callee.data(), callee.size() * sizeof(uint32_t), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.cmd_off, scripts.cmd_off.data(), scripts.cmd_off.size() * sizeof(uint32_t), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.cmds, scripts.cmds.data(), scripts.cmds.size() * sizeof(uint64_t), s);
  if (rc == ISIM_OK) rc = upload((void **)&t.svc_hold, hold.data(), hold.size() * sizeof(uint64_t), s);
  if (rc == ISIM_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_error(ISIM_EHIP, "trace spans: table upload failed");
  (void)hipStreamDestroy(s);
  if (rc != ISIM_OK) {
    free_tables(t);
    return rc;
  }
  st.dev.emplace(device, t);
  out = t;
  return ISIM_OK;
}

int scan_launch(const uint32_t *d_cnt, uint64_t n, uint64_t *d_tile, uint64_t *d_off, uint64_t cap_spans,
                uint64_t *d_info, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {  // d_off[0] = 0 and info: the scan of no tiles, with d_off[0] as its total word
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, d_off, 0ull, d_off, d_info, 0ull);
  } else {
    const uint32_t tiles = (uint32_t)tiles_of(n);
    hipLaunchKernelGGL(k_tile_sums, dim3(tiles), dim3(kT), 0, s, d_cnt, n, d_tile);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, d_tile, (uint64_t)tiles, d_off + n, d_info, n);
    hipLaunchKernelGGL(k_offsets, dim3(tiles), dim3(kT), 0, s, d_cnt, n, (const uint64_t *)d_tile, d_off, cap_spans,
                       d_info);
  }
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int spans_launch(const isim_handler *h, const uint64_t *d_ids, uint64_t n_ids, uint64_t *d_off, isim_span *d_spans,
                 uint64_t cap_spans, uint64_t *d_info, void *d_workspace, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const HandlerView v = handler_view(h);
  const Program &p = *v.prog;
  const SpanWs ws = span_ws(p, n_ids);
  char *wsp = (char *)d_workspace;
  if (n_ids == 0) return scan_launch(nullptr, 0, nullptr, d_off, cap_spans, d_info, stream);
  DevTables t;
  if (const int rc = device_tables(v, t)) return rc;
  unsigned long long *work = (unsigned long long *)(wsp + ws.off_work);
  WK k{};
  k.ids = d_ids;
  k.n = n_ids;
  k.nodes = t.nodes;
  k.ext = t.ext;
  k.step = t.step;
  k.slot_callee = t.slot_callee;
  k.cnt = (uint32_t *)(wsp + ws.off_cnt);
  k.off = d_off;
  k.spans = d_spans;
  k.cap = cap_spans;
  k.spill = (uint32_t *)(wsp + ws.off_spill);
  k.entry = (uint32_t)p.entry;
  k.k0 = (uint32_t)v.params->seed;
  k.k1 = (uint32_t)(v.params->seed >> 32);
  uint64_t *tile = (uint64_t *)(wsp + ws.off_tile);
  const Frames fr = frames_of(p.tree_frames);
  const bool mb = v.params->error_mode == ISIM_MODE_B;
  const uint32_t blocks = walk_blocks(n_ids);
  hipLaunchKernelGGL(k_zero_work, dim3(1), dim3(64), 0, s, work);
  hipLaunchKernelGGL(walk_kernel(fr, p.tree_t64, mb, p.tree_wide, false), dim3(blocks), dim3(kT), 0, s, k, work);
  if (const int rc = scan_launch(k.cnt, n_ids, tile, d_off, cap_spans, d_info, stream)) return rc;
  hipLaunchKernelGGL(walk_kernel(fr, p.tree_t64, mb, p.tree_wide, true), dim3(blocks), dim3(kT), 0, s, k, work + 1);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

int select_launch(const isim_trace_rec *d_records, uint64_t n, uint64_t trace_begin, uint64_t min_latency,
                  uint32_t cls, uint64_t max_ids, uint64_t *d_ids, uint64_t *d_info, void *d_workspace, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const dev::rec4 *rec = (const dev::rec4 *)d_records;
  if (n == 0) {
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, d_info, 0ull, (uint64_t *)nullptr, d_info, max_ids);
    ISIM_HIPCHK(hipGetLastError());
    return ISIM_OK;
  }
  uint64_t *tile = (uint64_t *)d_workspace;
  const uint32_t tiles = (uint32_t)tiles_of(n);
  hipLaunchKernelGGL(k_sel_count, dim3(tiles), dim3(kT), 0, s, rec, n, min_latency, cls, tile);
  hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, tile, (uint64_t)tiles, (uint64_t *)nullptr, d_info,
                     max_ids);
  hipLaunchKernelGGL(k_sel_scatter, dim3(tiles), dim3(kT), 0, s, rec, n, trace_begin, min_latency, cls, max_ids,
                     (const uint64_t *)tile, d_ids);
  ISIM_HIPCHK(hipGetLastError());
  return ISIM_OK;
}

}  // namespace spans
}  // namespace isim

namespace {
namespace sp = isim::spans;
int sfail(const std::string &msg) { return isim::set_error(ISIM_EINVAL, "trace spans: " + msg); }
}  // namespace

extern "C" {

int isim_trace_spans_device(const isim_handler *h, const uint64_t *d_trace_ids, uint64_t n_ids, uint64_t *d_off,
                            isim_span *d_spans, uint64_t cap_spans, uint64_t *d_info, void *d_workspace,
                            uint64_t workspace_bytes, void *hip_stream) {
  if (!h) return sfail("null handler");
  const isim::Program &p = *sp::handler_view(h).prog;
  if (const char *m = sp::handler_error(p); *m) return sfail(m);
  if (n_ids > sp::kMaxIds) return sfail("n_ids is above 2^32");
  if (!d_off || !d_info) return sfail("null offsets or info");
  if (n_ids && !d_trace_ids) return sfail("null trace ids");
  if (cap_spans && !d_spans) return sfail("null spans with cap_spans > 0");
  if (((uintptr_t)d_trace_ids | (uintptr_t)d_off | (uintptr_t)d_spans | (uintptr_t)d_info | (uintptr_t)d_workspace) & 7u)
    return sfail("the buffers must be 8-byte aligned");
  if (n_ids && (!d_workspace || workspace_bytes < sp::span_ws(p, n_ids).bytes))
    return sfail("the workspace is smaller than isim_trace_spans_workspace_bytes()");
  return sp::spans_launch(h, d_trace_ids, n_ids, d_off, d_spans, cap_spans, d_info, d_workspace, hip_stream);
}

int isim_trace_spans(int device, const isim_handler *h, const uint64_t *h_ids, uint64_t n_ids, uint64_t *h_off,
                     isim_span *h_spans, uint64_t cap_spans, uint64_t *h_info) {
  if (!h) return sfail("null handler");
  const isim::Program &p = *sp::handler_view(h).prog;
  if (const char *m = sp::handler_error(p); *m) return sfail(m);
  if (n_ids > sp::kMaxIds) return sfail("n_ids is above 2^32");
  if (!h_off || !h_info || (n_ids && !h_ids) || (cap_spans && !h_spans)) return sfail("null argument");
  const uint64_t ws_bytes = sp::span_ws(p, n_ids).bytes;
  isim::HostStage stage(device);
  void *d_ids = stage.upload(h_ids, n_ids * 8), *d_off = stage.alloc((n_ids + 1) * 8);
  void *d_spans = stage.alloc(cap_spans * sizeof(isim_span)), *d_info = stage.alloc(ISIM_SPAN_INFO_WORDS * 8);
  void *d_ws = stage.alloc(n_ids ? ws_bytes : 0);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_trace_spans_device(h, (const uint64_t *)d_ids, n_ids, (uint64_t *)d_off, (isim_span *)d_spans,
                                             cap_spans, (uint64_t *)d_info, d_ws, ws_bytes, stage.stream()))
    return rc;
  if (const int rc = stage.download(h_info, d_info, ISIM_SPAN_INFO_WORDS * 8)) return rc;
  if (const int rc = stage.download(h_off, d_off, (n_ids + 1) * 8)) return rc;
  const uint64_t written = h_info[ISIM_SPAN_WRITTEN];
  if (const int rc = stage.download(h_spans, d_spans, h_off[written] * sizeof(isim_span))) return rc;
  return isim_trace_spans_place(h, h_off, written, h_spans);
}

int isim_select_traces_device(const isim_trace_rec *d_records, uint64_t n, uint64_t trace_begin,
                              uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *d_ids,
                              uint64_t *d_info, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
  if (!d_info || (n && !d_records) || (max_ids && !d_ids)) return sfail("select: null argument");
  if (cls > ISIM_Q_500) return sfail("select: the class must be ISIM_Q_ALL, ISIM_Q_200 or ISIM_Q_500");
  if (n > sp::kMaxRecords) return sfail("select: n is above 2^40");
  if (((uintptr_t)d_records & 15u) || (((uintptr_t)d_ids | (uintptr_t)d_info | (uintptr_t)d_workspace) & 7u))
    return sfail("select: records must be 16-byte aligned, the other buffers 8-byte aligned");
  if (n && (!d_workspace || workspace_bytes < sp::select_ws_bytes(n)))
    return sfail("select: the workspace is smaller than isim_select_traces_workspace_bytes()");
  return sp::select_launch(d_records, n, trace_begin, min_latency_ns, cls, max_ids, d_ids, d_info, d_workspace,
                           hip_stream);
}

int isim_select_traces(int device, const isim_trace_rec *h_records, uint64_t n, uint64_t trace_begin,
                       uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *h_ids, uint64_t *h_info) {
  if (!h_info || (n && !h_records) || (max_ids && !h_ids)) return sfail("select: null argument");
  if (cls > ISIM_Q_500) return sfail("select: the class must be ISIM_Q_ALL, ISIM_Q_200 or ISIM_Q_500");
  if (n > sp::kMaxRecords) return sfail("select: n is above 2^40");
  const uint64_t keep = max_ids < n ? max_ids : n, ws_bytes = sp::select_ws_bytes(n);
  isim::HostStage stage(device);
  void *d_rec = stage.upload(h_records, n * sizeof(isim_trace_rec)), *d_ids = stage.alloc(keep * 8);
  void *d_info = stage.alloc(16), *d_ws = stage.alloc(n ? ws_bytes : 0);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (const int rc = isim_select_traces_device((const isim_trace_rec *)d_rec, n, trace_begin, min_latency_ns, cls, keep,
                                               (uint64_t *)d_ids, (uint64_t *)d_info, d_ws, ws_bytes, stage.stream()))
    return rc;
  if (const int rc = stage.download(h_info, d_info, 16)) return rc;
  h_info[1] = h_info[0] < max_ids ? h_info[0] : max_ids;
  return stage.download(h_ids, d_ids, h_info[1] * 8);
}

}  // extern "C"
