// The walk on a device (include/isim.h isim_serve*, isim_handler_launch_info):
// the kernel kind and launch shape of a handler, its tables' upload, and the
// launch.  Host code; the kernels are in walk.hip and tree.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "handler.h"
#include "host_stage.h"

namespace isim {
namespace {

#ifndef ISIM_DYN_MIN_GAIN
#define ISIM_DYN_MIN_GAIN 0  // resident waves a smaller workgroup / global counters must add to be chosen
#endif

// LDS layout of the walk kernel for a given workgroup size (walk.hip).
uint32_t lds_need(const Program &p, uint32_t waves, bool counters) {
  uint32_t b = kLdsAccBytes + kHistWords * 4u;
  if (counters) b += 8u * (uint32_t)p.n_slots;
  b = (b + 15u) & ~15u;
  if (!p.static_walk) {
    uint32_t tt = p.time_bits == 32 ? 4u : 8u;
    b += waves * (uint32_t)p.max_frames * 64u * (2u * tt + 4u);
  }
  return b;
}

struct KindChoice {
  uint32_t kind;
  uint32_t mark_words;  // kind 8
};

// The kernel kind of a program under the handler's flags, for a device with
// lds_max bytes of LDS per workgroup.  Each step reads the one before it.
KindChoice choose_kind(const Program &p, const isim_params &params, uint32_t lds_max) {
  const uint32_t interp = p.time_bits == 64 ? 1u : 0u;
  // 1. the draw stream when the program has one, else an interpreter
  uint32_t kind = p.stream_nodes ? 4u : (p.static_walk ? 0u : 2u) + interp;
  // 2. ISIM_FLAG_NO_STREAM
  if ((params.flags & ISIM_FLAG_NO_STREAM) && kind == 4) kind = interp;
  // 3. mode B on the draw stream: the per-lane bit stack holds 32 stack
  // positions (ISIM_FLAG_BIT_STACK), else the close list (any depth) ...
  if (kind == 4 && params.error_mode == ISIM_MODE_B)
    kind = (params.flags & ISIM_FLAG_BIT_STACK) ? (p.max_depth <= 32 ? 5u : 4u) : 6u;
  // ... or sparse ancestor marking (kind 8) when its per-position mark table
  // fits the LDS next to the histograms (ISIM_FLAG_CLOSE_LIST: kind 6)
  if (kind == 6 && !(params.flags & ISIM_FLAG_CLOSE_LIST)) {
    const uint32_t words = p.stream_nodes + 1u;
    if (kLdsAccBytes + kHistWords * 4u + 4u * words <= lds_max) return {8, words};
  }
  // 4. dynamic walks: the lane tree walk when the unrolled tree was built and
  // its LDS layout placed (program.cpp place_tree); else the wave walk
  if (!p.static_walk && p.has_tree() && !(params.flags & ISIM_FLAG_WAVE_WALK) && p.tree_layout.bytes <= lds_max)
    kind = 7;
  return {kind, 0};
}

// the lane tree walk's kernel and the workgroup size with the most resident
// waves per CU (registers and the LDS layout both bound it: two 768-thread
// workgroups = 24 waves when the kernel fits 80 VGPRs and the layout half the LDS)
int tune_tree(const Program &p, bool modeb, WalkShape &sh) {
  sh.kernel = tree_kernel(modeb, p.tree_frames, p.tree_frames > tree_reg_frames(p.tree_frames, p.tree_t64, p.tree_wide),
                          p.tree_layout.nodes_lds != 0, (p.tree_flags & kTreeAnyConc) != 0,
                          (p.tree_flags & kTreeAnyDraw) != 0, p.tree_layout.wg_per_cu == 2, p.tree_t64, p.tree_wide,
                          p.tree_dag);
  if (!sh.kernel) return set_error(ISIM_EHIP, "no lane-tree-walk kernel for this tree");
  sh.lds_bytes = p.tree_layout.bytes;
  sh.lds_counters = 1;
  ISIM_HIPCHK(hipFuncSetAttribute((const void *)sh.kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh.lds_bytes));
  uint32_t best_t = kWgThreads, best_res = 0;
  for (uint32_t t : {1024u, 768u, 512u}) {
    int pc = 0;
    ISIM_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void *)sh.kernel, (int)t, sh.lds_bytes));
    if ((uint32_t)pc * t / 64u > best_res) {
      best_res = (uint32_t)pc * t / 64u;
      best_t = t;
    }
  }
  sh.threads = best_t;
  return ISIM_OK;
}

// The launch shape of the chosen kind on this device: kernel, workgroup size,
// LDS bytes, where the site counters live, and the resident workgroups.
int tune_shape(const Program &p, const isim_params &params, const hipDeviceProp_t &prop, uint32_t lds_max,
               KindChoice choice, WalkShape &sh) {
  const bool modeb = params.error_mode == ISIM_MODE_B;
  // Largest workgroup (waves) whose LDS fits, counters in LDS if possible.
  bool counters = true;
  uint32_t waves = 16;
  while (waves > 1 && lds_need(p, waves, counters) > lds_max) waves >>= 1;
  if (lds_need(p, waves, counters) > lds_max) {
    counters = false;
    waves = 16;
    while (waves > 1 && lds_need(p, waves, counters) > lds_max) waves >>= 1;
    if (lds_need(p, waves, counters) > lds_max) return set_error(ISIM_EDEPTH, "call stack does not fit in LDS");
  }
  sh.kind = choice.kind;
  sh.mark_words = choice.mark_words;
  if (sh.kind == 7) {
    if (const int rc = tune_tree(p, modeb, sh)) return rc;
  } else if (!p.static_walk) {
    // dynamic walks keep per-lane frame stacks in LDS (waves x frames x 64
    // lanes): the workgroup size with the most resident waves per CU, not the
    // largest that fits
    uint32_t best_w = waves, best_res = 0;
    bool best_c = counters;
    for (int c = counters ? 1 : 0; c >= 0; --c) {
      void *kern = walk_kernel((int)sh.kind, modeb, c != 0);
      for (uint32_t w = 16; w >= 1; w >>= 1) {
        const uint32_t need = lds_need(p, w, c != 0);
        if (need > lds_max) continue;
        ISIM_HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        int pc = 0;
        ISIM_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void *)kern, (int)(w * 64u), need));
        const uint32_t res = (uint32_t)pc * w;
        if (res > best_res + ISIM_DYN_MIN_GAIN) {  // the LDS counter table wins ties
          best_res = res;
          best_w = w;
          best_c = c != 0;
        }
      }
    }
    waves = best_w;
    counters = best_c;
  } else if (sh.kind == 8) {  // the mark table in place of the LDS site counters' own rows
    counters = true;
    waves = 16;
  }
  if (sh.kind != 7) {
    sh.kernel = walk_kernel((int)sh.kind, modeb, counters);
    sh.threads = waves * 64u;
    sh.lds_bytes = sh.kind == 8 ? kLdsAccBytes + kHistWords * 4u + 4u * sh.mark_words : lds_need(p, waves, counters);
    sh.lds_counters = counters ? 1u : 0u;
  }
  if (is_stream(sh.kind)) {
    sh.draw_free = true;
    for (const Node &nd : p.stream) sh.draw_free = sh.draw_free && nd.thr == 0;
  }
  ISIM_HIPCHK(hipFuncSetAttribute((const void *)sh.kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh.lds_bytes));
  int per_cu = 0;
  ISIM_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)sh.kernel, (int)sh.threads,
                                                           sh.lds_bytes));
  if (per_cu < 1) return set_error(ISIM_EHIP, "walk kernel cannot be resident (occupancy 0)");
  sh.per_cu = (uint32_t)per_cu;
  sh.max_blocks = (uint32_t)per_cu * (uint32_t)prop.multiProcessorCount;
  // per-workgroup LDS site counters are u32: launch_walk splits a batch so
  // that no workgroup can count past 2^32 at one site (traces x calls
  // through the site per trace)
  sh.max_mult = std::max<uint64_t>(1, p.hops_upper);
  if (sh.kind == 7) sh.max_mult = std::max<uint32_t>(1, p.tree_mult);
  if (is_stream(sh.kind)) {
    sh.max_mult = 1;
    for (uint32_t m : p.stream_mult) sh.max_mult = std::max<uint64_t>(sh.max_mult, m);
  }
  return ISIM_OK;
}

// the lean mode-A kernel beside the general one: same workgroup, LDS and
// grid.  It is built for the same waves per SIMD (63 VGPRs against 60); were
// it ever less resident, the launches keep the general kernel.
int tune_lean(WalkShape &sh) {
  void *kern = walk_kernel_lean(sh.lds_counters != 0);
  ISIM_HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh.lds_bytes));
  int per_cu = 0;
  ISIM_HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kern, (int)sh.threads,
                                                           sh.lds_bytes));
  if ((uint32_t)per_cu >= sh.per_cu) sh.lean_kernel = kern;
  return ISIM_OK;
}

// the wave interpreters (kinds 0-3): the program and the per-slot duration words
int upload_interp(const isim_handler *h, DevState &st) {
  const Program &p = h->prog;
  if (const int rc = upload(st.prog, p.code)) return rc;
  return svc_dur_rows(h) && p.n_slots > 0 ? upload(st.dur, p.slot_dur) : ISIM_OK;
}

// the draw stream (kinds 4, 5, 6, 8): the records, the slot multiplicities, mode B's tables, the launches' slots
int upload_stream(const Program &p, bool modeb, DevState &st) {
  const WalkShape &sh = st.shape;
  // the kernel prefetches group g+1 unconditionally: two zero groups (32 B
  // each) of tail padding keep those reads inside the buffer
  if (const int rc = upload(st.prog, sh.kind == 8 ? p.stream_mark.data() : p.stream.data(),
                            p.stream.size() * sizeof(Node), 2 * 4 * sizeof(Node)))
    return rc;
  if (p.n_slots > 0)
    if (const int rc = upload(st.stream.mult, p.stream_mult)) return rc;
  size_t stage_words = 0;  // of one launch's row
  if (sh.kind == 6) {
    // zero tail padding: the kernel prefetches blocks of 8 closes past the end
    if (const int rc = upload(st.stream.closes, p.stream_closes, kClosePad * sizeof(StreamClose))) return rc;
    if (const int rc = upload(st.stream.close_slot, p.stream_close_slot, 64 * sizeof(uint32_t))) return rc;
    if (const int rc = upload(st.stream.close_end, p.stream_close_end, 2 * sizeof(uint32_t))) return rc;
  }
  if (sh.kind == 8) {
    // the fold's inputs (per real record) and the launches' mark rows
    std::vector<uint32_t> slot(p.stream_nodes);
    for (uint32_t r = 0; r < p.stream_nodes; ++r) slot[r] = p.stream[r].meta & 0xFFFFFFu;
    if (const int rc = upload(st.stream.mark_end, p.stream_end.data(), p.stream_nodes * sizeof(uint32_t))) return rc;
    if (const int rc = upload(st.stream.mark_slot, slot)) return rc;
    stage_words = sh.mark_words;
    ISIM_HIPCHK(hipFuncSetAttribute(mark_fold_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sh.mark_words * 4u)));
  } else if (sh.lds_counters && p.n_slots > 0 && p.n_slots <= kStageMaxSlots) {
    stage_words = p.n_slots;
  }
  if (stage_words)
    if (const int rc = upload(st.slots.stage, nullptr, 0, kWorkSlots * stage_words * sizeof(uint32_t))) return rc;
  // the launches' group tables, while kWorkSlots of them stay within the
  // cap (ISIM_NO_GROUP_TABLE=1, for tests: none, as for a longer stream)
  st.slots.gtab_groups = (p.stream_nodes + 3) / 4;
  const size_t tab_bytes = (size_t)(st.slots.gtab_groups + kGroupPad) * sizeof(GroupEnt) * kWorkSlots;
  const char *no_tab = std::getenv("ISIM_NO_GROUP_TABLE");
  if (tab_bytes > kGroupTableMaxBytes || (no_tab && no_tab[0] == '1')) return ISIM_OK;
  if (const int rc = alloc(st.slots.gtab, tab_bytes)) return rc;
  // mode A: the lean kernel for the launches that can take it (ISIM_NO_LEAN_WALK=1, for tests: none)
  const char *no_lean = std::getenv("ISIM_NO_LEAN_WALK");
  if (sh.kind == 4 && !modeb && !(no_lean && no_lean[0] == '1')) return tune_lean(st.shape);
  return ISIM_OK;
}

// the lane tree walk (kind 7): the nodes, the tables beside them, the first spill area
int upload_tree(const Program &p, DevState &st) {
  TreeTables &t = st.tree;
  if (const int rc = p.tree_wide ? upload(st.prog, p.tree_nodes_w) : upload(st.prog, p.tree_nodes)) return rc;
  if (const int rc = upload(t.ext, p.tree_ext)) return rc;
  if (const int rc = upload(t.step, p.tree_step)) return rc;
  if (const int rc = upload(t.sum_row, p.sum_row)) return rc;
  if (const int rc = upload(t.slot_tc, p.slot_tc)) return rc;
  if (const int rc = upload(t.lds_slot, p.tree_lds_slot)) return rc;
  if (const int rc = upload(t.dyn, p.tree_dyn)) return rc;
  if (p.n_slots > 0)  // per slot: callee row | static bucket (the kernel's duration flush)
    if (const int rc = upload(st.dur, p.slot_tbkt)) return rc;
  const uint32_t regf = tree_reg_frames(p.tree_frames, p.tree_t64, p.tree_wide);
  if (p.tree_frames <= regf) return ISIM_OK;
  // the spill areas: frames below the register frames, one column per lane
  // of a full grid; a launch waits for the area's previous launch (launch_walk_one)
  t.spill_lanes = st.shape.max_blocks * st.shape.threads;
  t.spill_words = (size_t)(p.tree_frames - regf) *
                  ((p.tree_t64 ? kTreeSpillWords64 : kTreeSpillWords) + (p.tree_wide ? kTreeSpillWide : 0u)) *
                  t.spill_lanes;
  if (const int rc = alloc(t.spill[0], t.spill_words * sizeof(uint32_t))) return rc;
  for (DevEvent &e : t.spill_ev) {
    hipEvent_t ev = nullptr;
    ISIM_HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e.reset(ev);
  }
  return ISIM_OK;
}

// Chooses the kernel and launch shape for `device` and uploads the program.
// On failure `st` frees whatever it holds by then.
int build_device(isim_handler *h, int device, DevState &st) {
  hipDeviceProp_t prop;
  ISIM_HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(ISIM_ENODEV, std::string("libisim is built for gfx950 only; device is ") + prop.gcnArchName);
  const Program &p = h->prog;
  // HIP reports 64 KiB per block by default; a gfx950 workgroup may use all
  // 160 KiB of the CU's LDS once the kernel attribute is raised.
  const uint32_t lds_max = (uint32_t)std::max<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor);
  if (const int rc = tune_shape(p, h->params, prop, lds_max, choose_kind(p, h->params, lds_max), st.shape)) return rc;
  const uint32_t kind = st.shape.kind;
  const bool modeb = h->params.error_mode == ISIM_MODE_B;
  const int rc = is_stream(kind) ? upload_stream(p, modeb, st) : kind == 7 ? upload_tree(p, st) : upload_interp(h, st);
  if (rc != ISIM_OK) return rc;
  return upload(st.slots.work, nullptr, 0, (size_t)kWorkWords * kWorkSlots * sizeof(unsigned long long));
}

// Per-workgroup LDS accumulators are u32: histogram counts (at most the
// launch's traces) and, with LDS site counters, per-site counts (at most
// traces x calls through the site per trace; a workgroup may claim any
// share of a launch's batches).  Launches are split so neither can wrap:
// below 2^31 traces, and below 2^32 / max_mult traces with LDS counters (a
// DAG whose shared callee is reached 2^22 times per trace: 1,023 traces per
// launch).  Global counters are u64 atomics and need no split.
uint64_t max_launch_traces(const WalkShape &sh) {
  uint64_t m = 1ull << 31;
  if (sh.lds_counters) m = std::min<uint64_t>(m, std::max<uint64_t>(1, 0xFFFFFFFFull / sh.max_mult));
  return m;
}

}  // namespace

// A launch takes the lean mode-A kernel when every one of its batches would
// draw from the launch's group table in the general kernel: there is a table,
// the walk is mode A on the draw stream, and the trace ids share the high
// word the table is built for (so no batch straddles 2^32 or lies past it).
bool lean_walk_eligible(bool has_table, uint32_t kind, bool modeb, uint64_t trace_begin, uint64_t n_traces) {
  if (!has_table || kind != 4 || modeb || n_traces == 0) return false;
  const uint64_t last = trace_begin + (n_traces - 1);
  return last >= trace_begin && (trace_begin >> 32) == (last >> 32);
}

// launches that took the lean kernel, process-wide (isim_debug_lean_walk_launches)
static uint64_t g_lean_launches = 0;

namespace {

int launch_walk_one(isim_handler *h, DevState *st, uint64_t trace_begin, uint64_t n_traces,
                    isim_trace_rec *d_records, uint64_t *d_stats, void *hip_stream) {
  const WalkShape &sh = st->shape;
  TreeTables &tree = st->tree;
  KParams kp{};
  kp.trace_begin = trace_begin;
  kp.n_traces = n_traces;
  kp.seed_lo = (uint32_t)h->params.seed;
  kp.seed_hi = (uint32_t)(h->params.seed >> 32);
  kp.n_slots = (uint32_t)h->prog.n_slots;
  kp.max_frames = (uint32_t)h->prog.max_frames;
  kp.lds_counters = sh.lds_counters;
  kp.n_nodes = h->prog.stream_nodes;
  kp.t_static = h->prog.max_latency;
  kp.svc_dur = svc_dur_rows(h) ? 1u : 0u;
  kp.root_dur = h->prog.root_dur;
  kp.closes = st->stream.closes.get();
  kp.close_slot = st->stream.close_slot.get();
  kp.close_end = st->stream.close_end.get();
  kp.tree_ext = tree.ext.get();
  kp.tree_step = tree.step.get();
  kp.tree_dyn = tree.dyn.get();
  kp.sum_row = tree.sum_row.get();
  kp.slot_tc = tree.slot_tc.get();
  kp.spill_lanes = tree.spill_lanes;
  kp.n_pos = h->prog.tree_positions();
  kp.n_rows = (uint32_t)h->prog.row_svc.size();
  kp.n_dyn = (uint32_t)h->prog.tree_dyn.size();
  kp.dyn_words = h->prog.tree_dyn_words;
  kp.tree_flags = h->prog.tree_flags;
  kp.lay = h->prog.tree_layout;
  kp.lds_slot = tree.lds_slot.get();
  kp.n_lds_slots = (uint32_t)h->prog.tree_lds_slot.size();
  const uint64_t per_wave = is_stream(sh.kind) ? stream_traces_per_wave() : 64u;
  const uint64_t batches = (n_traces + per_wave - 1) / per_wave;
  const uint64_t waves = sh.threads / 64;
  const uint64_t want = (batches + waves - 1) / waves;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, sh.max_blocks);
  const uint32_t slot = __atomic_fetch_add(&st->slots.next, 1u, __ATOMIC_RELAXED) % kWorkSlots;
  kp.work = st->slots.work.get() + kWorkWords * slot;
  // u32 staging of the 500 counts: the launch split (launch_walk) keeps n x max_mult below 2^32
  kp.stage = st->slots.stage
                 ? st->slots.stage.get() + (size_t)slot * (sh.kind == 8 ? sh.mark_words : h->prog.n_slots)
                 : nullptr;
  kp.mark_words = sh.mark_words;
  const void *prog = st->prog.get();
  const uint32_t *dur = st->dur.get();
  if (st->slots.gtab) {  // the launch's group table, for the trace ids' high word at its first trace
    GroupEnt *tab = st->slots.gtab.get() + (size_t)slot * (st->slots.gtab_groups + kGroupPad);
    uint32_t n_groups = st->slots.gtab_groups;
    kp.gtab = tab;
    kp.gtab_t_hi = (uint32_t)(trace_begin >> 32);
    void *args0[] = {&prog, &n_groups, &kp.seed_lo, &kp.seed_hi, &kp.gtab_t_hi, &tab};
    ISIM_HIPCHK(hipLaunchKernel(group_table_kernel(), dim3((n_groups + kGroupPad + 255) / 256), dim3(256), args0, 0,
                                (hipStream_t)hip_stream));
  }
  void *args[] = {&prog, &d_records, &d_stats, &dur, &kp};
  void *kernel = sh.kernel;
  if (sh.lean_kernel && lean_walk_eligible(kp.gtab != nullptr, sh.kind, h->params.error_mode == ISIM_MODE_B,
                                           trace_begin, n_traces)) {
    kernel = sh.lean_kernel;
    __atomic_fetch_add(&g_lean_launches, 1, __ATOMIC_RELAXED);
  }
  if (tree.spill[0]) {
    // a spilling walk: the area its stream used last (else the next one,
    // round robin; allocated on first use), ordered after the area's previous
    // launch by an event; the wait, launch and record are one step under the
    // handler's lock.  Not graph-capturable: a captured launch
    // would keep its area in the graph, and nothing could order its replays
    // against the eager launches that later take the same area.
    const hipStream_t hs = (hipStream_t)hip_stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(hs, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
      return set_error(ISIM_EINVAL, "a lane tree walk that spills frames (more nested calling invocations than its "
                                    "register frames) cannot be captured into a HIP graph");
    std::lock_guard<std::mutex> lk(h->spill_mu);
    uint32_t a = kSpillAreas;
    for (uint32_t i = 0; i < kSpillAreas; ++i)
      if (tree.spill_used[i] && tree.spill_last[i] == hs) a = i;
    if (a == kSpillAreas) a = tree.spill_next++ % kSpillAreas;
    if (!tree.spill[a])
      if (const int rc = alloc(tree.spill[a], tree.spill_words * sizeof(uint32_t))) return rc;
    if (tree.spill_used[a]) ISIM_HIPCHK(hipStreamWaitEvent(hs, tree.spill_ev[a].get(), 0));
    kp.spill = tree.spill[a].get();
    ISIM_HIPCHK(hipLaunchKernel(sh.kernel, dim3(grid), dim3(sh.threads), args, sh.lds_bytes, hs));
    ISIM_HIPCHK(hipEventRecord(tree.spill_ev[a].get(), hs));
    tree.spill_last[a] = hs;
    tree.spill_used[a] = true;
  } else {
    ISIM_HIPCHK(hipLaunchKernel(kernel, dim3(grid), dim3(sh.threads), args, sh.lds_bytes, (hipStream_t)hip_stream));
  }
  if (sh.kind == 8) {  // the launch's position marks into the per-site 500 counters
    uint32_t *row = kp.stage;
    uint32_t n = h->prog.stream_nodes, words = sh.mark_words, n_slots = (uint32_t)h->prog.n_slots;
    const uint32_t *end = st->stream.mark_end.get(), *mslot = st->stream.mark_slot.get();
    void *args3[] = {&row, &n, &words, &end, &mslot, &d_stats, &n_slots};
    ISIM_HIPCHK(hipLaunchKernel(mark_fold_kernel(), dim3(1), dim3(1024), args3, words * 4u, (hipStream_t)hip_stream));
  }
  if (is_stream(sh.kind) && h->prog.n_slots > 0) {
    uint32_t n_slots = (uint32_t)h->prog.n_slots;
    const uint32_t *mult = st->stream.mult.get();
    uint32_t *stage = sh.kind == 8 ? nullptr : kp.stage;
    void *args2[] = {&mult, &n_slots, &n_traces, &d_stats, &stage};
    ISIM_HIPCHK(hipLaunchKernel(stream_calls_kernel(), dim3((n_slots + 255) / 256), dim3(256), args2, 0,
                                (hipStream_t)hip_stream));
  }
  return ISIM_OK;
}

int launch_walk(isim_handler *h, DevState *st, uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records,
                uint64_t *d_stats, void *hip_stream) {
  const uint64_t kMaxLaunch = max_launch_traces(st->shape);
  for (uint64_t done = 0; done < n_traces;) {
    const uint64_t n = std::min(n_traces - done, kMaxLaunch);
    const int rc = launch_walk_one(h, st, trace_begin + done, n, d_records ? d_records + done : nullptr, d_stats,
                                   hip_stream);
    if (rc != ISIM_OK) return rc;
    done += n;
  }
  return ISIM_OK;
}

// A draw-free static walk gives every trace the same record and statistics:
// walk ONE trace with the stream kernel (once per device), then a batch is
// a record fill plus n x that trace's statistics (bit-identical by
// construction).
int prepare_constant(isim_handler *h, DevState *st) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (st->constant.stats) return ISIM_OK;
  const uint64_t words = stats_words(h);
  DevBuf<uint64_t> s1;
  DevBuf<isim_trace_rec> r1;
  hipStream_t s = nullptr;
  int rc = ISIM_OK;
  if (hipStreamCreate(&s) != hipSuccess || alloc(s1, words * 8) != ISIM_OK ||
      alloc(r1, sizeof(isim_trace_rec)) != ISIM_OK || hipMemsetAsync(s1.get(), 0, words * 8, s) != hipSuccess)
    rc = set_error(ISIM_EHIP, "constant-walk setup failed");
  if (rc == ISIM_OK) rc = launch_walk(h, st, 0, 1, r1.get(), s1.get(), s);
  if (rc == ISIM_OK &&
      (hipMemcpyAsync(&st->constant.rec, r1.get(), sizeof(isim_trace_rec), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess))
    rc = set_error(ISIM_EHIP, "constant-walk setup failed");
  if (s) (void)hipStreamDestroy(s);
  if (rc == ISIM_OK) st->constant.stats = std::move(s1);
  return rc;
}

}  // namespace

int prepare_device(isim_handler *h, int device, DevState *&out) {
  std::lock_guard<std::mutex> lk(h->mu);
  auto it = h->dev.find(device);
  if (it == h->dev.end()) {
    DevState st;
    if (const int rc = build_device(h, device, st)) return rc;
    it = h->dev.emplace(device, std::move(st)).first;
  }
  out = &it->second;
  return ISIM_OK;
}

}  // namespace isim

using isim::set_error;

extern "C" {

int isim_debug_lean_walk_eligible(int has_table, uint32_t kernel_kind, int mode_b, uint64_t trace_begin,
                                  uint64_t n_traces) {
  return isim::lean_walk_eligible(has_table != 0, kernel_kind, mode_b != 0, trace_begin, n_traces) ? 1 : 0;
}

uint64_t isim_debug_lean_walk_launches(void) { return __atomic_load_n(&isim::g_lean_launches, __ATOMIC_RELAXED); }

int isim_handler_launch_info(isim_handler *h, int device, isim_launch_info *out) {
  if (!h || !out) return set_error(ISIM_EINVAL, "null argument");
  int prev = 0;
  ISIM_HIPCHK(hipGetDevice(&prev));
  ISIM_HIPCHK(hipSetDevice(device));
  isim::DevState *st = nullptr;
  int rc = isim::prepare_device(h, device, st);
  (void)hipSetDevice(prev);
  if (rc != ISIM_OK) return rc;
  const isim::WalkShape &sh = st->shape;
  out->wg_threads = (int32_t)sh.threads;
  out->lds_bytes = (int32_t)sh.lds_bytes;
  out->lds_counters = (int32_t)sh.lds_counters;
  out->blocks_per_cu = (int32_t)sh.per_cu;
  out->max_blocks = (int32_t)sh.max_blocks;
  out->kernel_kind = (int32_t)sh.kind;
  out->fill = sh.draw_free && !(h->params.flags & ISIM_FLAG_WALK_ALL) ? 1 : 0;
  out->tree_wide = sh.kind == 7 && h->prog.tree_wide ? (h->prog.tree_dag ? 2 : 1) : 0;
  out->max_launch_traces = isim::max_launch_traces(sh);
  return ISIM_OK;
}

int isim_serve_device(isim_handler *h, uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records,
                      uint64_t *d_stats, void *hip_stream) {
  if (!h || !d_stats) return set_error(ISIM_EINVAL, "null argument");
  if (n_traces == 0) return ISIM_OK;
  int device = 0;
  ISIM_HIPCHK(hipGetDevice(&device));
  isim::DevState *st = nullptr;
  int rc = isim::prepare_device(h, device, st);
  if (rc != ISIM_OK) return rc;
  if (st->shape.draw_free && !(h->params.flags & ISIM_FLAG_WALK_ALL)) {
    rc = isim::prepare_constant(h, st);
    if (rc != ISIM_OK) return rc;
    const uint32_t words = (uint32_t)isim::stats_words(h);
    uint64_t blocks = (n_traces + 1023) / 1024;
    blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, 8192));
    const isim_trace_rec r = st->constant.rec;
    const uint64_t *s1 = st->constant.stats.get();
    void *args[] = {&d_records, &n_traces, (void *)&r, &s1, &d_stats, (void *)&words};
    ISIM_HIPCHK(hipLaunchKernel(isim::fill_const_kernel(), dim3((uint32_t)blocks), dim3(256), args, 0,
                                (hipStream_t)hip_stream));
    return ISIM_OK;
  }
  return isim::launch_walk(h, st, trace_begin, n_traces, d_records, d_stats, hip_stream);
}

int isim_serve(isim_handler *h, int device, uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *h_records,
               uint64_t *h_stats) {
  if (!h) return set_error(ISIM_EINVAL, "null handler");
  const uint64_t words = isim::stats_words(h), rec_bytes = h_records ? n_traces * sizeof(isim_trace_rec) : 0;
  isim::HostStage stage(device);
  uint64_t *d_stats = (uint64_t *)stage.alloc(words * 8);
  isim_trace_rec *d_rec = (isim_trace_rec *)stage.alloc(rec_bytes);
  if (stage.rc() != ISIM_OK) return stage.rc();
  if (hipMemsetAsync(d_stats, 0, words * 8, stage.stream()) != hipSuccess)
    return set_error(ISIM_EHIP, "hipMemset failed");
  if (const int rc = isim_serve_device(h, trace_begin, n_traces, d_rec, d_stats, stage.stream())) return rc;
  if (const hipError_t e = hipStreamSynchronize(stage.stream()); e != hipSuccess)
    return set_error(ISIM_EHIP, std::string("walk kernel failed: ") + hipGetErrorName(e) + ": " + hipGetErrorString(e));
  if (h_stats)
    if (const int rc = stage.download(h_stats, d_stats, words * 8)) return rc;
  return stage.download(h_records, d_rec, rec_bytes);
}

}  // extern "C"
