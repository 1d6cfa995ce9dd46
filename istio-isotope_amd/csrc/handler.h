// The handler behind the C ABI and what it keeps on each device, for the
// translation units that implement the ABI: api.hip (create, info, free, the
// stats folds), walk_host.hip (the walk's device setup and launch) and
// des_host.hip (the DES entry points).  Everything on a device is owned by a
// DevBuf or its kin (dev_buf.h): a DevState frees itself.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/isim.h"
#include "des.h"
#include "dev_buf.h"
#include "graph.h"
#include "kernel_abi.h"
#include "load_profile.h"
#include "program.h"

namespace isim {

// the kernel and its launch shape (walk_host.hip choose_kind, tune_shape)
struct WalkShape {
  void *kernel = nullptr;
  void *lean_kernel = nullptr;  // kind 4, mode A: the kernel of the launches that lean_walk_eligible admits (or none)
  uint32_t kind = 0;
  uint32_t mark_words = 0;  // kind 8: position marks per workgroup (records + the sentinel)
  uint32_t threads = 0;
  uint32_t lds_bytes = 0;
  uint32_t lds_counters = 0;
  uint32_t per_cu = 0;
  uint32_t max_blocks = 0;  // resident workgroups for the whole device
  uint64_t max_mult = 0;    // largest per-trace count of one per-site counter (calls through a site)
  bool draw_free = false;   // a static walk with no error draw anywhere: every trace walks alike
};

// the draw stream's tables beside the records (kinds 4, 5, 6, 8)
struct StreamTables {
  DevBuf<uint32_t> mult;        // per-slot call multiplicity
  DevBuf<StreamClose> closes;   // mode B, kind 6: the close list
  DevBuf<uint32_t> close_slot;  // per close: call-site slot
  DevBuf<uint32_t> close_end;   // and its per-chunk ends
  DevBuf<uint32_t> mark_end;    // mode B, kind 8: per record its subtree's last record
  DevBuf<uint32_t> mark_slot;   // and its call-site slot
};

// the lane tree walk's tables beside the nodes (kind 7)
struct TreeTables {
  DevBuf<TreeExt> ext;         // per position
  DevBuf<TreeStep> step;       // per position, the rare step facts
  DevBuf<TreeDynRow> dyn;      // the LDS bucket tables' rows
  DevBuf<uint32_t> sum_row;    // per LDS sum index, its row
  DevBuf<uint32_t> slot_tc;    // per slot, the leaf callee's latency
  DevBuf<uint32_t> lds_slot;   // wide tree: per LDS counter its slot
  // frames below the register stack, up to kSpillAreas areas (the first
  // allocated with the program, the others when a further stream first needs one)
  DevBuf<uint32_t> spill[kSpillAreas];
  uint32_t spill_lanes = 0;
  size_t spill_words = 0;                    // u32 words of one area
  DevEvent spill_ev[kSpillAreas];            // recorded after each area's latest launch
  hipStream_t spill_last[kSpillAreas] = {};  // the stream of that launch
  bool spill_used[kSpillAreas] = {};
  uint32_t spill_next = 0;
};

// per-launch state: launches in flight use distinct slots of each
struct LaunchSlots {
  DevBuf<unsigned long long> work;  // kWorkSlots sets of batch queues, zero between launches
  DevBuf<uint32_t> stage;  // draw stream: kWorkSlots rows of u32 500 counts (kind 8: marks), zero between launches
  DevBuf<GroupEnt> gtab;   // draw stream: kWorkSlots group tables, each written by its launch (or none)
  uint32_t gtab_groups = 0;  // Philox groups of the stream (a table: + kGroupPad entries)
  uint32_t next = 0;
};

// draw-free static walks: the one trace every trace repeats (computed on first use)
struct ConstWalk {
  DevBuf<uint64_t> stats;
  isim_trace_rec rec{};
};

// DES (config 5): the plan uploaded on first use (des_host.hip des_prepare)
struct DesTables {
  DevBuf<void> pos, ext, steps;
  DevBuf<uint32_t> child, level, mult, fast, sort, arr, zero, pipe;
  // the item engine (dynamic walks): per-position plan facts, BK rounds, the tree
  DevBuf<void> ipos, nodes, text, tstep;
  DevBuf<uint32_t> sround;
  DevBuf<lp::Seg> lp_table;  // load profiles: the segment table of the batch being enqueued (first use)
  DevPool pool;              // the item engine's per-batch arrays (a private pool)
  bool ready = false;        // every upload above succeeded
};

struct DevState {
  WalkShape shape;
  DevBuf<void> prog;      // Ins[] (interpreters), Node[] (draw stream) or the tree's nodes
  DevBuf<uint32_t> dur;   // dynamic walks: per-slot duration-table word (row | leaf bucket << 24)
  StreamTables stream;
  TreeTables tree;
  LaunchSlots slots;
  ConstWalk constant;
  DesTables des;
};

}  // namespace isim

struct isim_handler {
  isim::Program prog;
  isim_params params{};
  std::mutex mu;
  std::mutex spill_mu;  // kind 7 spill areas: area choice, wait, launch, record
  std::map<int, isim::DevState> dev;
  // the DES plan is built on first use (des_ensure): it unrolls the whole
  // invocation tree, which walks never need
  isim::ServiceGraph graph;
  std::mutex des_mu;
  bool des_built = false;
  int des_rc = ISIM_OK;
  std::string des_err;
  isim::DesPlan des;
  std::vector<uint32_t> des_workers;  // per service, workers per replica (isim_des_workers_set); empty: one each
  std::mutex report_mu;
  isim::DesItemsReport des_report{};  // the item engine's last batch (isim_des_last_batch)
  std::mutex span_mu;
  std::shared_ptr<void> span_state;   // trace spans: the per-device tables of spans.hip (its own deleter)
  // each device's state goes with that device current
  ~isim_handler() {
    while (!dev.empty()) {
      int cur = 0;
      const bool there = hipGetDevice(&cur) == hipSuccess && hipSetDevice(dev.begin()->first) == hipSuccess;
      dev.erase(dev.begin());
      if (there) (void)hipSetDevice(cur);
    }
  }
};

namespace isim {

// Kernel kinds 4, 5, 6 and 8 walk the draw stream (static walks); 7 is the lane tree walk.
inline bool is_stream(uint32_t kind) { return (kind >= 4 && kind <= 6) || kind == 8; }

// Rows of the device per-service duration table (dynamic walks only).
inline uint64_t svc_dur_rows(const isim_handler *h) {
  if (h->prog.static_walk || (h->params.flags & ISIM_FLAG_NO_SVC_DUR)) return 0;
  return h->prog.row_svc.size();
}

inline uint64_t stats_words(const isim_handler *h) {
  return ISIM_ST_SVC_DUR(h->prog.n_slots) + (uint64_t)ISIM_SVC_DUR_WORDS * svc_dur_rows(h);
}

// walk_host.hip: the handler's state on `device` (the current one), built on first use
int prepare_device(isim_handler *h, int device, DevState *&out);

}  // namespace isim
