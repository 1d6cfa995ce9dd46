// The workspaces of the two DES engines, each stated once (DESIGN.md §10.6,
// §10.9): a layout function over an Arena (arena.h) names every buffer and
// writes its size once; a null arena sizes, an arena over the allocation
// carves.  Host only, no HIP: rocPRIM's temporary sizes come in as numbers.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "arena.h"
#include "des.h"

namespace isim {

// ---- static engine (des.hip)
namespace dev {
// state of one (position, chunk) of the chained queue scan (des.hip chain_body)
struct ChainState {
  uint64_t B, C;   // B: the chunk's largest key a_t - t h, as int64 (flag >= 1); C unused
  uint64_t P;      // the largest key up to and including the chunk (flag 2)
  uint32_t flag, pad;
};
static_assert(sizeof(ChainState) == 32, "ChainState is 32 bytes");
}  // namespace dev

constexpr uint64_t kDesArrChunk = 8192;   // traces per arrivals chunk (des.hip kDesChunk)
constexpr uint64_t kDesDownChunk = 4096;  // traces per queue-pass chunk (des.hip kDownChunk)
inline uint64_t des_row_ld(uint64_t n) { return (n + 15) & ~15ull; }                     // row pitch, elements
inline uint64_t des_status_wpr(uint64_t n) { return (((n + 31) / 32) + 15) & ~15ull; }  // status words per row

inline void des_layout(Arena &a, DesBufs &b, const DesPlan &plan, uint64_t n, uint64_t stats_words,
                       uint64_t table_rows, uint64_t sort_tmp_bytes) {
  const uint64_t n_pos = plan.pos.size(), ld = des_row_ld(n);
  // rows [n_pos][ld] (starts, finishes) and [steps][ld], sized for u64 so
  // one workspace serves both row widths; no step begins: no BK part
  b.W = a.take<uint64_t>(n_pos * ld);
  b.WF = a.take<uint64_t>(n_pos * ld);
  b.BK = plan.steps.empty() ? a.here() : a.take<uint64_t>(plan.steps.size() * ld);
  b.A = a.take<uint64_t>(n);
  b.E = a.take<uint32_t>(n);
  b.blk = a.take<uint64_t>((n + kDesArrChunk - 1) / kDesArrChunk + 1);
  // chained and pipelined queue passes: a ticket counter per launch, the
  // positions' published chunk counts, one state per (position, chunk); all
  // zeroed before every pass, [tickets, tickets + pass_zero_bytes)
  const uint64_t states = n_pos * ((n + kDesDownChunk - 1) / kDesDownChunk), z0 = a.bytes();
  b.tickets = a.take<uint32_t>(4ull * plan.rounds());
  b.prog = a.take<uint32_t>(n_pos);
  b.pass_zero_bytes = a.bytes() - z0 + states * sizeof(dev::ChainState);
  b.chain = a.take<dev::ChainState>(states);
  // two words of one part, cleared together: the overflow / fault flag and a
  // cyclic schedule's changed flag
  b.ovf = a.take<uint32_t>(2);
  b.changed = b.ovf ? b.ovf + 1 : nullptr;
  b.stage = a.take<uint64_t>(stats_words + table_rows * ISIM_DES_ROW_WORDS);
  b.stbits = a.take<uint32_t>(n_pos * des_status_wpr(n));
  // the sort path (plans with sort-path services only): keys and values in
  // and out, rocPRIM's temporary storage
  const uint64_t m = (uint64_t)plan.max_sort_pos * n;
  b.keys_a = b.keys_b = nullptr;
  b.vals_a = b.vals_b = nullptr;
  b.sort_tmp = nullptr;
  if (m) {
    b.keys_a = a.take<uint64_t>(m);
    b.keys_b = a.take<uint64_t>(m);
    b.vals_a = a.take<uint32_t>(m);
    b.vals_b = a.take<uint32_t>(m);
    b.sort_tmp = a.take<char>(sort_tmp_bytes);
  }
}

// ---- item engine (des_items.hip)
namespace dit {
// FIFO of one worker as a max-plus map x -> max(x + B, C) on "free at x"
// (des.hip SegMP without the segment flag: rocPRIM's scan by key segments)
struct MP {
  uint64_t B, C;
};
// state of one tile of the chained queue scan (des_items.hip k_qscan)
struct QState {
  uint64_t agg, inc;  // the max after the tile's last segment start (flag >= 1); with the prefix (flag 2)
  uint32_t flag, pad[3];
};
static_assert(sizeof(QState) == 32, "QState is 32 bytes");
// one item of the pre-walk's output (the kernels' uint4, des_items.hip K::erec)
struct alignas(16) ItemRec {
  uint32_t x, y, z, w;
};
constexpr uint32_t kQTile = 512;  // items of k_qscan's smaller tile: the most states a batch needs
constexpr uint32_t kWkTile = 1024; // items of a tile of the worker pools' head-flag scan (des_workers.h)
}  // namespace dit

// the caller's per-trace workspace (isim_des_workspace_bytes)
struct ItemTraceBufs {
  uint64_t *gap, *A, *cnt, *tend;  // gaps, arrivals, hops, inclusive item offsets
  uint32_t *terr;                  // status_err
  unsigned long long *work;        // the refill counters of the two pre-walks
  void *scan_tmp;                  // rocPRIM's u64 scan
};
inline void des_items_trace_layout(Arena &a, ItemTraceBufs &b, uint64_t n, uint64_t scan_tmp_bytes) {
  b.gap = a.take<uint64_t>(n);
  b.A = a.take<uint64_t>(n);
  b.cnt = a.take<uint64_t>(n);
  b.tend = a.take<uint64_t>(n);
  b.terr = a.take<uint32_t>(n);
  b.work = a.take<unsigned long long>(2);
  b.scan_tmp = a.take<char>(scan_tmp_bytes);
  (void)a.take<char>(256);  // one unit of slack the reported size has always had
}

// the per-batch allocation: sized once the batch's items are counted
struct ItemDims {
  uint64_t M, n;             // items, traces
  uint32_t aw, bw, R;        // acc / bk slots per item (DesPlan::item_acc, item_bk); rounds
  uint64_t rows_n, n_pos;    // duration-table rows, positions
  bool cyclic, modeb;
  uint64_t tmp_bytes;        // the largest rocPRIM temporary storage of the batch
  uint32_t chunk_shift;      // the incremental quiet passes' trace chunks: 2^chunk_shift traces
  uint64_t n_chunks() const { return (n >> chunk_shift) + 1; }
  bool pooled = false;       // some service has more than one worker per replica (des_workers.h)
};
struct ItemBufs {
  // per item (after the renumbering: position-major)
  uint32_t *ipos, *ipar, *itr, *ihop;
  uint8_t *iown;
  uint64_t *IA, *IS, *IF, *acc, *bk;
  uint64_t *acc_b;                 // cyclic: callee maxima of the previous pass
  uint16_t *irep;
  uint32_t *ifst;                  // mode B: failed call step per item
  dit::ItemRec *erec;              // the pre-walk's records, trace order
  uint32_t *inv;                   // inverse of the renumbering
  uint32_t *troot;                 // per trace: its entry item
  // step-begin ops: round keys and (item, step) values, unsorted and sorted; offsets per round
  uint32_t *op_k, *op_k2, *d_soff;
  unsigned long long *op_v, *op_v2;
  // the rounds' and finish groups' item lists; per sort round its kept order and the order's trace chunks
  uint32_t *qids, *fids, *ord;
  uint16_t *ordc;
  // one round's queue: sort keys and values in and out, row keys and values, maps, segment ids
  uint64_t *key_a, *key_b;
  uint32_t *val_a, *val_b, *rk_a, *rk_b, *rv_a, *rv_b, *sid;
  dit::MP *mp_in, *mp_out;
  dit::QState *qstate;             // k_qscan's tile states
  uint32_t *qticket;               // and its ticket counter
  uint32_t *ovf;                   // [4]: key overflow, no fixed point, look-back fault, step-op count
  uint64_t *mm;                    // [2][4]: two arrival-range slots (k_qarr)
  uint32_t *chg;                   // [2]: a quiet pass changed a value, (unused)
  uint64_t *d_row_hold;            // per duration-table row: the service's worker hold
  uint32_t *d_poff, *d_qdst, *d_fdst;  // per position: item range, list destinations
  void *tmp;                       // rocPRIM temporary storage
  uint8_t *chg_a, *chg_b;          // the two chunk-change maps
  uint8_t *chg_ta, *chg_tb;        // the two per-trace change maps
  // worker pools (des_workers.h; null unless ItemDims::pooled): per row its workers; a pooled round's
  // segment starts and lengths, the tiles' last segment starts, and the round's order refined into rank
  // classes: segment keys, rows, items, maps
  uint32_t *d_row_workers, *wk_start, *wk_len, *wk_tile, *wk_seg, *wk_row, *wk_sid;
  dit::MP *wk_mp;
};
inline void des_items_layout(Arena &a, ItemBufs &b, const ItemDims &d) {
  const uint64_t M = d.M, ops = M * d.bw, kept = d.cyclic ? M : 0;
  for (uint32_t **p : {&b.ipos, &b.ipar, &b.itr, &b.ihop, &b.inv, &b.qids, &b.fids, &b.val_a, &b.val_b, &b.rk_a,
                       &b.rk_b, &b.rv_a, &b.rv_b, &b.sid})
    *p = a.take<uint32_t>(M);
  for (uint64_t **p : {&b.IA, &b.IS, &b.IF, &b.key_a, &b.key_b}) *p = a.take<uint64_t>(M);
  for (dit::MP **p : {&b.mp_in, &b.mp_out}) *p = a.take<dit::MP>(M);
  b.iown = a.take<uint8_t>(M);
  b.irep = a.take<uint16_t>(M);
  b.erec = a.take<dit::ItemRec>(M);
  b.acc = a.take<uint64_t>(M * d.aw);
  b.bk = a.take<uint64_t>(M * (d.bw ? d.bw : 1));
  b.acc_b = a.take<uint64_t>(kept * d.aw);
  b.ord = a.take<uint32_t>(kept);
  b.ordc = a.take<uint16_t>(kept);
  b.ifst = a.take<uint32_t>(d.modeb ? M : 0);
  for (uint32_t **p : {&b.op_k, &b.op_k2}) *p = a.take<uint32_t>(ops);
  for (unsigned long long **p : {&b.op_v, &b.op_v2}) *p = a.take<unsigned long long>(ops);
  b.d_soff = a.take<uint32_t>(d.R + 1);
  b.qstate = a.take<dit::QState>((M + dit::kQTile - 1) / dit::kQTile);
  b.qticket = a.take<uint32_t>(1);
  b.ovf = a.take<uint32_t>(4);
  b.mm = a.take<uint64_t>(8);
  b.chg = a.take<uint32_t>(2);
  b.d_row_hold = a.take<uint64_t>(d.rows_n);
  b.troot = a.take<uint32_t>(d.n);
  b.d_poff = a.take<uint32_t>(d.n_pos + 1);
  for (uint32_t **p : {&b.d_qdst, &b.d_fdst}) *p = a.take<uint32_t>(d.n_pos);
  b.tmp = a.take<char>(d.tmp_bytes);
  for (uint8_t **p : {&b.chg_a, &b.chg_b}) *p = a.take<uint8_t>(d.n_chunks());
  for (uint8_t **p : {&b.chg_ta, &b.chg_tb}) *p = a.take<uint8_t>(d.n + 1);
  // worker pools: nothing unless some service has more than one worker
  // (not even an empty part: the allocation is the same to the byte)
  b.d_row_workers = b.wk_start = b.wk_len = b.wk_seg = b.wk_row = b.wk_sid = b.wk_tile = nullptr;
  b.wk_mp = nullptr;
  if (!d.pooled) return;
  b.d_row_workers = a.take<uint32_t>(d.rows_n);
  for (uint32_t **p : {&b.wk_start, &b.wk_len, &b.wk_seg, &b.wk_row, &b.wk_sid}) *p = a.take<uint32_t>(M);
  b.wk_tile = a.take<uint32_t>((M + dit::kWkTile - 1) / dit::kWkTile + 1);
  b.wk_mp = a.take<dit::MP>(M);
}

}  // namespace isim
