// CPU check of the DES engines' workspace layouts (csrc/des_layout.h): for the
// product's plan of a graph file (build_des_plan) and a grid of item-engine
// sizes, the sizing run and the carving run of each layout function agree,
// every part is 256-byte aligned, inside the allocation, large enough for its
// elements and disjoint from every other part (declared aliases exempt).
// Prints the sizes with stand-in rocPRIM temporary sizes (sort 4096, scan
// 1024): tests/test_des_layout.py pins them.  Plain C++, no HIP.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "des_layout.h"
#include "graph.h"
#include "kernel_abi.h"
#include "program.h"

using namespace isim;

namespace {

struct Part {
  const char *name;
  const void *p;
  uint64_t bytes;  // elements x element size the engine uses
};
#define PART(b, m, count) Part{#m, (b).m, (uint64_t)(count) * sizeof(*(b).m)}

int g_bad = 0;
void bad(const std::string &what, const char *part, const char *why) {
  std::fprintf(stderr, "%s: %s: %s\n", what.c_str(), part, why);
  ++g_bad;
}

// `parts` were carved from [base, base + total)
void check(const std::string &what, const char *base, uint64_t sized, uint64_t total, std::vector<Part> parts) {
  if (sized != total) bad(what, "total", "the sizing run and the carving run differ");
  for (const Part &q : parts) {
    const char *p = (const char *)q.p;
    if (!p) {
      if (q.bytes) bad(what, q.name, "null");
      continue;
    }
    if ((uintptr_t)(p - base) % 256) bad(what, q.name, "not 256-byte aligned");
    if (p < base || p + q.bytes > base + total) bad(what, q.name, "outside the allocation");
  }
  parts.erase(std::remove_if(parts.begin(), parts.end(), [](const Part &q) { return !q.p || !q.bytes; }), parts.end());
  std::sort(parts.begin(), parts.end(), [](const Part &x, const Part &y) { return x.p < y.p; });
  for (size_t i = 0; i + 1 < parts.size(); ++i)
    if ((const char *)parts[i].p + parts[i].bytes > (const char *)parts[i + 1].p)
      bad(what, parts[i].name, (std::string("overlaps ") + parts[i + 1].name).c_str());
}

struct Alloc {
  char *p;
  explicit Alloc(uint64_t bytes) : p((char *)std::aligned_alloc(256, bytes ? bytes : 256)) {}
  ~Alloc() { std::free(p); }
};

uint64_t check_static(const DesPlan &pl, uint64_t n, uint64_t words, uint64_t rows) {
  const uint64_t sort_tmp = (uint64_t)pl.max_sort_pos * n ? 4096 : 0;
  Arena sizing;
  DesBufs b;
  des_layout(sizing, b, pl, n, words, rows, sort_tmp);
  Alloc mem(sizing.bytes());
  Arena carving(mem.p);
  des_layout(carving, b, pl, n, words, rows, sort_tmp);
  const uint64_t np = pl.pos.size(), ld = des_row_ld(n), m = (uint64_t)pl.max_sort_pos * n;
  std::vector<Part> parts = {
      {"W", b.W, np * ld * 8}, {"WF", b.WF, np * ld * 8}, {"BK", b.BK, pl.steps.size() * ld * 8},
      PART(b, A, n), PART(b, E, n), PART(b, blk, (n + 8191) / 8192 + 1), PART(b, tickets, 4 * pl.rounds()),
      PART(b, prog, np), PART(b, chain, np * ((n + 4095) / 4096)), PART(b, ovf, 2),
      PART(b, stage, words + rows * ISIM_DES_ROW_WORDS), PART(b, stbits, np * des_status_wpr(n)),
      PART(b, keys_a, m), PART(b, keys_b, m), PART(b, vals_a, m), PART(b, vals_b, m),
      {"sort_tmp", b.sort_tmp, sort_tmp}};
  const std::string what = "static n=" + std::to_string(n);
  check(what, mem.p, sizing.bytes(), carving.bytes(), parts);
  if (b.changed != b.ovf + 1) bad(what, "changed", "not the word behind ovf");  // the declared alias
  if ((const char *)b.chain + np * ((n + 4095) / 4096) * sizeof(dev::ChainState) !=
      (const char *)b.tickets + b.pass_zero_bytes)
    bad(what, "pass_zero_bytes", "does not end with the chain states");
  return sizing.bytes();
}

uint64_t check_trace(uint64_t n) {
  Arena sizing;
  ItemTraceBufs b;
  des_items_trace_layout(sizing, b, n, 1024);
  Alloc mem(sizing.bytes());
  Arena carving(mem.p);
  des_items_trace_layout(carving, b, n, 1024);
  check("items per trace n=" + std::to_string(n), mem.p, sizing.bytes(), carving.bytes(),
        {PART(b, gap, n), PART(b, A, n), PART(b, cnt, n), PART(b, tend, n), PART(b, terr, n), PART(b, work, 2),
         {"scan_tmp", b.scan_tmp, 1024}});
  return sizing.bytes();
}

void check_items(const ItemDims &d) {
  Arena sizing;
  ItemBufs b;
  des_items_layout(sizing, b, d);
  Alloc mem(sizing.bytes());
  Arena carving(mem.p);
  des_items_layout(carving, b, d);
  const uint64_t M = d.M, ops = M * d.bw, cyc = d.cyclic ? M : 0;
  check("items M=" + std::to_string(M) + " n=" + std::to_string(d.n) + " bw=" + std::to_string(d.bw) +
            (d.cyclic ? " cyclic" : "") + (d.modeb ? " mode B" : ""),
        mem.p, sizing.bytes(), carving.bytes(),
        {PART(b, ipos, M), PART(b, ipar, M), PART(b, itr, M), PART(b, ihop, M), PART(b, iown, M), PART(b, IA, M),
         PART(b, IS, M), PART(b, IF, M), PART(b, acc, M * d.aw), PART(b, bk, ops), PART(b, acc_b, cyc * d.aw),
         PART(b, irep, M), PART(b, ifst, d.modeb ? M : 0), PART(b, erec, M), PART(b, inv, M), PART(b, troot, d.n),
         PART(b, op_k, ops), PART(b, op_k2, ops), PART(b, d_soff, d.R + 1), PART(b, op_v, ops), PART(b, op_v2, ops),
         PART(b, qids, M), PART(b, fids, M), PART(b, ord, cyc), PART(b, ordc, cyc), PART(b, key_a, M),
         PART(b, key_b, M), PART(b, val_a, M), PART(b, val_b, M), PART(b, rk_a, M), PART(b, rk_b, M),
         PART(b, rv_a, M), PART(b, rv_b, M), PART(b, sid, M), PART(b, mp_in, M), PART(b, mp_out, M),
         PART(b, qstate, (M + 511) / 512), PART(b, qticket, 1), PART(b, ovf, 4), PART(b, mm, 8), PART(b, chg, 2),
         PART(b, d_row_hold, d.rows_n), PART(b, d_poff, d.n_pos + 1), PART(b, d_qdst, d.n_pos),
         PART(b, d_fdst, d.n_pos), {"tmp", b.tmp, d.tmp_bytes}, PART(b, chg_a, d.n_chunks()),
         PART(b, chg_b, d.n_chunks()), PART(b, chg_ta, d.n), PART(b, chg_tb, d.n)});
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string js = ss.str();
  ServiceGraph g;
  std::string err;
  if (!unmarshal_service_graph(js.data(), js.size(), g, err)) {
    std::fprintf(stderr, "parse: %s\n", err.c_str());
    return 2;
  }
  int32_t entry = -1;
  for (size_t i = 0; i < g.services.size() && entry < 0; ++i)
    if (g.services[i].is_entrypoint) entry = (int32_t)i;
  isim_params prm{};
  prm.hop_base_ns = 500000;
  prm.error_mode = ISIM_MODE_A;
  Program prog;
  if (compile_program(g, entry, prm, prog, err) != ISIM_OK) {
    std::fprintf(stderr, "compile: %s\n", err.c_str());
    return 2;
  }
  DesPlan pl;
  if (build_des_plan(g, prog, false, pl, err) != ISIM_OK || pl.items) {
    std::fprintf(stderr, "plan: %s\n", err.c_str());
    return 3;
  }
  // the C ABI's stats words and table rows (handler.h stats_words)
  const uint64_t rows = prog.row_svc.size();
  const uint64_t words = ISIM_ST_SVC_DUR(prog.n_slots) + (uint64_t)ISIM_SVC_DUR_WORDS * (prog.static_walk ? 0 : rows);
  for (uint64_t n : {1ull, 255ull, 256ull, 4097ull, 5000ull})
    std::printf("static n=%llu bytes=%llu\n", (unsigned long long)n,
                (unsigned long long)check_static(pl, n, words, rows));
  for (uint64_t n : {1ull, 255ull, 256ull, 3000ull, 4097ull, 5000ull})
    std::printf("items n=%llu bytes=%llu\n", (unsigned long long)n, (unsigned long long)check_trace(n));
  for (uint64_t M : {0ull, 1ull, 511ull, 512ull, 513ull, 100000ull})
    for (uint64_t n : {1ull, 3000ull})
      for (int v = 0; v < 8; ++v)
        check_items(ItemDims{M, n, 2, (v & 1) ? 3u : 0u, 5, 7, 9, (v & 2) != 0, (v & 4) != 0, 4096, 8});
  if (g_bad) return 1;
  std::printf("layouts ok\n");
  return 0;
}
