// The service timeline's host fold (csrc/service_timeline.h) as a stand-alone host program:
// svt::fold_host, the loop isim_service_timeline_host runs, over the hand-derived vectors of
// tests/golden/service_timeline_kat.json (argv[1]): each case into a zeroed table, twice into one table,
// next to refused spans, and as one of two services.
// tests/test_service_timeline_check.py builds it with -fsanitize=address,undefined and runs it on the CPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "json.h"
#include "service_timeline.h"

using namespace isim;

namespace {

int fails = 0;
void expect(bool ok, const std::string &what) {
  if (!ok) {
    ++fails;
    std::printf("FAIL %s\n", what.c_str());
  }
}

const JVal &field(const JVal &o, const char *name) {
  for (const auto &kv : o.obj)
    if (kv.first == name) return kv.second;
  std::printf("no field %s\n", name);
  std::exit(2);
}
uint64_t num(const JVal &v) { return std::strtoull(v.s.c_str(), nullptr, 10); }

struct Case {
  std::string name;
  isim_timeline_params p{};
  uint64_t hold = 0;
  std::vector<isim_des_span> spans;
  std::vector<uint64_t> table;  // one service: [n_windows + 2][kW], then the header
};

// the fold of `spans` for n_services services of the case's hold into `table` (added into)
void fold(const Case &k, uint32_t n_services, const std::vector<isim_des_span> &spans, std::vector<uint64_t> &table) {
  svt::RowArgs a{};
  tl::set_row_args(a, k.p);
  const std::vector<uint64_t> hold(n_services, k.hold);
  std::vector<uint64_t> cover(2 * svt::cells_of(n_services, k.p.n_windows), 0xABABABABABABABABull);  // dirty
  svt::fold_host(a, n_services, hold.data(), spans.data(), spans.size(), table.data(), cover.data());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string text = ss.str();
  JVal doc;
  std::string err;
  if (!json_parse(text.data(), text.size(), doc, err)) {
    std::printf("fixture: %s\n", err.c_str());
    return 2;
  }
  std::vector<Case> cases;
  for (const JVal &c : field(doc, "cases").arr) {
    Case k;
    k.name = field(c, "name").s;
    k.p.t0_ns = num(field(c, "t0"));
    k.p.window_ns = num(field(c, "window"));
    k.p.n_windows = (uint32_t)num(field(c, "n_windows"));
    k.hold = num(field(c, "hold"));
    for (const JVal &r : field(c, "spans").arr) {
      isim_des_span s{};
      s.arrival_ns = num(r.arr[0]);
      s.start_ns = num(r.arr[1]);
      s.finish_ns = num(r.arr[2]);
      s.status = (uint32_t)num(r.arr[3]);
      k.spans.push_back(s);
    }
    const uint64_t cells = svt::cells_of(1, k.p.n_windows);
    k.table.assign(svt::table_words(cells), 0);
    for (const JVal &w : field(c, "cells").arr) k.table[num(w.arr[0]) * svt::kW + num(w.arr[1])] = num(w.arr[2]);
    k.table[cells * svt::kW + ISIM_SVT_H_FOLDED] = num(field(c, "header").arr[0]);
    k.table[cells * svt::kW + ISIM_SVT_H_REFUSED] = num(field(c, "header").arr[1]);
    cases.push_back(k);
  }
  expect(cases.size() == 2, "two cases");

  for (const Case &k : cases) {
    expect(tl::params_error(&k.p) == nullptr, k.name + ": parameters");
    const uint64_t cells = svt::cells_of(1, k.p.n_windows), words = svt::table_words(cells);
    // into a zeroed table: as derived by hand
    std::vector<uint64_t> t(words, 0);
    fold(k, 1, k.spans, t);
    expect(t == k.table, k.name + ": table");
    for (size_t i = 0; i < t.size(); ++i)
      if (t[i] != k.table[i])
        std::printf("  word %zu: %llu, want %llu\n", i, (unsigned long long)t[i], (unsigned long long)k.table[i]);
    // again into the same table: every word doubles but the maxima
    fold(k, 1, k.spans, t);
    bool doubled = true;
    for (uint64_t i = 0; i < words; ++i)
      doubled &= t[i] == (i < cells * svt::kW && i % svt::kW == ISIM_SVT_MAX_WAIT ? k.table[i] : 2 * k.table[i]);
    expect(doubled, k.name + ": twice");
    // refused spans between the good ones: counted in the header, nothing else moves
    std::vector<isim_des_span> mixed;
    for (const isim_des_span &s : k.spans) {
      isim_des_span bad = s;
      bad.service = 1;  // out of range for one service
      mixed.push_back(bad);
      mixed.push_back(s);
      bad = s;
      bad.start_ns = s.arrival_ns - 1;  // S < a (wraps to the top for a = 0: then S > F)
      mixed.push_back(bad);
      bad = s;
      bad.service = 0xFFFFFFFFu;
      bad.finish_ns = s.start_ns - 1;  // F < S
      mixed.push_back(bad);
    }
    std::vector<uint64_t> m(words, 0), want = k.table;
    want[cells * svt::kW + ISIM_SVT_H_REFUSED] = 3 * k.spans.size();
    fold(k, 1, mixed, m);
    expect(m == want, k.name + ": refused spans");
    // as the second of two services: the first service's rows stay zero
    std::vector<isim_des_span> second = k.spans;
    for (isim_des_span &s : second) s.service = 1;
    std::vector<uint64_t> two(svt::table_words(2 * cells), 0), want2(svt::table_words(2 * cells), 0);
    for (uint64_t i = 0; i < words; ++i) want2[cells * svt::kW + i] = k.table[i];
    fold(k, 2, second, two);
    expect(two == want2, k.name + ": second service");
    // no span at all
    std::vector<uint64_t> none(words, 7);
    fold(k, 1, {}, none);
    expect(none == std::vector<uint64_t>(words, 7), k.name + ": no span");
  }
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails != 0;
}
