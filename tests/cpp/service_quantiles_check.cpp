// The per-service percentiles' host fold (csrc/service_quantiles.h) as a stand-alone host
// program: svq::fold_host, the loop isim_service_quantiles_host runs, over the hand-derived vectors of
// tests/golden/service_quantiles_kat.json (argv[1]): each case into a dirty table, with its spans reversed,
// next to further refused spans, with empty services in front, and with no span at all.
// tests/test_service_quantiles_check.py builds it with -fsanitize=address,undefined and runs it on the CPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "json.h"
#include "service_quantiles.h"

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
  uint32_t n_services = 0;
  std::vector<uint32_t> ppm;
  std::vector<isim_des_span> spans;
  std::vector<uint64_t> table;
};

std::vector<uint64_t> fold(uint32_t n_services, const std::vector<uint32_t> &ppm, const std::vector<isim_des_span> &spans) {
  std::vector<uint64_t> t(svq::table_words(n_services, (uint32_t)ppm.size()), 0xABABABABABABABABull);  // dirty
  svq::fold_host(n_services, ppm.data(), (uint32_t)ppm.size(), spans.data(), spans.size(), t.data());
  return t;
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
    k.n_services = (uint32_t)num(field(c, "n_services"));
    for (const JVal &q : field(c, "q_ppm").arr) k.ppm.push_back((uint32_t)num(q));
    for (const JVal &r : field(c, "spans").arr) {
      isim_des_span s{};
      s.arrival_ns = num(r.arr[0]);
      s.start_ns = num(r.arr[1]);
      s.finish_ns = num(r.arr[2]);
      s.service = (uint32_t)num(r.arr[3]);
      s.status = (uint32_t)num(r.arr[4]);
      k.spans.push_back(s);
    }
    const uint64_t ow = svq::cell_words((uint32_t)k.ppm.size());
    k.table.assign(svq::table_words(k.n_services, (uint32_t)k.ppm.size()), 0);
    for (const JVal &w : field(c, "cells").arr) {
      expect(w.arr.size() == 3 + ow, k.name + ": a cell's words");
      const uint64_t base = ((num(w.arr[0]) * svq::kMeasures + num(w.arr[1])) * svq::kClasses + num(w.arr[2])) * ow;
      for (uint64_t i = 0; i < ow; ++i) k.table[base + i] = num(w.arr[3 + i]);
    }
    k.table[k.table.size() - 2 + ISIM_SVQ_H_FOLDED] = num(field(c, "header").arr[0]);
    k.table[k.table.size() - 2 + ISIM_SVQ_H_REFUSED] = num(field(c, "header").arr[1]);
    cases.push_back(k);
  }
  expect(cases.size() == 2, "two cases");

  for (const Case &k : cases) {
    const uint32_t n_q = (uint32_t)k.ppm.size();
    expect(q::list_error(k.ppm.data(), n_q).empty(), k.name + ": quantile list");
    // into a dirty table: as derived by hand, every word written
    const std::vector<uint64_t> t = fold(k.n_services, k.ppm, k.spans);
    expect(t == k.table, k.name + ": table");
    for (size_t i = 0; i < t.size(); ++i)
      if (t[i] != k.table[i])
        std::printf("  word %zu: %llu, want %llu\n", i, (unsigned long long)t[i], (unsigned long long)k.table[i]);
    // order statistics do not depend on the order of the spans
    std::vector<isim_des_span> rev(k.spans.rbegin(), k.spans.rend());
    expect(fold(k.n_services, k.ppm, rev) == k.table, k.name + ": reversed");
    // further refused spans between the others: counted in the header, nothing else moves
    std::vector<isim_des_span> mixed;
    for (const isim_des_span &s : k.spans) {
      isim_des_span bad = s;
      bad.service = k.n_services;  // out of range
      mixed.push_back(bad);
      mixed.push_back(s);
      bad = s;
      bad.service = 0;
      bad.arrival_ns = 9;
      bad.start_ns = 8;  // S < a
      bad.finish_ns = 10;
      mixed.push_back(bad);
      bad.service = 0xFFFFFFFFu;
      bad.start_ns = 11;  // F < S
      mixed.push_back(bad);
    }
    std::vector<uint64_t> want = k.table;
    want[want.size() - 2 + ISIM_SVQ_H_REFUSED] += 3 * k.spans.size();
    expect(fold(k.n_services, k.ppm, mixed) == want, k.name + ": refused spans");
    // two empty services in front: their cells are zero, the others move up
    std::vector<isim_des_span> moved = k.spans;
    for (isim_des_span &s : moved)
      if (s.service < k.n_services) s.service += 2;
      else s.service = k.n_services + 2;
    const uint64_t per = svq::kMeasures * svq::kClasses * svq::cell_words(n_q);
    std::vector<uint64_t> want2(svq::table_words(k.n_services + 2, n_q), 0);
    std::copy(k.table.begin(), k.table.end(), want2.begin() + 2 * per);
    expect(fold(k.n_services + 2, k.ppm, moved) == want2, k.name + ": empty services in front");
    // no span at all: zeros
    expect(fold(k.n_services, k.ppm, {}) == std::vector<uint64_t>(k.table.size(), 0), k.name + ": no span");
  }
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails != 0;
}
