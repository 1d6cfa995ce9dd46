// The per-service sketch's host fold (csrc/service_sketch.h) as a stand-alone host program:
// svs::fold_host, the loop isim_service_sketch_host runs, over the hand-derived vectors of
// tests/golden/service_sketch_kat.json (argv[1]): each case into zeros, twice into one table, into a table that
// holds counts already, with its spans reversed, next to further refused spans, with empty services in front,
// and with no span at all; and the bounds of every bin it hit.
// tests/test_service_sketch_check.py builds it with -fsanitize=address,undefined and runs it on the CPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "json.h"
#include "service_sketch.h"

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
  uint32_t n_services = 0, sub_bits = 0;
  std::vector<isim_des_span> spans;
  std::vector<uint64_t> table;
};

// the fold added into a copy of `into`, which is exactly as long as the table: a word past it is the sanitizer's
std::vector<uint64_t> fold(uint32_t n_services, uint32_t s, const std::vector<isim_des_span> &spans,
                           std::vector<uint64_t> into) {
  svs::fold_host(n_services, s, spans.data(), spans.size(), into.data());
  return into;
}
std::vector<uint64_t> zeros(uint32_t n_services, uint32_t s) {
  return std::vector<uint64_t>(svs::table_words(n_services, s), 0);
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
    k.sub_bits = (uint32_t)num(field(c, "sub_bits"));
    for (const JVal &r : field(c, "spans").arr) {
      isim_des_span s{};
      s.arrival_ns = num(r.arr[0]);
      s.start_ns = num(r.arr[1]);
      s.finish_ns = num(r.arr[2]);
      s.service = (uint32_t)num(r.arr[3]);
      s.status = (uint32_t)num(r.arr[4]);
      k.spans.push_back(s);
    }
    k.table = zeros(k.n_services, k.sub_bits);
    const uint64_t bins = sk::bins(k.sub_bits);
    for (const JVal &w : field(c, "words").arr) {
      expect(w.arr.size() == 5 && num(w.arr[3]) < bins, k.name + ": a word's fields");
      k.table[((num(w.arr[0]) * svs::kMeasures + num(w.arr[1])) * 2 + num(w.arr[2])) * bins + num(w.arr[3])] =
          num(w.arr[4]);
    }
    k.table[k.table.size() - 2 + ISIM_SVQ_H_FOLDED] = num(field(c, "header").arr[0]);
    k.table[k.table.size() - 2 + ISIM_SVQ_H_REFUSED] = num(field(c, "header").arr[1]);
    cases.push_back(k);
  }
  expect(cases.size() == 3, "three cases");

  for (const Case &k : cases) {
    const uint32_t ns = k.n_services, s = k.sub_bits;
    expect(svs::table_words(ns, s) == (uint64_t)ns * 6 * ((65ull - s) << s) + 2, k.name + ": table words");
    // into zeros: as derived by hand
    const std::vector<uint64_t> t = fold(ns, s, k.spans, zeros(ns, s));
    expect(t == k.table, k.name + ": table");
    for (size_t i = 0; i < t.size(); ++i)
      if (t[i] != k.table[i])
        std::printf("  word %zu: %llu, want %llu\n", i, (unsigned long long)t[i], (unsigned long long)k.table[i]);
    // accumulated into: twice into one table, and into a table whose every word holds 7 already
    std::vector<uint64_t> twice = k.table, sevens(k.table.size(), 7), plus7 = k.table;
    for (uint64_t &w : twice) w *= 2;
    for (uint64_t &w : plus7) w += 7;
    expect(fold(ns, s, k.spans, t) == twice, k.name + ": twice");
    expect(fold(ns, s, k.spans, sevens) == plus7, k.name + ": added into");
    // counts do not depend on the order of the spans
    std::vector<isim_des_span> rev(k.spans.rbegin(), k.spans.rend());
    expect(fold(ns, s, rev, zeros(ns, s)) == k.table, k.name + ": reversed");
    // further refused spans between the others: counted in the header, nothing else moves
    std::vector<isim_des_span> mixed;
    for (const isim_des_span &x : k.spans) {
      isim_des_span bad = x;
      bad.service = ns;  // out of range
      mixed.push_back(bad);
      mixed.push_back(x);
      bad = x;
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
    expect(fold(ns, s, mixed, zeros(ns, s)) == want, k.name + ": refused spans");
    // two empty services in front: their blocks are zero, the others move up
    std::vector<isim_des_span> moved = k.spans;
    for (isim_des_span &x : moved)
      if (x.service < ns) x.service += 2;
      else x.service = ns + 2;
    std::vector<uint64_t> want2 = zeros(ns + 2, s);
    std::copy(k.table.begin(), k.table.end(), want2.begin() + 2 * svs::kMeasures * svs::block_words(s));
    expect(fold(ns + 2, s, moved, zeros(ns + 2, s)) == want2, k.name + ": empty services in front");
    // no span at all: nothing is touched
    expect(fold(ns, s, {}, sevens) == sevens, k.name + ": no span");
    // every bin hit brackets its value: word_of and sk::bounds agree
    for (const isim_des_span &x : k.spans) {
      if (svq::span_refused(ns, x.arrival_ns, x.start_ns, x.finish_ns, x.service)) continue;
      for (uint32_t m = 0; m < svs::kMeasures; ++m) {
        const uint64_t v = svq::measure(m, x.arrival_ns, x.start_ns, x.finish_ns);
        const uint64_t w = svs::word_of(s, x.service, m, x.status & 1u, v);
        uint64_t lo = 0, hi = 0;
        sk::bounds(s, (uint32_t)(w % sk::bins(s)), lo, hi);
        expect(w < svs::table_words(ns, s) - 2 && lo <= v && v <= hi, k.name + ": a word's bounds");
      }
    }
  }
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails != 0;
}
