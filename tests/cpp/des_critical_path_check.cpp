// The DES critical path fold (csrc/des_critical_path.h) as a stand-alone host program:
// dcp::fold_list, the loop isim_des_critical_path_host runs, over the hand-derived traces of
// tests/golden/des_critical_path_kat.json (argv[1]): each case alone, the three as one list, and every
// corruption of every case, each refused and left untouched next to an intact neighbour.
// tests/test_des_critical_path_check.py builds it with -fsanitize=address,undefined and runs it on the CPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "des_critical_path.h"
#include "json.h"

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
  std::vector<isim_des_span> spans;
  std::vector<uint64_t> table;
  std::vector<uint32_t> critical;
  uint64_t trace_wait;
};

// the fixture's graph: e = sleep 1 ms, {a | b}, c;  a sleeps 2 ms, b and c 1 ms (critical_path.h's flat scripts)
const std::vector<uint32_t> kCmdOff = {0, 5, 6, 7, 8};
const std::vector<uint64_t> kCmds = {1000000, cp::kCmdConc | 2, cp::kCmdCall, cp::kCmdCall, cp::kCmdCall,
                                     2000000, 1000000,          1000000};
// TreeNode words: size | k << 16 of positions e, a, b, c
const std::vector<uint64_t> kNodes = {4ull, 1ull | (0ull << 16), 1ull | (1ull << 16), 1ull | (2ull << 16)};
constexpr uint32_t kServices = 4, kWords = (kServices + 1) * ISIM_DCP_ROW_WORDS;

struct Result {
  std::vector<isim_des_span> spans;
  std::vector<uint64_t> table, wait;
};
Result fold(std::vector<isim_des_span> spans, const std::vector<uint64_t> &off) {
  const cp::ScriptView v{kCmdOff.data(), kCmds.data(), kServices, 4};
  Result r{std::move(spans), std::vector<uint64_t>(kWords, 0), std::vector<uint64_t>(off.size() - 1, 0x1111)};
  dcp::fold_list(v, cp::K8{kNodes.data()}, off.data(), off.size() - 1, r.spans.data(), r.table.data(), r.wait.data());
  return r;
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
    for (const JVal &r : field(c, "spans").arr) {  // arrival, start, finish, hop_ns, hop, caller, position, site, service, status
      isim_des_span s{};
      s.arrival_ns = num(r.arr[0]);
      s.start_ns = num(r.arr[1]);
      s.finish_ns = num(r.arr[2]);
      s.hop_ns = num(r.arr[3]);
      s.hop = (uint32_t)num(r.arr[4]);
      s.caller_hop = (uint32_t)num(r.arr[5]);
      s.position = (uint32_t)num(r.arr[6]);
      s.slot = (uint32_t)num(r.arr[7]);
      s.service = (uint32_t)num(r.arr[8]);
      s.status = (uint32_t)num(r.arr[9]);
      k.spans.push_back(s);
    }
    for (const JVal &row : field(c, "table").arr)
      for (const JVal &w : row.arr) k.table.push_back(num(w));
    for (const JVal &b : field(c, "critical").arr) k.critical.push_back((uint32_t)num(b));
    k.trace_wait = num(field(c, "trace_wait"));
    cases.push_back(k);
  }
  expect(cases.size() == 3, "three cases");

  // each case alone: table, bits and the trace's critical wait as derived by hand
  std::vector<isim_des_span> all;
  std::vector<uint64_t> all_off = {0}, sum(kWords, 0);
  for (const Case &k : cases) {
    const Result r = fold(k.spans, {0, k.spans.size()});
    expect(r.table == k.table, k.name + ": table");
    expect(r.wait[0] == k.trace_wait, k.name + ": trace wait");
    for (size_t j = 0; j < k.spans.size(); ++j)
      expect(r.spans[j].status == (k.spans[j].status | (k.critical[j] ? ISIM_SPAN_CRITICAL : 0u)), k.name + ": bit");
    all.insert(all.end(), k.spans.begin(), k.spans.end());
    all_off.push_back(all.size());
    for (uint32_t w = 0; w < kWords; ++w) sum[w] += k.table[w];
  }
  // the three as one list
  expect(fold(all, all_off).table == sum, "one list: table");

  // corruptions: the damaged case in the middle of a list of three, refused and untouched; its neighbours folded
  using Damage = std::function<void(std::vector<isim_des_span> &)>;
  const std::vector<std::pair<const char *, Damage>> damages = {
      {"a wrong hop", [](auto &s) { s[1].hop = 2; }},
      {"a forward caller_hop", [](auto &s) { s[1].caller_hop = 2; }},
      {"a caller_hop far out of range", [](auto &s) { s.back().caller_hop = 0xFFFFFFF0u; }},
      {"S < a", [](auto &s) { s[2].start_ns = s[2].arrival_ns - 1; }},
      {"F < S", [](auto &s) { s.back().finish_ns = s.back().start_ns - 1; }},
      {"a child's arrival off by one", [](auto &s) { s[1].arrival_ns -= 1; }},
      {"a position out of range", [](auto &s) { s.back().position = 0x7FFFFFFFu; }},
      {"a service out of range", [](auto &s) { s.back().service = kServices; }},
      {"a negative self", [](auto &s) { s[0].finish_ns = s[0].start_ns + 1; }},
      {"an entry with a hop cost", [](auto &s) { s[0].hop_ns = 1; }},
  };
  for (const Case &k : cases)
    for (const auto &d : damages) {
      std::vector<isim_des_span> bad = k.spans;
      d.second(bad);
      const Case &n = cases[0];
      std::vector<isim_des_span> list = n.spans;
      list.insert(list.end(), bad.begin(), bad.end());
      list.insert(list.end(), n.spans.begin(), n.spans.end());
      const size_t a = n.spans.size(), b = a + bad.size();
      const Result r = fold(list, {0, a, b, list.size()});
      const std::string what = k.name + ": " + d.first;
      expect(r.wait[1] == UINT64_MAX && r.wait[0] == n.trace_wait && r.wait[2] == n.trace_wait, what + ": waits");
      expect(std::memcmp(r.spans.data() + a, bad.data(), bad.size() * sizeof(isim_des_span)) == 0, what + ": untouched");
      std::vector<uint64_t> want(kWords, 0);
      for (uint32_t w = 0; w < kWords; ++w) want[w] = 2 * n.table[w];
      want[kServices * ISIM_DCP_ROW_WORDS + ISIM_DCP_H_REFUSED] = 1;
      expect(r.table == want, what + ": table");
    }
  // offsets out of order: the middle entry runs backwards, its neighbours reach into each other's spans
  {
    const Case &n = cases[0];
    std::vector<isim_des_span> list = n.spans;
    list.insert(list.end(), n.spans.begin(), n.spans.end());
    const Result r = fold(list, {0, 2 * n.spans.size(), n.spans.size(), 2 * n.spans.size()});
    expect(r.wait[0] == UINT64_MAX && r.wait[1] == UINT64_MAX && r.wait[2] == n.trace_wait, "offsets out of order");
    expect(r.table[kServices * ISIM_DCP_ROW_WORDS + ISIM_DCP_H_REFUSED] == 2, "offsets out of order: counted");
  }
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails != 0;
}
