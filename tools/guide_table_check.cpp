// tools/guide_table_check.cpp — the guide table validator (csrc/guide_table.cpp) under the host sanitizers.
//
// A stand-alone CPU program: it feeds guide_table_check the malformed tables of tests/test_guide_host.py, each in
// arrays of exactly the declared size on the heap, so that a read past an array while rejecting a table is an
// AddressSanitizer report.  Host only; nothing here touches a GPU.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Idistributed_inference_demo_amd/csrc tools/guide_table_check.cpp \
//       distributed_inference_demo_amd/csrc/guide_table.cpp -o tools/guide_table_check && tools/guide_table_check
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "guide_table.h"

namespace {

struct Case {
  const char* name;
  int n_states, start;
  std::vector<int> row_ptr, tok, nxt, dn;
  int vocab;
  const char* expect;  // a piece of the message; nullptr: the table is valid
};

// Exact-size heap copies: the validator must stay inside them.
std::unique_ptr<int[]> heap(const std::vector<int>& v) {
  std::unique_ptr<int[]> p(new int[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}

}  // namespace

int main() {
  const int V = 64;
  const std::vector<Case> cases = {
      {"smallest default-allow", 1, 0, {0, 0}, {}, {}, {0}, 1, nullptr},
      {"smallest default-ban", 1, 0, {0, 1}, {0}, {0}, {-1}, 1, nullptr},
      {"two states", 2, 1, {0, 2, 3}, {3, 9, 5}, {1, -1, 0}, {-1, 1}, V, nullptr},
      {"n_states = 0", 0, 0, {0}, {}, {}, {}, V, "n_states"},
      {"n_states > 2^20", (1 << 20) + 1, 0, {0}, {}, {}, {}, V, "n_states"},
      {"start", 1, 1, {0, 1}, {5}, {0}, {-1}, V, "start"},
      {"negative start", 1, -1, {0, 1}, {5}, {0}, {-1}, V, "start"},
      {"row_ptr[0]", 1, 0, {1, 1}, {5}, {0}, {0}, V, "start at 0"},
      {"row_ptr decreases", 2, 0, {0, 1, 0}, {5}, {0}, {0, 0}, V, "decreases at state 1"},
      {"descending tokens", 2, 0, {0, 0, 2}, {6, 5}, {0, 0}, {0, -1}, V, "ascending in state 1"},
      {"a token twice", 1, 0, {0, 2}, {5, 5}, {0, 0}, {-1}, V, "ascending in state 0"},
      {"token = vocab", 1, 0, {0, 1}, {V}, {0}, {-1}, V, "vocab) in state 0"},
      {"negative token", 1, 0, {0, 1}, {-1}, {0}, {0}, V, "vocab) in state 0"},
      {"edge_next = n_states", 2, 0, {0, 0, 1}, {5}, {2}, {0, -1}, V, "edge_next"},
      {"edge_next < -1", 1, 0, {0, 1}, {5}, {-2}, {0}, V, "edge_next"},
      {"default_next = n_states", 2, 0, {0, 0, 0}, {}, {}, {0, 2}, V, "default_next"},
      {"default_next < -1", 1, 0, {0, 0}, {}, {}, {-2}, V, "default_next"},
      {"default-ban, no allowed edge", 2, 0, {0, 1, 2}, {5, 5}, {0, -1}, {-1, -1}, V, "no token is allowed in state 1"},
      {"default-allow, every token banned", 1, 0, {0, 4}, {0, 1, 2, 3}, {-1, -1, -1, -1}, {0}, 4, "no token is allowed in state 0"},
  };
  int failed = 0;
  for (const Case& c : cases) {
    auto rp = heap(c.row_ptr), tk = heap(c.tok), nx = heap(c.nxt), dn = heap(c.dn);
    const bs_guide_desc d{c.n_states, c.start, rp.get(), tk.get(), nx.get(), dn.get()};
    std::string msg;
    const bool ok = guide_table_check(&d, c.vocab, &msg);
    const bool good = c.expect ? (!ok && msg.find(c.expect) != std::string::npos) : ok;
    std::printf("%-36s %s%s%s\n", c.name, good ? "ok" : "FAILED", msg.empty() ? "" : ": ", msg.c_str());
    failed += !good;
  }
  std::string msg;
  if (guide_table_check(nullptr, V, &msg)) failed++;
  return failed ? 1 : 0;
}
