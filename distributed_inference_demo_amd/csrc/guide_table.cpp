// guide_table.cpp — host-side check of a guide's tables (guide_table.h).  Plain C++, no HIP.
#include "guide_table.h"

bool guide_table_check(const bs_guide_desc* g, int vocab, std::string* msg) {
  auto bad = [&](const std::string& m) {
    if (msg) *msg = m;
    return false;
  };
  if (!g) return bad("guide is NULL");
  const int n = g->n_states;
  if (n < 1 || n > BS_GUIDE_MAX_STATES) return bad("n_states must be in [1, 2^20]");
  if (!g->row_ptr || !g->default_next) return bad("row_ptr / default_next is NULL");
  if (g->start < 0 || g->start >= n) return bad("start state outside [0, n_states)");
  if (g->row_ptr[0] != 0) return bad("row_ptr must start at 0 (state 0)");
  for (int q = 0; q < n; q++)
    if (g->row_ptr[q + 1] < g->row_ptr[q]) return bad("row_ptr decreases at state " + std::to_string(q));
  if (g->row_ptr[n] > 0 && (!g->edge_token || !g->edge_next)) return bad("edge_token / edge_next is NULL");
  for (int q = 0; q < n; q++) {
    const std::string at = " in state " + std::to_string(q);
    const int dn = g->default_next[q];
    if (dn < -1 || dn >= n) return bad("default_next outside [-1, n_states)" + at);
    long long allowed = dn >= 0 ? vocab : 0;
    for (int e = g->row_ptr[q]; e < g->row_ptr[q + 1]; e++) {
      const int t = g->edge_token[e], nx = g->edge_next[e];
      if (t < 0 || t >= vocab) return bad("edge token outside [0, vocab)" + at);
      if (e > g->row_ptr[q] && t <= g->edge_token[e - 1]) return bad("edge tokens not strictly ascending" + at);
      if (nx < -1 || nx >= n) return bad("edge_next outside [-1, n_states)" + at);
      if (dn >= 0 && nx < 0) allowed--;
      if (dn < 0 && nx >= 0) allowed++;
    }
    if (allowed <= 0) return bad("no token is allowed" + at);
  }
  return true;
}
