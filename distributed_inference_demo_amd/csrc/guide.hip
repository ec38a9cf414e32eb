// guide.hip — guided decoding: per-row token automata (include/bloomstage.h "Guided decoding").
//
// A guide is a DFA over token ids in CSR form (GuideDev); a KV row holds {guide, state, n_steps, n_rejected}
// (GuideRowDev).  Three kernels:
//   set      writes table rows from kernel arguments
//   apply    grid (ceil(V / kGuideSlice), B): block (x, b) owns tokens [x * slice, (x + 1) * slice) of row slot + b.  It
//            binary-searches the state's sorted edges for the ends of its slice.  Default-allow state: it stores
//            -FLT_MAX at the slice's explicit bans and nothing else, so the cost follows the edges, never V.
//            Default-ban state: it marks the slice's allowed tokens in an LDS bitmap (integer atomicOr), then stores
//            -FLT_MAX over the slice with 16-byte stores, reading a vector first only where it holds an allowed token.
//            Every logit has one writer, no block waits for another, allowed logits are never written with another value.
//   advance  block b, one thread: a binary search in the state's edges, then the default, per token, in order
// The launches and grids depend on (B, V) only; every per-call value comes from the device tables, so a captured graph
// stays valid while guides are loaded, unloaded, set and cleared.  A row without state returns at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kApplyThreads = 256;
constexpr int kAdvThreads = 64;
constexpr int kAdvArgIds = 512;  // host ids travel by kernel arguments, this many a launch
constexpr int kSetArgRows = 256;  // table rows a set launch carries by kernel arguments
static_assert(kGuideSlice % 32 == 0 && kGuideSlice % 4 == 0, "slice: whole bitmap words and whole 16-byte vectors");

struct GdStates { int v[kSetArgRows]; };
struct GdIds { int v[kAdvArgIds]; };

// First index in [lo, hi) whose entry is >= key (hi if none).
__device__ __forceinline__ int gd_lower_bound(const int* a, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The row's guide and state if both are usable (a cleared row, an unloaded guide or a state outside it: false).
__device__ __forceinline__ bool gd_row(const GuideBufs& gb, int row, GuideRowDev* r, GuideDev* g) {
  *r = gb.rows[row];
  if (r->guide < 0 || r->guide >= kGuideMax) return false;
  *g = gb.guides[r->guide];
  return r->state >= 0 && r->state < g->n_states;
}

__global__ void __launch_bounds__(kSetArgRows) guide_set_kernel(GuideBufs gb, int slot, int n, int guide, GdStates st) {
  const int i = threadIdx.x;
  if (i < n) gb.rows[slot + i] = GuideRowDev{guide, guide < 0 ? 0 : st.v[i], 0, 0};
}

__global__ void __launch_bounds__(kApplyThreads) guide_apply_kernel(GuideBufs gb, float* logits, int ld, int slot) {
  __shared__ uint32_t allow[kGuideSlice / 32];
  GuideRowDev r;
  GuideDev g;
  if (!gd_row(gb, slot + blockIdx.y, &r, &g)) return;  // uniform over the block
  const int tid = threadIdx.x, q = r.state;
  const int s0 = blockIdx.x * kGuideSlice, s1 = min(s0 + kGuideSlice, gb.V);
  float* l = logits + (size_t)blockIdx.y * ld;
  const int e0 = g.row_ptr[q], e1 = g.row_ptr[q + 1];
  const int lo = gd_lower_bound(g.edge_token, e0, e1, s0), hi = gd_lower_bound(g.edge_token, lo, e1, s1);
  if (g.default_next[q] >= 0) {  // default-allow: the slice's explicit bans, tokens in [s0, s1) by the search
    for (int e = lo + tid; e < hi; e += kApplyThreads)
      if (g.edge_next[e] < 0) l[g.edge_token[e]] = -FLT_MAX;
    return;
  }
  for (int i = tid; i < kGuideSlice / 32; i += kApplyThreads) allow[i] = 0u;
  __syncthreads();
  for (int e = lo + tid; e < hi; e += kApplyThreads)
    if (g.edge_next[e] >= 0) {
      const int t = g.edge_token[e] - s0;  // in [0, slice)
      atomicOr(&allow[t >> 5], 1u << (t & 31));
    }
  __syncthreads();
  const bool vec = ((uintptr_t)(l + s0) & 15) == 0;  // s0 is a multiple of 4: vector i starts at a 16-byte boundary
  for (int i = tid; i < kGuideSlice / 4; i += kApplyThreads) {
    const int t = s0 + 4 * i;
    if (t >= s1) break;
    const uint32_t m = (allow[i >> 3] >> ((i & 7) * 4)) & 0xFu;  // bit j: token t + j is allowed
    if (vec && t + 4 <= s1) {
      float4* p = reinterpret_cast<float4*>(l + t);
      float4 x = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
      if (m) {
        const float4 o = *p;
        if (m & 1u) x.x = o.x;
        if (m & 2u) x.y = o.y;
        if (m & 4u) x.z = o.z;
        if (m & 8u) x.w = o.w;
      }
      *p = x;
    } else {
      for (int j = 0; j < 4 && t + j < s1; j++)
        if (!((m >> j) & 1u)) l[t + j] = -FLT_MAX;
    }
  }
}

// One thread walks ids[0..n) through the row's state.
__device__ void gd_walk(const GuideBufs& gb, int row, const int* ids, int n) {
  GuideRowDev r;
  GuideDev g;
  if (!gd_row(gb, row, &r, &g)) return;
  int q = r.state, rej = 0;
  for (int i = 0; i < n; i++) {
    const int v = ids[i];
    int nx = -1;
    if (v >= 0 && v < gb.V) {
      const int e1 = g.row_ptr[q + 1];
      const int e = gd_lower_bound(g.edge_token, g.row_ptr[q], e1, v);
      nx = (e < e1 && g.edge_token[e] == v) ? g.edge_next[e] : g.default_next[q];
    }
    if (nx >= 0 && nx < g.n_states) q = nx; else rej++;
  }
  gb.rows[row] = GuideRowDev{r.guide, q, r.n_steps + n, r.n_rejected + rej};
}

// stride 0, grid 1: n device ids through one row.  stride 1, n 1: the tail's advance, block b steps row slot + b by
// tokens[b].
__global__ void __launch_bounds__(kAdvThreads) guide_advance_dev_kernel(GuideBufs gb, int slot, const int* ids, int stride,
                                                                        int n) {
  if (threadIdx.x == 0) gd_walk(gb, slot + blockIdx.x, ids + (size_t)blockIdx.x * stride, n);
}

__global__ void __launch_bounds__(kAdvThreads) guide_advance_args_kernel(GuideBufs gb, int row, GdIds ids, int n) {
  __shared__ int sid[kAdvArgIds];
  for (int i = threadIdx.x; i < kAdvArgIds; i += kAdvThreads) sid[i] = ids.v[i];
  __syncthreads();
  if (threadIdx.x == 0) gd_walk(gb, row, sid, min(n, kAdvArgIds));
}

}  // namespace

int guide_advance_arg_ids() { return kAdvArgIds; }

void launch_guide_set(const GuideBufs& gb, int slot, int n, int guide, const int* states, hipStream_t s) {
  for (int i = 0; i < n; i += kSetArgRows) {
    GdStates a{};
    const int c = std::min(kSetArgRows, n - i);
    for (int j = 0; j < c; j++) a.v[j] = states ? states[i + j] : 0;
    guide_set_kernel<<<1, kSetArgRows, 0, s>>>(gb, slot + i, c, guide, a);
  }
}

void launch_guide_apply(const GuideBufs& gb, float* logits, int ld, int slot, int B, hipStream_t s) {
  if (B <= 0) return;
  const dim3 grid((gb.V + kGuideSlice - 1) / kGuideSlice, B);
  guide_apply_kernel<<<grid, kApplyThreads, 0, s>>>(gb, logits, ld, slot);
}

void launch_guide_advance_picks(const GuideBufs& gb, int slot, int B, const int* tokens, hipStream_t s) {
  if (B <= 0) return;
  guide_advance_dev_kernel<<<B, kAdvThreads, 0, s>>>(gb, slot, tokens, 1, 1);
}

void launch_guide_advance(const GuideBufs& gb, int slot, const int* ids_host, const int* ids_dev, int n, hipStream_t s) {
  if (n <= 0) return;
  if (!ids_host) {
    guide_advance_dev_kernel<<<1, kAdvThreads, 0, s>>>(gb, slot, ids_dev, 0, n);
    return;
  }
  for (int i = 0; i < n; i += kAdvArgIds) {
    GdIds a;
    const int c = std::min(kAdvArgIds, n - i);
    for (int j = 0; j < kAdvArgIds; j++) a.v[j] = j < c ? ids_host[i + j] : -1;
    guide_advance_args_kernel<<<1, kAdvThreads, 0, s>>>(gb, slot, a, c);
  }
}
