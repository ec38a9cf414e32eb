// kv_fork.hip — KV row fork (bs_fork_kv): positions [0, npos) of one cache row copied to
// `count` other rows, every (layer, K|V, head) segment of the stage in one launch.
//
// The cache is [layer][K|V][slot][head][pos][hd] (one allocation), so a row's cached prefix is L * 2 * n_head
// segments of npos * hd * esz contiguous bytes, one every max_ctx * hd * esz bytes inside the row and one row every
// n_head of those.  The kernel walks the flattened list of fixed-size chunks of all segments (16 bytes for codes and
// values, 4 bytes for the int8 cache's fp32 scales, whose segments start on no wider boundary): a grid-stride loop
// over tiles of 256 * kForkU chunks.  Every lane issues its kForkU loads before its first store and stores each
// loaded chunk `count` times, so the source is read once whatever the fan-out.  Plain vector loads and stores (with
// non-temporal hints the fork measured slower at 11 of 12 points, up to 1.4x at count 7: profiles/kv_fork_ab.txt);
// no atomics, nothing a block waits for; no byte at or beyond npos of a segment is touched.
#include "kernels.h"

namespace {

constexpr int kForkThreads = 256;
constexpr int kForkU = 4;  // chunks per lane in flight before the first store

typedef unsigned int fork_u4 __attribute__((ext_vector_type(4)));

struct ForkGeom {
  unsigned long long total;     // chunks of all segments
  unsigned cps;                 // chunks per segment (npos * bytes per position / chunk bytes)
  unsigned n_head;
  unsigned long long seg_stride;  // bytes between the heads of a row: max_ctx * bytes per position
  unsigned long long half;        // bytes of K (or V) of one layer: max_batch * n_head * seg_stride
  unsigned long long src_row;     // src_slot * n_head * seg_stride
  unsigned long long dst_row;     // dst_slot * n_head * seg_stride
  int count;
};

template <typename V>
__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(char* __restrict__ base, ForkGeom g) {
  constexpr unsigned long long tile = (unsigned long long)kForkThreads * kForkU;
  const unsigned long long row_bytes = (unsigned long long)g.n_head * g.seg_stride;
  for (unsigned long long t = (unsigned long long)blockIdx.x * tile; t < g.total; t += (unsigned long long)gridDim.x * tile) {
    // the tile's first chunk, by uniform 64-bit arithmetic; every lane's chunk is then a 32-bit step away
    const unsigned long long s0 = t / g.cps;
    const unsigned seg0 = (unsigned)s0;  // segments: layers * 2 * n_head, far below 2^32
    const unsigned c0 = (unsigned)(t - s0 * g.cps);
    V v[kForkU];
    unsigned long long off[kForkU];  // byte offset of the chunk inside a row's (layer, K|V) image, plus the layer
    bool live[kForkU];
#pragma unroll
    for (int u = 0; u < kForkU; u++) {
      const unsigned i = (unsigned)u * kForkThreads + threadIdx.x;
      live[u] = t + i < g.total;
      const unsigned c = c0 + i;  // cps + tile fits 32 bits (host check)
      const unsigned q = c / g.cps, cc = c - q * g.cps;
      const unsigned seg = seg0 + q;
      const unsigned lw = seg / g.n_head;  // layer * 2 + (K|V)
      const unsigned head = seg - lw * g.n_head;
      off[u] = (unsigned long long)lw * g.half + (unsigned long long)head * g.seg_stride + (unsigned long long)cc * sizeof(V);
      if (live[u]) v[u] = *reinterpret_cast<const V*>(base + g.src_row + off[u]);
    }
    for (int d = 0; d < g.count; d++) {
      char* dst = base + g.dst_row + (unsigned long long)d * row_bytes;
#pragma unroll
      for (int u = 0; u < kForkU; u++)
        if (live[u]) *reinterpret_cast<V*>(dst + off[u]) = v[u];
    }
  }
}

template <typename V>
void fork_launch(char* base, const ForkGeom& g, int cus, hipStream_t s) {
  constexpr unsigned long long tile = (unsigned long long)kForkThreads * kForkU;
  const unsigned long long tiles = (g.total + tile - 1) / tile;
  const unsigned grid = (unsigned)(tiles < (unsigned long long)cus * 8 ? tiles : (unsigned long long)cus * 8);
  kv_fork_kernel<V><<<grid, kForkThreads, 0, s>>>(base, g);
}

}  // namespace

bool kv_fork_supported(int npos, size_t pos_bytes) {
  // chunks per segment (at most one per 4 bytes) plus one tile must fit 32 bits: the kernel's per-lane arithmetic
  return (unsigned long long)npos * pos_bytes / 4 + (unsigned long long)kForkThreads * kForkU < (1ull << 32);
}

void launch_kv_fork(void* base, int chunk_bytes, int n_lw, int n_head, int max_batch, int max_ctx, size_t pos_bytes,
                    int src_slot, int dst_slot, int count, int npos, int cus, hipStream_t s) {
  ForkGeom g;
  g.cps = (unsigned)((unsigned long long)npos * pos_bytes / chunk_bytes);
  g.total = (unsigned long long)n_lw * n_head * g.cps;
  g.n_head = (unsigned)n_head;
  g.seg_stride = (unsigned long long)max_ctx * pos_bytes;
  g.half = (unsigned long long)max_batch * n_head * g.seg_stride;
  g.src_row = (unsigned long long)src_slot * n_head * g.seg_stride;
  g.dst_row = (unsigned long long)dst_slot * n_head * g.seg_stride;
  g.count = count;
  if (!g.total) return;
  if (cus <= 0) cus = 256;
  if (chunk_bytes == 16) fork_launch<fork_u4>((char*)base, g, cus, s);
  else fork_launch<unsigned int>((char*)base, g, cus, s);
}
