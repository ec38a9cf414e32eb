// row_sample.hip — per-row nucleus sampling (include/bloomstage.h "Per-row sampling").
//
// An exact top-k / top-p selection over the V fp32 logits of each row, then a seeded draw, all in integer arithmetic
// on 2^40 fixed-point weights q_v = rint(exp((l_v - max l) / temperature) * 2^40): histogram and scan sums are
// integer adds, so they do not depend on the order the blocks or the atomics arrive in, and every threshold
// comparison is exact.  No floating-point atomics, no cross-block hand-off inside a launch: the blocks of one row
// meet only at kernel boundaries.
//
// The selection is a radix select on key(l) = f32_order_key(l + 0.0f) (monotone in l; -0 and +0 share a key) in
// three digits of 11, 11 and 10 bits.  Seven launches on the step's stream, grids static in (B, V):
//   stage 0      every row: max key (first index on ties) -> rowmax; count histogram of digit 0 (top_k rows)
//   stage 1, 2   resolve the previous count digit, histogram the next one under the chosen prefix
//   stage 3      resolve the last count digit -> tk = key of the top_k-th largest logit (0: no top_k);
//                (count, mass) histogram of digit 0 over the candidates key >= tk
//   stage 4      totals of that histogram = |C|, mass(C); thr = ceil(top_p * mass(C)) (exact, 128-bit product);
//                resolve digit 0 by mass, histogram digit 1
//   stage 5      resolve digit 1, histogram digit 2
//   pick         one block per row: resolve digit 2 -> t, |N|, mass(N); u24 from the counter generator; one masked
//                scan in vocabulary index order for the first v whose running mass exceeds (u24 * mass(N)) >> 24;
//                writes the token and the read-out, zeroes the row's histograms for the next step and advances the
//                row's cached length (the step's last kernel).
// "Resolve" walks a 2048-bin histogram from the top bin down until the running sum reaches the target; every block of
// the row does it for itself (a few KB out of L2) and block 0 records the result for the next launch.  A row without
// sampler state runs stage 0 and the pick only and gets the first index of its largest logit.
//
// A selection has three indices: the table row whose state it uses, the logits row it reads and the scratch lane it
// works in.  The plain tail and bs_sample_logits make one selection per KV row (lane = table row = slot + b).  The
// tail of a verify-draw pass makes B * S of them, S per KV row, in a scratch of its own: selection m uses table row
// slot + m / S and lane m, and draws at position past_dev[m / S] + m % S + 1.  Stage 0 fixes that position in the
// lane (pos), because the pick of the row's last position advances past_dev while the picks of its other positions
// run.  The per-row scratch is never touched by a verify-draw pass, so a plain step between two passes finds its
// histograms zero.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

// What the launches of one row hand on (written by block 0 of a stage, read by every block of the next one).
struct RsState {
  unsigned long long mass_above;   // mass of the candidates strictly above the prefix range
  unsigned long long thr;          // ceil(top_p * mass(C))
  unsigned long long massC;
  uint32_t prefix;  // digits chosen so far (mass phase after stage 3, count phase before)
  uint32_t cnt_above;
  uint32_t tk;      // key of the top_k-th largest logit (0: every key is a candidate)
  uint32_t nC;
};

namespace {

typedef unsigned long long u64;

constexpr int kBins = 2048;
constexpr int kThreads = 1024;

__device__ __forceinline__ uint64_t rs_sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t rs_lb32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// The repo's counter generator (kernels.hip d_sm64 / d_bits) keyed by (seed, position): tag "ROWS", no KV row.
__device__ __forceinline__ uint32_t row_draw_bits(uint64_t seed, uint32_t pos) {
  const uint64_t key = rs_sm64(seed ^ rs_sm64(0x524F575300000000ull));
  return rs_lb32((uint32_t)key ^ rs_lb32(pos + (uint32_t)(key >> 32)));
}

__device__ __forceinline__ uint32_t rs_key(float l) { return f32_order_key(l + 0.0f); }
__device__ __forceinline__ float rs_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// q_v: IEEE subtraction and division, expf within one ulp, an exact power-of-two scaling, round to nearest integer
__device__ __forceinline__ u64 rs_weight(float l, float lmax, float temperature) {
  const float w = expf(__fdiv_rn(__fsub_rn(l, lmax), temperature));
  return (u64)__float2ull_rn(w * 0x1p40f);
}

// ceil(top_p * mass) for top_p in (0, 1]: top_p = mant * 2^-sh exactly, the product in 128 bits
__device__ __forceinline__ u64 rs_ceil_frac(float top_p, u64 mass) {
  const uint32_t bits = __float_as_uint(top_p), ex = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu;
  const u64 mant = ex ? (frac | 0x800000u) : frac;
  const int sh = ex ? 150 - (int)ex : 149;  // >= 23 for top_p <= 1
  const u64 lo = mant * mass, hi = __umul64hi(mant, mass);
  if ((lo | hi) == 0) return 0;
  if (sh >= 128) return 1;
  u64 q, rem;
  if (sh >= 64) {
    q = sh == 64 ? hi : hi >> (sh - 64);
    rem = (sh == 64 ? 0ull : (hi & ((1ull << (sh - 64)) - 1))) | lo;
  } else {  // 23 <= sh < 64; hi < 2^18 because mant < 2^24 and mass < 2^58
    q = (hi << (64 - sh)) | (lo >> sh);
    rem = lo & ((1ull << sh) - 1);
  }
  return q + (rem ? 1 : 0);
}

struct RsResolved {
  int bin;
  u64 val_above, val_bin;
  uint32_t cnt_above, cnt_bin;
};

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}

// Wave 0 only, all 64 lanes: the highest bin d with base + sum_{j >= d} val[j] >= target (val, cnt: LDS [kBins]), the
// sums above it and its own entries.  Lane L owns bins [32 L, 32 L + 32).  Every lane returns the result.
__device__ RsResolved rs_resolve(const u64* val, const uint32_t* cnt, u64 base, u64 target) {
  const int lane = threadIdx.x & 63;
  u64 mine = 0;
  uint32_t minec = 0;
  for (int j = 0; j < 32; j++) { mine += val[lane * 32 + j]; minec += cnt[lane * 32 + j]; }
  // sums over the lanes above this one
  u64 above = 0;
  uint32_t abovec = 0;
  for (int o = 63; o > 0; o--) {  // 63 shuffles of two words: once per block and launch
    const u64 v = shfl_u64(mine, o);
    const uint32_t c = (uint32_t)__shfl((int)minec, o, 64);
    if (o > lane) { above += v; abovec += c; }
  }
  const bool crosses = base + above < target && base + above + mine >= target;  // one lane at most
  const u64 mask = __ballot(crosses);
  RsResolved r{0, 0, 0, 0, 0};
  if (!mask) return r;  // never for 1 <= target <= base + total, which every caller guarantees
  const int owner = (int)__builtin_ctzll(mask);
  if (lane == owner) {
    u64 acc = above;
    uint32_t accc = abovec;
    int d = 0;
    for (int j = 31; j >= 0; j--) {
      const u64 v = val[lane * 32 + j];
      if (base + acc + v >= target) { d = j; break; }
      acc += v; accc += cnt[lane * 32 + j];
    }
    r.bin = lane * 32 + d;
    r.val_above = acc; r.cnt_above = accc;
    r.val_bin = val[r.bin]; r.cnt_bin = cnt[r.bin];
  }
  r.bin = __shfl(r.bin, owner, 64);
  r.val_above = shfl_u64(r.val_above, owner);
  r.val_bin = shfl_u64(r.val_bin, owner);
  r.cnt_above = (uint32_t)__shfl((int)r.cnt_above, owner, 64);
  r.cnt_bin = (uint32_t)__shfl((int)r.cnt_bin, owner, 64);
  return r;
}

// digit `lvl` of a key and the prefix above it
__device__ __forceinline__ uint32_t rs_digit(uint32_t key, int lvl) {
  return lvl == 0 ? key >> 21 : (lvl == 1 ? (key >> 10) & 2047u : key & 1023u);
}
__device__ __forceinline__ uint32_t rs_prefix_of(uint32_t key, int lvl) { return lvl == 0 ? 0u : (lvl == 1 ? key >> 21 : key >> 10); }

__device__ __forceinline__ bool rs_topk_on(const RowSamplerDev& p, int V) { return p.active && p.top_k > 0 && p.top_k < V; }

// Resolve histogram `j` (0..5) of the lane from the state before it; wave 0 computes, everyone gets it through LDS.
// sval / scnt: LDS [kBins] scratch.  Call with the whole block.
__device__ void rs_advance(const RowSampleBufs& rb, int lane, int j, const RowSamplerDev& p, const RsState& ps, u64* sval,
                           uint32_t* scnt, RsState* out) {
  const int tid = threadIdx.x;
  const uint32_t* hc = rb.hcnt + ((size_t)lane * 6 + j) * kBins;
  const u64* hm = j >= 3 ? rb.hmass + ((size_t)lane * 3 + (j - 3)) * kBins : nullptr;
  for (int i = tid; i < kBins; i += kThreads) {
    const uint32_t c = hc[i];
    scnt[i] = c;
    sval[i] = hm ? hm[i] : (u64)c;
  }
  __syncthreads();
  if (tid < 64) {
    RsState ns = ps;
    const int lvl = j % 3;
    if (j == 3) {  // totals over the candidates: |C|, mass(C), the nucleus target
      u64 m = 0;
      uint32_t c = 0;
      for (int i = tid; i < kBins; i += 64) { m += sval[i]; c += scnt[i]; }
      for (int o = 32; o >= 1; o >>= 1) {
        m += shfl_u64(m, tid ^ o);
        c += (uint32_t)__shfl((int)c, tid ^ o, 64);
      }
      ns.massC = m; ns.nC = c; ns.thr = rs_ceil_frac(p.top_p, m);
    }
    const u64 base = j >= 3 ? ns.mass_above : (u64)ns.cnt_above;
    const u64 target = j >= 3 ? ns.thr : (u64)p.top_k;
    const RsResolved r = rs_resolve(sval, scnt, base, target);
    ns.prefix = lvl == 0 ? (uint32_t)r.bin : ((ns.prefix << (lvl == 1 ? 11 : 10)) | (uint32_t)r.bin);
    ns.cnt_above += r.cnt_above;
    if (j >= 3) ns.mass_above += r.val_above;
    if (j == 2) {  // the count phase ends: tk is a whole key; the mass phase starts from nothing
      ns.tk = ns.prefix; ns.prefix = 0; ns.cnt_above = 0; ns.mass_above = 0;
    }
    if (j == 5) {  // the mass phase ends: the entries of the last bin belong to the nucleus
      ns.cnt_above += r.cnt_bin; ns.mass_above += r.val_bin;
    }
    if (tid == 0) *out = ns;
  }
  __syncthreads();
}

// Where selection m (the block's y or x index) finds its state, its scratch and its logits: table row slot + m / per,
// lane lane0 + m, logits row m.  per == 1 and lane0 == slot: one selection per KV row in the row's own lane.
struct RsMap { int slot, lane0, per; };

__global__ __launch_bounds__(kThreads) void row_level_kernel(RowSampleBufs rb, const float* __restrict__ logits, int ld,
                                                             int V, RsMap mp, int stage, const int* past_dev) {
  __shared__ u64 sval[kBins];
  __shared__ uint32_t scnt[kBins];
  __shared__ RsState cur;
  __shared__ u64 red[16];
  const int m = blockIdx.y, row = mp.slot + m / mp.per, lane = mp.lane0 + m, tid = threadIdx.x;
  const RowSamplerDev p = rb.table[row];
  const float* lr = logits + (size_t)m * ld;
  const bool topk = rs_topk_on(p, V);
  // a verify-draw pass: the draw position of this selection, read by the pick (which advances past_dev)
  if (stage == 0 && rb.pos && blockIdx.x == 0 && tid == 0) rb.pos[lane] = past_dev[m / mp.per] + m % mp.per + 1;
  if (stage > 0 && !p.active) return;
  if (stage > 0 && stage < 3 && !topk) return;

  if (stage == 0) {
    for (int i = tid; i < kBins; i += kThreads) scnt[i] = 0;
    __syncthreads();
    u64 best = 0;
    for (int i = blockIdx.x * kThreads + tid; i < V; i += gridDim.x * kThreads) {
      const uint32_t key = rs_key(lr[i]);
      const u64 k = ((u64)key << 32) | (0xFFFFFFFFu - (uint32_t)i);
      best = k > best ? k : best;
      if (topk) atomicAdd(&scnt[key >> 21], 1u);
    }
    for (int o = 32; o >= 1; o >>= 1) {
      const u64 other = shfl_u64(best, (tid & 63) ^ o);
      best = other > best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kThreads / 64; w++) best = red[w] > best ? red[w] : best;
      atomicMax(rb.rowmax + lane, best);
    }
    if (topk) {
      uint32_t* hc = rb.hcnt + ((size_t)lane * 6 + 0) * kBins;
      for (int i = tid; i < kBins; i += kThreads)
        if (scnt[i]) atomicAdd(hc + i, scnt[i]);
    }
    return;
  }

  // state before histogram stage - 1, then resolve that histogram
  RsState ps{};
  if (stage == 3 && !topk) {
    if (tid == 0) cur = ps;  // every key is a candidate
    __syncthreads();
  } else {
    if (stage != 1) ps = rb.st[(size_t)lane * 6 + stage - 1];
    rs_advance(rb, lane, stage - 1, p, ps, sval, scnt, &cur);
  }
  const RsState st = cur;
  if (blockIdx.x == 0 && tid == 0) rb.st[(size_t)lane * 6 + stage] = st;
  __syncthreads();  // sval / scnt are reused below

  // histogram of this stage's digit under the chosen prefix
  const int lvl = stage % 3;
  const bool mass = stage >= 3;
  for (int i = tid; i < kBins; i += kThreads) { scnt[i] = 0; sval[i] = 0; }
  __syncthreads();
  const float lmax = rs_unkey((uint32_t)(rb.rowmax[lane] >> 32));
  for (int i = blockIdx.x * kThreads + tid; i < V; i += gridDim.x * kThreads) {
    const float l = lr[i];
    const uint32_t key = rs_key(l);
    if (rs_prefix_of(key, lvl) != st.prefix) continue;
    if (mass && key < st.tk) continue;
    const uint32_t d = rs_digit(key, lvl);
    atomicAdd(&scnt[d], 1u);
    if (mass) atomicAdd(&sval[d], rs_weight(l, lmax, p.temperature));
  }
  __syncthreads();
  uint32_t* hc = rb.hcnt + ((size_t)lane * 6 + stage) * kBins;
  u64* hm = mass ? rb.hmass + ((size_t)lane * 3 + (stage - 3)) * kBins : nullptr;
  for (int i = tid; i < kBins; i += kThreads)
    if (scnt[i]) {
      atomicAdd(hc + i, scnt[i]);
      if (mass && sval[i]) atomicAdd(hm + i, sval[i]);
    }
}

struct RsPositions { int v[64]; };

// One block per selection: the step's last kernel.  positions: by value when use_pos (bs_sample_logits), the lane's
// rb.pos where the scratch has one (a verify-draw pass), else past_dev[b] + seq; past_adv (optional): the block of
// the last selection of every KV row does past_adv[m / per] += seq.
__global__ __launch_bounds__(kThreads) void row_pick_kernel(RowSampleBufs rb, const float* __restrict__ logits, int ld,
                                                            int V, RsMap mp, RsPositions pos, int use_pos,
                                                            const int* past_dev, int seq, int* __restrict__ tokens,
                                                            int* past_adv) {
  __shared__ u64 sval[kBins];
  __shared__ uint32_t scnt[kBins];
  __shared__ RsState cur;
  __shared__ u64 wtot[kThreads / 64];
  __shared__ int found;
  const int b = blockIdx.x, row = mp.slot + b / mp.per, sl = mp.lane0 + b, tid = threadIdx.x, lane = tid & 63,
            wave = tid >> 6;
  const RowSamplerDev p = rb.table[row];
  const float* lr = logits + (size_t)b * ld;
  const u64 rmax = rb.rowmax[sl];
  const int position = use_pos ? pos.v[b] : (rb.pos ? rb.pos[sl] : past_dev[b] + seq);
  const int greedy = (int)(0xFFFFFFFFu - (uint32_t)(rmax & 0xFFFFFFFFull));
  const float lmax = rs_unkey((uint32_t)(rmax >> 32));
  RowDrawDev out{};
  out.position = position;
  int token = greedy;
  if (!p.active) {
    out.threshold = lmax; out.token = greedy;
  } else {
    const RsState ps = rb.st[(size_t)sl * 6 + 5];
    rs_advance(rb, sl, 5, p, ps, sval, scnt, &cur);
    const RsState st = cur;
    const uint32_t tkey = st.prefix;
    const u64 massN = st.mass_above;
    const uint32_t u24 = row_draw_bits(p.seed, (uint32_t)position) >> 8;
    // (u24 * mass(N)) >> 24 in 128 bits: u24 < 2^24, mass(N) < 2^58
    const u64 target = (__umul64hi((u64)u24, massN) << 40) | (((u64)u24 * massN) >> 24);
    if (tid == 0) found = -1;
    __syncthreads();
    u64 run = 0;  // mass of the nucleus members before this tile (block-uniform)
    for (int t0 = 0; t0 < V; t0 += kThreads * 4) {
      u64 q[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = t0 + tid * 4 + j;
        q[j] = 0;
        if (i < V) {
          const float l = lr[i];
          if (rs_key(l) >= tkey) q[j] = rs_weight(l, lmax, p.temperature);
        }
        s += q[j];
      }
      // inclusive scan of s over the block, index order = thread order
      u64 inc = s;
      for (int o = 1; o < 64; o <<= 1) {
        const u64 v = shfl_u64(inc, lane - o < 0 ? lane : lane - o);
        if (lane >= o) inc += v;
      }
      if (lane == 63) wtot[wave] = inc;
      __syncthreads();
      u64 before = run, total = run;
      for (int w = 0; w < kThreads / 64; w++) {
        if (w < wave) before += wtot[w];
        total += wtot[w];
      }
      before += inc - s;
      // the first v whose running mass exceeds target: before <= target < before + s for exactly one thread
      if (before <= target && target < before + s) {
        u64 r = before;
        int sel = -1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          r += q[j];
          if (sel < 0 && r > target) sel = t0 + tid * 4 + j;
        }
        found = sel;
      }
      __syncthreads();
      run = total;
      if (found >= 0) break;
    }
    token = found >= 0 ? found : greedy;  // target < mass(N): always found
    out.threshold = rs_unkey(tkey); out.n_nucleus = (int)st.cnt_above; out.n_candidates = (int)st.nC;
    out.u24 = u24; out.mass_nucleus = massN; out.mass_candidates = st.massC; out.token = token;
    // the lane's histograms back to zero for the next step (stream-ordered behind every reader)
    uint32_t* hc = rb.hcnt + (size_t)sl * 6 * kBins;
    u64* hm = rb.hmass + (size_t)sl * 3 * kBins;
    for (int i = tid; i < 6 * kBins; i += kThreads) hc[i] = 0;
    for (int i = tid; i < 3 * kBins; i += kThreads) hm[i] = 0;
  }
  if (tid == 0) {
    tokens[b] = token;
    rb.draw[sl] = out;
    rb.rowmax[sl] = 0;
    if (past_adv && b % mp.per == mp.per - 1) past_adv[b / mp.per] += seq;  // once per KV row
  }
}

struct RsTableRows { RowSamplerDev v[16]; };
__global__ void row_table_kernel(RowSamplerDev* table, RsTableRows r, int n) {
  if ((int)threadIdx.x < n) table[threadIdx.x] = r.v[threadIdx.x];
}

}  // namespace

size_t row_sample_bytes(int max_batch, size_t* offsets) {
  const size_t sizes[5] = {(size_t)max_batch * sizeof(RowSamplerDev), (size_t)max_batch * 8,
                           (size_t)max_batch * 6 * kBins * 4, (size_t)max_batch * 3 * kBins * 8,
                           (size_t)max_batch * sizeof(RowDrawDev)};
  size_t off = 0;
  for (int i = 0; i < 5; i++) { offsets[i] = off; off = (off + sizes[i] + 255) / 256 * 256; }
  offsets[5] = off;  // the launch-to-launch states [max_batch][6]
  off = (off + (size_t)max_batch * 6 * sizeof(RsState) + 255) / 256 * 256;
  return off;
}

RowSampleBufs row_sample_bufs(char* base, const size_t* offsets) {
  RowSampleBufs rb;
  rb.table = (RowSamplerDev*)(base + offsets[0]);
  rb.rowmax = (unsigned long long*)(base + offsets[1]);
  rb.hcnt = (uint32_t*)(base + offsets[2]);
  rb.hmass = (unsigned long long*)(base + offsets[3]);
  rb.draw = (RowDrawDev*)(base + offsets[4]);
  rb.st = (RsState*)(base + offsets[5]);
  rb.pos = nullptr;
  return rb;
}

size_t row_sample_verify_bytes(size_t* offsets) {
  offsets[6] = row_sample_bytes(kVerifyMaxTokens, offsets);  // its table part stays unused
  return offsets[6] + (size_t)kVerifyMaxTokens * 4;
}

RowSampleBufs row_sample_verify_bufs(const RowSampleBufs& rows, char* base, const size_t* offsets) {
  RowSampleBufs vb = row_sample_bufs(base, offsets);
  vb.table = rows.table;
  vb.pos = (int*)(base + offsets[6]);
  return vb;
}

void launch_row_table(const RowSampleBufs& rb, int slot, const RowSamplerDev* rows, int n, hipStream_t s) {
  for (int i = 0; i < n; i += 16) {
    RsTableRows r{};
    const int c = std::min(16, n - i);
    for (int j = 0; j < c; j++) r.v[j] = rows[i + j];
    row_table_kernel<<<1, 64, 0, s>>>(rb.table + slot + i, r, c);
  }
}

void launch_row_sample(const RowSampleBufs& rb, const float* logits, int ld, int V, int slot, int B,
                       const int* positions, const int* past_dev, int seq, int* tokens, int* past_adv, hipStream_t s) {
  if (B <= 0) return;
  const int nb = std::min(64, std::max(1, (V + 2 * kThreads - 1) / (2 * kThreads)));
  for (int stage = 0; stage < 6; stage++)
    row_level_kernel<<<dim3(nb, B), kThreads, 0, s>>>(rb, logits, ld, V, RsMap{slot, slot, 1}, stage, nullptr);
  for (int i = 0; i < B; i += 64) {  // positions travel by value, 64 rows a launch
    RsPositions pos{};
    const int c = std::min(64, B - i);
    if (positions)
      for (int j = 0; j < c; j++) pos.v[j] = positions[i + j];
    row_pick_kernel<<<c, kThreads, 0, s>>>(rb, logits + (size_t)i * ld, ld, V, RsMap{slot + i, slot + i, 1}, pos,
                                           positions ? 1 : 0,
                                           past_dev ? past_dev + i : nullptr, seq, tokens + i,
                                           past_adv ? past_adv + i : nullptr);
  }
}

void launch_row_sample_verify(const RowSampleBufs& vb, const float* logits, int ld, int V, int slot, int B, int S,
                              const int* past_dev, int* tokens, int* past_adv, hipStream_t s) {
  const int M = B * S;
  if (M <= 0 || M > kVerifyMaxTokens || !vb.pos) return;  // the scratch holds kVerifyMaxTokens lanes
  const int nb = std::min(64, std::max(1, (V + 2 * kThreads - 1) / (2 * kThreads)));
  const RsMap mp{slot, 0, S};
  for (int stage = 0; stage < 6; stage++)
    row_level_kernel<<<dim3(nb, M), kThreads, 0, s>>>(vb, logits, ld, V, mp, stage, past_dev);
  row_pick_kernel<<<M, kThreads, 0, s>>>(vb, logits, ld, V, mp, RsPositions{}, 0, past_dev, S, tokens, past_adv);
}
