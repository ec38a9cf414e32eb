// lora.hip — per-row LoRA adapters (bs_load_adapter, bs_set_row_adapter): y += scale * B_a (A_a x) behind the unchanged
// weight GEMVs / GEMMs, with the adapter a chosen per KV row.  bf16 stages.
//
// The work unit is a token tile: up to 16 consecutive tokens of ONE KV row, which therefore share one adapter.  A pass
// of B rows x S tokens has B * ceil(S / 16) tiles; a decode step has one live token per tile.  A tile reads its row's
// adapter id from the device table of the rows (or takes the launch's fixed id: bs_adapter_delta) and the adapter's
// arrays from the device table of adapters, so a replayed graph follows later bs_set_row_adapter / load / unload
// calls.  A tile whose row names no adapter, or an adapter without this target, leaves both kernels before its first
// load of anything else: nothing of such a row is read or written.
//
// (a) lora_shrink_kernel, grid (tiles, KS), 4 waves: u^T [r_pad][16 tokens] = A_a[:, kslice] . x[tile, kslice]^T on
//     v_mfma_f32_16x16x32_bf16.  Both operands are K-contiguous, so every fragment is one 16-B global load straight
//     into the operand (an adapter row for A, a token's activation row for B): no LDS, no shuffle.  The block's waves
//     stride the 32-wide k-steps of its slice with the next step's loads in flight behind the MFMAs; their
//     accumulators meet in LDS, are folded in wave order and leave as the fp32 partial u[ks][token][64] by plain
//     stores.  KS = ceil(K / kLoraKSlice) is a function of K alone, so the grid is static under capture; a block
//     streams at most 64 KB of A (r_pad = 64), 32 KB at r_pad = 32.
// (b) lora_expand_kernel, grid (tiles, ceil(N / 128)), 4 waves x 2 column tiles of 16: the KS partials of the lane's
//     token are summed in index order, multiplied by scale and split into bf16 hi + lo (as the attention kernels
//     split P): the two B operands of 1 (r_pad = 32) or 2 (r_pad = 64) k-steps.  The A operand is B_a: r_pad * 2 = 64
//     or 128 contiguous bytes per output row, 16 rows of a wave one contiguous 1 or 2 KB.  In the accumulator lane
//     (token r, g) holds columns n0 + 4 g .. + 3 of its token: EPI_RESID is one 16-B fp32 load / add / store;
//     EPI_QKV routes the four columns as the GEMV epilogue does (they stay inside one (head, q | k | v) run because
//     head_dim % 4 == 0) and stores bf16(float(old) + delta) with one 8-B read-modify-write.  Only live tokens store.
// No atomics, no tickets: the kernel boundary publishes u.  Results are bit-identical from run to run and between graph
// replay and eager launches.
#include "attn_merge.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kLoraWaves = 4;
constexpr int kLoraNTW = 2;  // 16-column tiles per wave of the expand

struct LoraArgs {
  const LoraDev* table;
  const int* rows;
  float* u;        // [KS][B * S][kLoraMaxRank]
  const bf16* x;   // [B * S][K]
  int fixed_id;    // >= 0: every row uses it
  int layer, target, B, S, slot, K, N, KS;
};

__global__ void lora_table_kernel(LoraDev* table, int id, LoraDev v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) table[id] = v;
}

__global__ void lora_rows_kernel(int* rows, int slot, int count, int id) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) rows[slot + i] = id;
}

// The tile's adapter for the launch's target, or r_pad = 0 when its row has none (or none for this target).
// Block-uniform.  (The table entry is read field by field: a local copy indexed by the target would live in scratch.)
struct LoraTile {
  const bf16* a;
  const bf16* b;
  int r_pad;
  float scale;
};
__device__ __forceinline__ LoraTile lora_tile_adapter(const LoraArgs& a, int b) {
  const LoraTile none{nullptr, nullptr, 0, 0.f};
  const int id = a.fixed_id >= 0 ? a.fixed_id : a.rows[a.slot + b];
  if (id < 0 || id >= kLoraMax) return none;
  const LoraDev* ad = a.table + id;
  const LoraTile t{ad->a[a.target], ad->b[a.target], ad->r_pad, ad->scale};
  if ((t.r_pad != 32 && t.r_pad != 64) || !t.a || !t.b) return none;
  return t;
}

template <int RT>  // r_pad = 16 RT
__device__ __forceinline__ void lora_shrink_body(const LoraArgs& a, const bf16* A, int b, int tt, float* lds) {
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ks = blockIdx.y, M = a.B * a.S;
  const int k0 = ks * kLoraKSlice, k1 = min(a.K, k0 + kLoraKSlice);
  const int nsteps = (k1 - k0) >> 5;
  // the B operand's column r is token 16 tt + r (a token past the row's end re-reads its last one and is never stored)
  const bf16* xp = a.x + (size_t)(b * a.S + min(tt * 16 + r, a.S - 1)) * a.K + k0 + 8 * g;
  const bf16* ap = A + (size_t)r * a.K + k0 + 8 * g;  // A operand row r of rank tile jt: adapter row 16 jt + r
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[RT];
  bf16x8 af[RT], an[RT], xf = zero, xn = zero;
#pragma unroll
  for (int jt = 0; jt < RT; jt++) {
    acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    af[jt] = zero;
    an[jt] = zero;
  }
  int s = w;
  if (s < nsteps) {
    xf = *reinterpret_cast<const bf16x8*>(xp + 32 * s);
#pragma unroll
    for (int jt = 0; jt < RT; jt++) af[jt] = *reinterpret_cast<const bf16x8*>(ap + (size_t)jt * 16 * a.K + 32 * s);
  }
  for (; s < nsteps; s += kLoraWaves) {
    const int sn = s + kLoraWaves;
    if (sn < nsteps) {  // the next step's loads, in flight behind this step's MFMAs
      xn = *reinterpret_cast<const bf16x8*>(xp + 32 * sn);
#pragma unroll
      for (int jt = 0; jt < RT; jt++) an[jt] = *reinterpret_cast<const bf16x8*>(ap + (size_t)jt * 16 * a.K + 32 * sn);
    }
#pragma unroll
    for (int jt = 0; jt < RT; jt++) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[jt], xf, acc[jt], 0, 0, 0);
    xf = xn;
#pragma unroll
    for (int jt = 0; jt < RT; jt++) af[jt] = an[jt];
  }
  // acc[jt][i] = u[token r][rank 16 jt + 4 g + i]: the waves meet in LDS [wave][token][64]
#pragma unroll
  for (int jt = 0; jt < RT; jt++)
    *reinterpret_cast<f32x4*>(lds + (w * 16 + r) * kLoraMaxRank + 16 * jt + 4 * g) = acc[jt];
  __syncthreads();
  constexpr int G = RT * 4;  // groups of 4 ranks per token
  for (int idx = tid; idx < 16 * G; idx += kLoraWaves * 64) {
    const int tok = idx / G, j4 = (idx - tok * G) * 4;
    const int t = tt * 16 + tok;
    if (t >= a.S) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(lds + tok * kLoraMaxRank + j4);
#pragma unroll
    for (int ww = 1; ww < kLoraWaves; ww++) v += *reinterpret_cast<const f32x4*>(lds + (ww * 16 + tok) * kLoraMaxRank + j4);
    *reinterpret_cast<f32x4*>(a.u + ((size_t)ks * M + b * a.S + t) * kLoraMaxRank + j4) = v;
  }
}

__global__ __launch_bounds__(kLoraWaves * 64) void lora_shrink_kernel(LoraArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kLoraWaves * 16 * kLoraMaxRank];
  const int tps = (a.S + 15) >> 4;
  const int b = blockIdx.x / tps, tt = blockIdx.x - b * tps;
  const LoraTile ad = lora_tile_adapter(a, b);
  if (!ad.r_pad) return;
  const bf16* A = ad.a + (size_t)a.layer * ad.r_pad * a.K;
  if (ad.r_pad == 32) lora_shrink_body<2>(a, A, b, tt, lds);
  else lora_shrink_body<4>(a, A, b, tt, lds);
}

template <int RT>
__device__ __forceinline__ void lora_expand_body(const LoraArgs& a, const Epi& ep, const LoraTile& ad, int b, int tt) {
  constexpr int KST = RT / 2, RP = RT * 16;
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.B * a.S, ntiles = a.N >> 4;
  const int t = tt * 16 + r;
  const bool live = t < a.S;
  const int m = b * a.S + min(t, a.S - 1);
  const bf16* Bm = ad.b + (size_t)a.layer * a.N * RP;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // B_a rows of this wave's column tiles: issued first, in flight behind the sum of the partials
  const int nt0 = (blockIdx.y * kLoraWaves + w) * kLoraNTW;
  bf16x8 bf[kLoraNTW][KST];
#pragma unroll
  for (int i = 0; i < kLoraNTW; i++)
#pragma unroll
    for (int kk = 0; kk < KST; kk++)
      bf[i][kk] = nt0 + i < ntiles
                      ? *reinterpret_cast<const bf16x8*>(Bm + (size_t)((nt0 + i) * 16 + r) * RP + 32 * kk + 8 * g)
                      : zero;
  // u of token r, ranks 32 kk + 8 g .. + 7: the KS partials in index order
  float us[KST][8];
#pragma unroll
  for (int kk = 0; kk < KST; kk++)
#pragma unroll
    for (int e = 0; e < 8; e++) us[kk][e] = 0.f;
  if (live) {
    const float* up = a.u + (size_t)m * kLoraMaxRank + 8 * g;
    for (int ks = 0; ks < a.KS; ks++, up += (size_t)M * kLoraMaxRank)
#pragma unroll
      for (int kk = 0; kk < KST; kk++) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(up + 32 * kk);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(up + 32 * kk + 4);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          us[kk][e] += lo[e];
          us[kk][4 + e] += hi[e];
        }
      }
  }
  bf16x8 uh[KST], ul[KST];
#pragma unroll
  for (int kk = 0; kk < KST; kk++)
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float v = ad.scale * us[kk][e];
      const bf16 hi = (bf16)v;
      uh[kk][e] = hi;
      ul[kk][e] = (bf16)(v - (float)hi);
    }
  const bool vec = (((uintptr_t)ep.out_f32 | ((uintptr_t)ep.ldo * 4)) & 15) == 0;
#pragma unroll
  for (int i = 0; i < kLoraNTW; i++) {
    if (nt0 + i >= ntiles) break;  // wave-uniform
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KST; kk++) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i][kk], uh[kk], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[i][kk], ul[kk], acc, 0, 0, 0);
    }
    if (!live) continue;
    const int n = (nt0 + i) * 16 + 4 * g;  // acc[j] = delta[token r][n + j]
    if (ep.kind == EPI_RESID) {
      float* o = ep.out_f32 + (size_t)m * ep.ldo + n;
      if (vec) {
        f32x4 v = *reinterpret_cast<f32x4*>(o);
        v += acc;
        *reinterpret_cast<f32x4*>(o) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] += acc[j];
      }
    } else {  // EPI_QKV: epi_store's routing of column n
      const int three = 3 * ep.head_dim;
      const int head = n / three, rr = n - head * three, which = rr / ep.head_dim, d = rr - which * ep.head_dim;
      bf16* p;
      if (which == 0) {
        p = (bf16*)ep.q_out + (size_t)m * ep.hidden + head * ep.head_dim + d;
      } else {
        const int past = ep.past_dev ? ep.past_dev[b] : ep.past;
        const size_t idx = (((size_t)(ep.slot + b) * ep.n_head + head) * ep.max_ctx + past + t) * ep.head_dim + d;
        p = (bf16*)(which == 1 ? ep.k_cache : ep.v_cache) + idx;
      }
      bf16x4 v = *reinterpret_cast<bf16x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = (bf16)((float)v[j] + acc[j]);
      *reinterpret_cast<bf16x4*>(p) = v;
    }
  }
}

__global__ __launch_bounds__(kLoraWaves * 64) void lora_expand_kernel(LoraArgs a, Epi ep) {
  const int tps = (a.S + 15) >> 4;
  const int b = blockIdx.x / tps, tt = blockIdx.x - b * tps;
  const LoraTile ad = lora_tile_adapter(a, b);
  if (!ad.r_pad) return;
  if (ad.r_pad == 32) lora_expand_body<2>(a, ep, ad, b, tt);
  else lora_expand_body<4>(a, ep, ad, b, tt);
}

// ctx [M][K] bf16 = the merge of a deferred-merge attention's partials (attn_merge.h), as the dense GEMV's prologue
// forms it: the dense adapter's input on the steps whose base path never writes ctx.
__global__ __launch_bounds__(256) void lora_ctx_parts_kernel(AttnParts p, bf16* ctx, int M, int K) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  const int kq = K >> 2;
  const int gidx = blockIdx.x * 256 + threadIdx.x;
  if (gidx >= M * kq) return;
  const int b = gidx / kq, e = (gidx - b * kq) * 4;
  PartsRegs rr;
  attn_parts_load(p, b, e, [](const float* q, size_t i) { return q[i]; },
                  [](const float* q, size_t i) { return *reinterpret_cast<const float4*>(q + i); }, rr);
  float o[4];
  attn_parts_combine(p.nsplit, rr, o);
  bf16x4 v;
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = (bf16)o[j];
  *reinterpret_cast<bf16x4*>(ctx + (size_t)b * K + e) = v;
}

}  // namespace

int lora_ksplits(int K) { return (K + kLoraKSlice - 1) / kLoraKSlice; }

void launch_lora_table(LoraDev* table, int id, const LoraDev& v, hipStream_t s) {
  lora_table_kernel<<<1, 64, 0, s>>>(table, id, v);
}

void launch_lora_rows(int* rows, int slot, int count, int id, hipStream_t s) {
  lora_rows_kernel<<<(count + 255) / 256, 256, 0, s>>>(rows, slot, count, id);
}

void launch_lora_delta(const LoraBufs& lb, int fixed_id, int layer, int target, const void* x, int B, int S, int slot,
                       int K, int N, const Epi& ep, hipStream_t s) {
  LoraArgs a{lb.table, lb.rows, lb.u, (const bf16*)x, fixed_id, layer, target, B, S, slot, K, N, lora_ksplits(K)};
  const int tiles = B * ((S + 15) / 16);
  const int per_block = 16 * kLoraWaves * kLoraNTW;
  lora_shrink_kernel<<<dim3(tiles, a.KS), kLoraWaves * 64, 0, s>>>(a);
  lora_expand_kernel<<<dim3(tiles, (N + per_block - 1) / per_block), kLoraWaves * 64, 0, s>>>(a, ep);
}

void launch_lora_ctx_parts(const AttnParts& p, void* ctx, int M, int K, hipStream_t s) {
  const int groups = M * (K / 4);
  lora_ctx_parts_kernel<<<(groups + 255) / 256, 256, 0, s>>>(p, (bf16*)ctx, M, K);
}
