// attn_tree.hip — attention of a tree verify pass (bs_forward_tree) and the in-row KV compaction
// behind it (bs_compact_kv).  bf16 stages, head_dim % 8 == 0 and <= 128.  Compiled like attn_prefix.hip with
// -mllvm -amdgpu-mfma-vgpr-form=1 and without packed fp32 (build.py).
//
// A pass feeds N <= 16 tree nodes per row: node i sits at cache position past_b + i (the QKV epilogue of an S = N pass
// wrote it) and attends every cached position < past_b plus the pass's nodes j that are i or an ancestor of i.  A
// cached key's ALiBi position is its index; node j's is past_b + depth(j).  The host turns `parents` into one TreeRow
// per row of the call: anc[i] = the ancestor-or-self mask of node i, depth = 16 nibbles.
//
// attn_tree_kernel, grid (n_head, B, nsplit), 4 waves; nsplit is the verify pass's static rule, the row's length comes
// from past_dev and the tree from the device table, so a captured launch follows a later tree of the same (B, N).
// Wave w of split sp walks the 64-position chunks w + 4 (sp + nsplit j) of [0, past_b + N) in attn_prefix_kernel's
// matrix-core form:
//  * the row's N queries, zero-padded to 16 (and head_dim to HDE = 64 / 96 / 128), are the B operand of
//    v_mfma_f32_16x16x32_bf16 for the whole loop; a K fragment is 16 contiguous bytes of a cache row, loaded from
//    global memory straight into the A operand: S^T = K.Q^T;
//  * mask and bias per element in fp32 after the MFMA; chunks wholly below past_b skip the tree test (wave-uniform);
//    one fp32 online softmax per query (the four g lanes of a query meet by v_permlane swaps); a chunk that holds
//    nothing live for a query leaves its state alone;
//  * O^T = V^T . P^T with P = bf16(p) + bf16(p - bf16(p)); V by LDS-DMA into the wave's own two-stage ring in the
//    swizzled [64][128 x 16-bit] image and out of it with ds_read_b64_tr_b16;
//  * the next chunk's K loads and V DMA are issued behind the chunk's score MFMAs; the ring is the wave's own: no
//    block barrier in the loop;
//  * both buffer descriptors end at position past_b + N: a load beyond it returns zeros, so whatever a rolled-back row
//    still holds there cannot reach a result (a zero V row times p = 0, never junk times 0).
// The waves' (m, l, o) meet in LDS and are folded in wave order.  nsplit == 1: the block writes ctx.  Otherwise the
// verify kernel's ticket path into the verify partials: write-through stores, every storing wave drains them, one lane
// takes the (row, head) ticket, and the block that draws the last one folds splits 0 .. nsplit - 1 in index order.
// No floating-point atomics: bit-identical from run to run.
//
// kv_compact_kernel, grid (n_head, layers * 2): position past + k of a (layer, K|V, head) segment receives what
// position past + src[k] held, k < n <= 16.  The indices travel as kernel arguments.  One block owns one segment, reads
// all n rows into registers, meets at a block barrier, then writes: a source row may be another row's destination.
#include <algorithm>
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kTreeWaves = 4;

__device__ __forceinline__ int tree_tr_off(int row, int ch) {  // attn_prefill.hip attn_tr_off: the [64][128] bf16 image
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
__device__ __forceinline__ float tree_xmax(float v) {  // over the lanes l, l ^ 16, l ^ 32, l ^ 48
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float tree_xsum(float v) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tree_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)0xFFFFFFFF, 0x00020000);
}
__device__ __forceinline__ void tree_store_sc1(float v, float* base, uint32_t elem) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), tree_rsrc(base), elem * 4, 0, 16);
}
__device__ __forceinline__ float tree_load_sc1(const float* base, uint32_t elem) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(tree_rsrc(base), elem * 4, 0, 16));
}

// a.S = N nodes per row; a.part_acc / a.part_ml: the verify partials [B * N][n_head][a.max_chunks][hd] and [..][2].
template <int HDE>
__global__ __launch_bounds__(kTreeWaves * 64) void attn_tree_kernel(AttnArgs a, const TreeRow* table) {
  constexpr int KT = 64, TILEB = KT * 256, NSTG = 2;
  constexpr int KSE = HDE / 32, NTE = HDE / 16;
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  typedef __attribute__((address_space(3))) void lds_void;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kTreeWaves * NSTG * TILEB];
  __shared__ int last;
  const int head = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.S;
  const int hd = a.head_dim, nch = hd >> 3;
  const int past = min(a.past_dev[b], a.max_ctx - N);  // the host checked past + N <= max_ctx
  const int nk = past + N;                              // nothing at or beyond it is read
  const size_t rowbase = ((size_t)(a.slot + b) * a.n_head + head) * a.max_ctx;
  const int cbytes = nk * hd * 2;
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>((const bf16*)a.k_cache + rowbase * hd), (short)0, cbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>((const bf16*)a.v_cache + rowbase * hd), (short)0, cbytes, 0x00020000);
  unsigned char* ring = smem + w * NSTG * TILEB;  // this wave's V stages
  // V DMA: piece pc (1 KB = 4 rows) of a tile; lane l writes LDS chunk l & 15 of row 4 pc + (l >> 4) and fetches that
  // row's logical chunk (l & 15) ^ swz(row).  The lane offsets repeat every 4 pieces (16 rows).
  uint32_t voff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = 4 * i + (lane >> 4);
    const int x = (lane & 15) ^ (((lane >> 4) << 2) | i);
    voff[i] = (uint32_t)(row * hd * 2 + min(x, nch - 1) * 16);
  }
  auto issue_v = [&](int st, int k0) {
#pragma unroll
    for (int pc = 0; pc < 16; pc++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_void*)(ring + st * TILEB + pc * 1024), 16, voff[pc & 3],
                                               (k0 + (pc >> 2) * 16) * hd * 2, 0, 0);
  };
  // A row r of subtile t is key 16 t + arow (the permutation that makes the transposed V reads conflict-free)
  const int pg4 = ((g & 1) << 1) | (g >> 1);
  const int arow = ((((r >> 2) & 1) << 1) | (r >> 3)) * 4 + (r & 3);
  bf16x8 kf[4][KSE];
  auto load_k = [&](int k0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int ks = 0; ks < KSE; ks++) {
        const int d = ks * 32 + 8 * g;
        kf[t][ks] = d < hd ? __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                 rk, (uint32_t)((k0 + t * 16 + arow) * hd * 2 + d * 2), 0, 0))
                           : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      }
  };
  // Q of node r (zero past N and past head_dim); its ancestor-or-self mask; the nodes' depths
  bf16x8 qf[KSE];
  {
    const bf16* qp = (const bf16*)a.q + (size_t)(b * N + min(r, N - 1)) * a.hidden + head * hd;
#pragma unroll
    for (int ks = 0; ks < KSE; ks++) {
      const int d = ks * 32 + 8 * g;
      qf[ks] = (d < hd && r < N) ? *reinterpret_cast<const bf16x8*>(qp + d) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const unsigned anc = r < N ? table[b].anc[r] : 0u;
  const unsigned long long depth = table[b].depth;
  const float slope = a.slopes[head];
  const int nlive = (nk + KT - 1) / KT;
  const int cstep = nsplit * kTreeWaves;
  int c = w + kTreeWaves * sp;
  if (c < nlive) {
    load_k(c * KT);
    issue_v(0, c * KT);
  }
  float m_q = -INFINITY, l_q = 0.f;
  f32x4 o[NTE];  // o[t][i]: unnormalised context of node r, dim 16 t + 4 g + i
#pragma unroll
  for (int t = 0; t < NTE; t++) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int qq = r >> 2, pp = r & 3;
  for (int it = 0; c < nlive; c += cstep, it++) {
    const int st = it & 1, k0 = c * KT;
    // the chunk's K registers and V stage have landed; the other stage's reads (chunk it - 1) have retired
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    f32x4 sacc[4];  // sacc[t][i]: key k0 + 16 t + 4 perm(g) + i against node r
#pragma unroll
    for (int t = 0; t < 4; t++) {
      sacc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSE; ks++)
        sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[ks], sacc[t], 0, 0, 0);
    }
    float sv[4][4];
    if (k0 + KT <= past) {  // wave-uniform: the cached past alone
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++)
          sv[t][i] = fmaf(a.inv_norm, sacc[t][i], slope * (float)(k0 + t * 16 + 4 * pg4 + i));
    } else {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int kpos = k0 + t * 16 + 4 * pg4 + i;
          const int j = kpos - past;  // >= 0: this pass's node j
          const int jc = min(max(j, 0), 15);
          const bool live = j < 0 || (j < N && ((anc >> jc) & 1u));
          const int apos = j < 0 ? kpos : past + (int)((depth >> (4 * jc)) & 15ull);
          sv[t][i] = live ? fmaf(a.inv_norm, sacc[t][i], slope * (float)apos) : -INFINITY;
        }
    }
    // the next chunk: K into the registers the MFMAs above have consumed, V into the other stage
    asm volatile("" ::: "memory");
    if (c + cstep < nlive) {
      load_k((c + cstep) * KT);
      issue_v(st ^ 1, (c + cstep) * KT);
    }
    bf16x8 ph[2], pl[2];
    {
      float rmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) rmax = fmaxf(rmax, sv[t][i]);
      rmax = tree_xmax(rmax);
      const float m_new = fmaxf(m_q, rmax);
      const float scale_q = m_new == -INFINITY ? 1.f : __expf(m_q - m_new);
      float rs = 0.f;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float p = m_new == -INFINITY ? 0.f : __expf(sv[t][i] - m_new);
          sv[t][i] = p;
          rs += p;
        }
      rs = tree_xsum(rs);
      l_q = l_q * scale_q + rs;
      m_q = m_new;
#pragma unroll
      for (int t = 0; t < NTE; t++) o[t] *= scale_q;
      // P^T (B operand of step kb): element e = key 32 kb + 16 (e >> 2) + 4 perm(g) + (e & 3) of node r; hi + lo
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float p = sv[2 * kb + (e >> 2)][e & 3];
          const bf16 hi = (bf16)p;
          ph[kb][e] = hi;
          pl[kb][e] = (bf16)(p - (float)hi);
        }
    }
    // V^T fragments by transposed reads: lane 4q + p of group g addresses row 32 kb + 16 h + 4 perm(g) + q, columns
    // 16 t + 4 p .. + 3, and lane r receives column 16 t + r of those 4 rows
    const unsigned char* vs_ = ring + st * TILEB;
#pragma unroll
    for (int t = 0; t < NTE; t++)
#pragma unroll
      for (int kb = 0; kb < 2; kb++) {
        const int rw0 = 32 * kb + 4 * pg4 + qq;
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s16x4*)(vs_ + tree_tr_off(rw0, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s16x4*)(vs_ + tree_tr_off(rw0 + 16, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const bf16x8 vf = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, ph[kb], o[t], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl[kb], o[t], 0, 0, 0);
      }
  }
  // ---- the waves' (m, l, o) meet in LDS (each wave's own ring: o in stage 0, m / l in stage 1)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  {
    float* wo = reinterpret_cast<float*>(ring);
    float* wml = reinterpret_cast<float*>(ring + TILEB);
#pragma unroll
    for (int t = 0; t < NTE; t++) *reinterpret_cast<f32x4*>(wo + r * HDE + 16 * t + 4 * g) = o[t];
    if (g == 0) {
      wml[r * 2] = m_q;
      wml[r * 2 + 1] = l_q;
    }
  }
  __syncthreads();
  // the block's partial of (node q, dims d .. d + 3): the waves folded in wave order
  const int nq4 = hd >> 2;
  const size_t pairq = (size_t)(b * N) * a.n_head + head;  // + q * n_head per node
  for (int idx = tid; idx < N * nq4; idx += kTreeWaves * 64) {
    const int q = idx / nq4, d = (idx - q * nq4) * 4;
    float mw[kTreeWaves], M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < kTreeWaves; ww++) {
      mw[ww] = reinterpret_cast<const float*>(smem + ww * NSTG * TILEB + TILEB)[q * 2];
      M = fmaxf(M, mw[ww]);
    }
    float L = 0.f;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (M != -INFINITY) {  // a split without a live key for this node holds nothing
#pragma unroll
      for (int ww = 0; ww < kTreeWaves; ww++) {
        const float wgt = __expf(mw[ww] - M);  // idle waves: exp(-inf) = 0
        L += wgt * reinterpret_cast<const float*>(smem + ww * NSTG * TILEB + TILEB)[q * 2 + 1];
        acc += wgt * *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem + ww * NSTG * TILEB) + q * HDE + d);
      }
    }
    if (nsplit == 1) {  // every node sees itself: L > 0
      bf16* cp = (bf16*)a.ctx_out + (size_t)(b * N + q) * a.hidden + head * hd + d;
#pragma unroll
      for (int i = 0; i < 4; i++) cp[i] = from_f32<bf16>(acc[i] / L);
    } else {
      const size_t pq = (pairq + (size_t)q * a.n_head) * a.max_chunks;
#pragma unroll
      for (int i = 0; i < 4; i++) tree_store_sc1(acc[i], a.part_acc + pq * hd, (uint32_t)(sp * hd + d + i));
      if (d == 0) {
        tree_store_sc1(M, a.part_ml + pq * 2, (uint32_t)sp * 2);
        tree_store_sc1(L, a.part_ml + pq * 2, (uint32_t)sp * 2 + 1);
      }
    }
  }
  if (nsplit == 1) return;
  // ---- every storing wave drains its write-through stores, then one lane takes the (row, head) ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    typedef __attribute__((address_space(1))) unsigned gu32;
    unsigned* tk = a.tickets + (size_t)(a.slot + b) * a.n_head + head;
    const unsigned old = __hip_atomic_fetch_add((gu32*)tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == (unsigned)(nsplit - 1);
    if (last) __hip_atomic_store((gu32*)tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // zero between launches
  }
  __syncthreads();
  if (!last) return;
  // ---- the last arriver folds splits 0 .. nsplit - 1 in index order (sc1 loads, a group's loads in flight together)
  for (int i = tid; i < N * hd; i += kTreeWaves * 64) {
    const int q = i / hd, d = i - q * hd;
    const size_t pq = (pairq + (size_t)q * a.n_head) * a.max_chunks;
    const float* pacc_g = a.part_acc + pq * hd;
    const float* pml_g = a.part_ml + pq * 2;
    float mx = -INFINITY, acc2 = 0.f, lsum = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float m8[8], l8[8], o8[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int s = min(s0 + u, nsplit - 1);
        m8[u] = tree_load_sc1(pml_g, (uint32_t)s * 2);
        l8[u] = tree_load_sc1(pml_g, (uint32_t)s * 2 + 1);
        o8[u] = tree_load_sc1(pacc_g, (uint32_t)(s * hd + d));
      }
      float gm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; u++) gm = s0 + u < nsplit ? fmaxf(gm, m8[u]) : gm;
      const float nm = fmaxf(mx, gm);
      if (nm != -INFINITY) {
        const float sc = __expf(mx - nm);  // mx = -inf before the first split that holds a live key: 0
        acc2 *= sc;
        lsum *= sc;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          if (s0 + u < nsplit && m8[u] != -INFINITY) {
            const float wgt = __expf(m8[u] - nm);
            acc2 += wgt * o8[u];
            lsum += wgt * l8[u];
          }
        }
        mx = nm;
      }
    }
    ((bf16*)a.ctx_out)[(size_t)(b * N + q) * a.hidden + head * hd + d] = from_f32<bf16>(acc2 / lsum);
  }
}

// ---- bs_compact_kv
struct CompactArgs {
  char* base;                   // the stage's cache: n_lw images [max_batch][n_head][max_ctx] of pos_bytes each
  unsigned long long half;      // bytes of one image
  unsigned long long row_off;   // (slot * n_head) * seg_stride
  unsigned long long seg_stride;  // max_ctx * pos_bytes
  int past, n, pos_bytes;
  int src[kTreeMaxNodes];       // strictly increasing, src[k] >= k; src[k] = k beyond n
};

constexpr int kCompactThreads = 256;

__global__ __launch_bounds__(kCompactThreads) void kv_compact_kernel(CompactArgs c) {
  typedef unsigned int u4 __attribute__((ext_vector_type(4)));
  char* seg = c.base + (unsigned long long)blockIdx.y * c.half + c.row_off +
              (unsigned long long)blockIdx.x * c.seg_stride + (unsigned long long)c.past * c.pos_bytes;
  const int cpr = c.pos_bytes >> 4;  // 16-byte chunks per row: head_dim / 8 <= 16, so one lane holds one chunk
  const int k = threadIdx.x / cpr, ch = threadIdx.x - k * cpr;
  const bool live = k < c.n;
  int sk = k;  // src[k] by selects: the arguments stay in SGPRs
#pragma unroll
  for (int kk = 0; kk < kTreeMaxNodes; kk++) sk = k == kk ? c.src[kk] : sk;
  u4 v = (u4){0u, 0u, 0u, 0u};
  if (live) v = *reinterpret_cast<const u4*>(seg + (size_t)sk * c.pos_bytes + ch * 16);
  __syncthreads();  // every source row is in registers before any destination is written
  if (live && sk != k) *reinterpret_cast<u4*>(seg + (size_t)k * c.pos_bytes + ch * 16) = v;
}

template <int HDE>
void tree_launch(const AttnArgs& a, const TreeRow* table, int nsplit, hipStream_t s) {
  attn_tree_kernel<HDE><<<dim3(a.n_head, a.B, nsplit), kTreeWaves * 64, 0, s>>>(a, table);
}

}  // namespace

void launch_attention_tree(const AttnArgs& a, const TreeRow* table, hipStream_t s) {
  // a.max_chunks carries the split stride of the partials; the chunk count of the cache sizes the split rule
  const int chunks = (a.max_ctx + 63) / 64;
  const int nsplit = std::min(attention_decode_splits(a.B, a.n_head, chunks), a.max_chunks);
  if (a.head_dim <= 64) tree_launch<64>(a, table, nsplit, s);
  else if (a.head_dim <= 96) tree_launch<96>(a, table, nsplit, s);
  else tree_launch<128>(a, table, nsplit, s);
}

void launch_kv_compact(void* base, int n_lw, int n_head, int max_batch, int max_ctx, int head_dim, int slot, int past,
                       const int* src, int n, hipStream_t s) {
  CompactArgs c{};
  c.pos_bytes = head_dim * 2;
  c.seg_stride = (unsigned long long)max_ctx * c.pos_bytes;
  c.half = (unsigned long long)max_batch * n_head * c.seg_stride;
  c.row_off = (unsigned long long)slot * n_head * c.seg_stride;
  c.base = (char*)base;
  c.past = past;
  c.n = n;
  for (int k = 0; k < kTreeMaxNodes; k++) c.src[k] = k < n ? src[k] : k;
  kv_compact_kernel<<<dim3(n_head, n_lw), kCompactThreads, 0, s>>>(c);
}
