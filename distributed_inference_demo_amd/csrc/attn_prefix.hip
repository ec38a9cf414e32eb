// attn_prefix.hip — shared-prefix decode attention (bs_set_row_prefix): the B rows of a decode step whose first npos
// cached positions hold the same bits stream that prefix ONCE per head instead of once per (row, head).  bf16 stages,
// head_dim <= 128, 2 <= B <= 32.  Compiled like attn_prefill.hip with -mllvm -amdgpu-mfma-vgpr-form=1 (build.py): the
// P.V accumulators stay in VGPRs and the per-chunk rescale is plain VALU.
//
// Two launches replace launch_attention; the kernel boundary publishes the partials (no tickets, no write-through
// protocol, no floating-point atomics: bit-identical from run to run).  Both read (src_slot, npos) from the device
// table entry of the call's first row, so a replayed graph follows a later bs_set_row_prefix of the same shape.
//
// (a) attn_prefix_kernel, grid (n_head, nsplit), 4 waves.  nsplit is a function of the stage alone
//     (attention_prefix_splits).  64-position chunk c of src_slot's row belongs to split c % nsplit and there to wave
//     (c / nsplit) % 4: the live chunks spread over the splits whatever npos is, and a split without a chunk stores
//     (m = -inf, l = 0).  Each wave walks its own chunks against the queries of ALL B rows of the head:
//      * S^T = K.Q^T on v_mfma_f32_16x16x32_bf16.  A K fragment is 16 contiguous bytes of a cache row (8 dims of one
//        position), loaded from global memory straight into the A operand -- no LDS, no shuffle; Q is the B operand,
//        in registers for the whole loop; B is padded to QG = 1 or 2 tiles of 16 query rows (rows >= B hold zeros and
//        are never stored), head_dim to HDE = 64 / 96 / 128 with zeros;
//      * scores = slope_h * pos + q.k / sqrt(hd) in fp32, positions >= npos masked, one fp32 online softmax per query
//        row (lane (r, g) holds 16 of the chunk's scores of query r; the four g lanes meet by v_permlane swaps); a
//        chunk that contributes nothing leaves the state alone;
//      * P.V as attn_prefill.hip does it: O^T = V^T . P^T, P = bf16(p) + bf16(p - bf16(p)) as two B operands, V by
//        LDS-DMA into the wave's own two-stage ring in the swizzled [64][128 x 16-bit] image and out of it with
//        ds_read_b64_tr_b16; normalisation is left to the merge;
//      * the next chunk's K loads and V DMA are issued behind the chunk's score MFMAs and stay in flight through its
//        softmax and P.V.  The ring is the wave's own: no block barrier in the loop.
//     The waves' (m, l, o) meet in LDS and are folded in wave order; (m, l, acc[hd]) per (row, head, split) go out
//     with plain stores.
// (b) attn_suffix_merge_kernel, grid (n_head, B), 4 waves: the row's own positions [npos, past_b] (the new token
//     included: the QKV epilogue wrote it) with the decode kernel's arithmetic -- 16 lanes per cache row, fp32 dot
//     products, one online softmax per wave, waves folded in wave order through LDS -- then the prefix partials of
//     the (row, head) over splits 0 .. nsplit - 1 in index order, then the suffix partial, and bf16 ctx.  Suffixes
//     are short by construction; a long one is served correctly but by one block per (row, head).
// Neither kernel reads a position < npos of any row but src_slot, nor any position > past_b.
#include <algorithm>
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kPfxWaves = 4;

__device__ __forceinline__ int pfx_tr_off(int row, int ch) {  // attn_prefill.hip attn_tr_off: the [64][128] bf16 image
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
__device__ __forceinline__ float pfx_xmax(float v) {  // over the lanes l, l ^ 16, l ^ 32, l ^ 48
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float pfx_xsum(float v) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__global__ void prefix_table_kernel(PrefixRow* table, int slot, int count, PrefixRow v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) table[slot + i] = v;
}

// a.part_acc / a.part_ml: the prefix partials [kPrefixMaxRows][n_head][a.max_chunks (= nsplit)][hd] and [..][2].
template <int HDE, int QG>
__global__ __launch_bounds__(kPfxWaves * 64) void attn_prefix_kernel(AttnArgs a, const PrefixRow* table) {
  constexpr int KT = 64, TILEB = KT * 256, NSTG = 2;
  constexpr int KSE = HDE / 32, NTE = HDE / 16;
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  typedef __attribute__((address_space(3))) void lds_void;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kPfxWaves * NSTG * TILEB];
  const int head = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PrefixRow pr = table[a.slot];
  const int npos = min(pr.npos, a.max_ctx);
  const int hd = a.head_dim, nch = hd >> 3;
  const size_t rowbase = ((size_t)pr.src_slot * a.n_head + head) * a.max_ctx;
  const int cbytes = a.max_ctx * hd * 2;  // rows past max_ctx read 0 through the bounded descriptors
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
  // Q of rows 16 j + r (zero past B and past head_dim)
  bf16x8 qf[QG][KSE];
#pragma unroll
  for (int j = 0; j < QG; j++) {
    const int b = 16 * j + r;
    const bf16* qp = (const bf16*)a.q + (size_t)min(b, a.B - 1) * a.hidden + head * hd;
#pragma unroll
    for (int ks = 0; ks < KSE; ks++) {
      const int d = ks * 32 + 8 * g;
      qf[j][ks] = (d < hd && b < a.B) ? *reinterpret_cast<const bf16x8*>(qp + d) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const float slope = a.slopes[head];
  const int nlive = (npos + KT - 1) / KT;
  const int cstep = nsplit * kPfxWaves;
  int c = sp + nsplit * w;
  if (c < nlive) {
    load_k(c * KT);
    issue_v(0, c * KT);
  }
  float m_q[QG], l_q[QG];
  f32x4 o[QG][NTE];  // o[j][t][i]: unnormalised context of query 16 j + r, dim 16 t + 4 g + i
#pragma unroll
  for (int j = 0; j < QG; j++) {
    m_q[j] = -INFINITY;
    l_q[j] = 0.f;
#pragma unroll
    for (int t = 0; t < NTE; t++) o[j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const int qq = r >> 2, pp = r & 3;
  for (int it = 0; c < nlive; c += cstep, it++) {
    const int st = it & 1, k0 = c * KT;
    // the chunk's K registers and V stage have landed; the other stage's reads (chunk it - 1) have retired
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    f32x4 sacc[QG][4];  // sacc[j][t][i]: key k0 + 16 t + 4 perm(g) + i against query 16 j + r
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int j = 0; j < QG; j++) {
        sacc[j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSE; ks++)
          sacc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[j][ks], sacc[j][t], 0, 0, 0);
      }
    float sv[QG][4][4];
    const bool full = k0 + KT <= npos;
#pragma unroll
    for (int j = 0; j < QG; j++)
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int kpos = k0 + t * 16 + 4 * pg4 + i;
          const float s = fmaf(a.inv_norm, sacc[j][t][i], slope * (float)kpos);
          sv[j][t][i] = (full || kpos < npos) ? s : -INFINITY;
        }
    // the next chunk: K into the registers the MFMAs above have consumed, V into the other stage
    asm volatile("" ::: "memory");
    if (c + cstep < nlive) {
      load_k((c + cstep) * KT);
      issue_v(st ^ 1, (c + cstep) * KT);
    }
    bf16x8 ph[QG][2], pl[QG][2];
#pragma unroll
    for (int j = 0; j < QG; j++) {
      float rmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) rmax = fmaxf(rmax, sv[j][t][i]);
      rmax = pfx_xmax(rmax);
      const float m_new = fmaxf(m_q[j], rmax);
      const float scale_q = m_new == -INFINITY ? 1.f : __expf(m_q[j] - m_new);
      float rs = 0.f;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float p = m_new == -INFINITY ? 0.f : __expf(sv[j][t][i] - m_new);
          sv[j][t][i] = p;
          rs += p;
        }
      rs = pfx_xsum(rs);
      l_q[j] = l_q[j] * scale_q + rs;
      m_q[j] = m_new;
#pragma unroll
      for (int t = 0; t < NTE; t++) o[j][t] *= scale_q;
      // P^T (B operand of step kb): element e = key 32 kb + 16 (e >> 2) + 4 perm(g) + (e & 3) of query r; hi + lo
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float p = sv[j][2 * kb + (e >> 2)][e & 3];
          const bf16 hi = (bf16)p;
          ph[j][kb][e] = hi;
          pl[j][kb][e] = (bf16)(p - (float)hi);
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
            (lds_s16x4*)(vs_ + pfx_tr_off(rw0, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s16x4*)(vs_ + pfx_tr_off(rw0 + 16, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const bf16x8 vf = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
#pragma unroll
        for (int j = 0; j < QG; j++) {
          o[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, ph[j][kb], o[j][t], 0, 0, 0);
          o[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl[j][kb], o[j][t], 0, 0, 0);
        }
      }
  }
  // ---- the waves' (m, l, o) meet in LDS (each wave's own ring: o in stage 0, m / l in stage 1)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  {
    float* wo = reinterpret_cast<float*>(ring);
    float* wml = reinterpret_cast<float*>(ring + TILEB);
#pragma unroll
    for (int j = 0; j < QG; j++) {
#pragma unroll
      for (int t = 0; t < NTE; t++) *reinterpret_cast<f32x4*>(wo + (16 * j + r) * HDE + 16 * t + 4 * g) = o[j][t];
      if (g == 0) {
        wml[(16 * j + r) * 2] = m_q[j];
        wml[(16 * j + r) * 2 + 1] = l_q[j];
      }
    }
  }
  __syncthreads();
  // the block's partial of (row q, dims d .. d + 3): the waves folded in wave order
  const int nq4 = hd >> 2;
  for (int idx = tid; idx < a.B * nq4; idx += kPfxWaves * 64) {
    const int q = idx / nq4, d = (idx - q * nq4) * 4;
    float mw[kPfxWaves], M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < kPfxWaves; ww++) {
      mw[ww] = reinterpret_cast<const float*>(smem + ww * NSTG * TILEB + TILEB)[q * 2];
      M = fmaxf(M, mw[ww]);
    }
    float L = 0.f;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (M != -INFINITY) {  // a split without a chunk holds nothing
#pragma unroll
      for (int ww = 0; ww < kPfxWaves; ww++) {
        const float wgt = __expf(mw[ww] - M);  // idle waves: exp(-inf) = 0
        L += wgt * reinterpret_cast<const float*>(smem + ww * NSTG * TILEB + TILEB)[q * 2 + 1];
        acc += wgt * *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem + ww * NSTG * TILEB) + q * HDE + d);
      }
    }
    const size_t rec = ((size_t)q * a.n_head + head) * nsplit + sp;
    *reinterpret_cast<f32x4*>(a.part_acc + rec * hd + d) = acc;
    if (d == 0) {
      a.part_ml[rec * 2] = M;
      a.part_ml[rec * 2 + 1] = L;
    }
  }
}

// The row's own positions and the merge; the decode kernel's arithmetic (attn_verify.hip with one query).
__global__ __launch_bounds__(kPfxWaves * 64) void attn_suffix_merge_kernel(AttnArgs a, const PrefixRow* table) {
  constexpr int WV = kPfxWaves, CH = 64, NI = CH / 4;
  __shared__ __attribute__((aligned(16))) float qs[128];
  __shared__ float es[WV][64];
  __shared__ float pm[WV], pl[WV];
  __shared__ float pacc[WV][128];
  const int head = blockIdx.x, b = blockIdx.y, nsplit = a.max_chunks;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hd = a.head_dim;
  const size_t rowbase = ((size_t)(a.slot + b) * a.n_head + head) * a.max_ctx;
  const bf16* kb = (const bf16*)a.k_cache + rowbase * hd;
  const bf16* vb = (const bf16*)a.v_cache + rowbase * hd;
  const int grp = lane >> 4, dl = lane & 15;
  const bool dval = dl * 8 < hd;
  const int doff = dval ? dl * 8 : 0;  // masked lanes re-read dims 0..7 (their products are dropped)
  const float slope = a.slopes[head];
  const int npos = table[a.slot].npos;
  const int nk = min(a.past_dev[b] + 1, a.max_ctx);  // the new token sits at past_b
  const int nlast = nk - 1;
  const int nch = nk > npos ? (nk - npos + CH - 1) / CH : 0;
  for (int i = threadIdx.x; i < hd; i += WV * 64)
    qs[i] = to_f32(((const bf16*)a.q)[(size_t)b * a.hidden + head * hd + i]);
  __syncthreads();
  float m_run = -INFINITY, l_run = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
  const float4 q0 = *reinterpret_cast<const float4*>(&qs[doff]);
  const float4 q1 = *reinterpret_cast<const float4*>(&qs[doff + 4]);
  const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  for (int c = w; c < nch; c += WV) {
    const int p0 = npos + c * CH;
    u16x8 kr[NI], vr[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) raw_load(kb + (size_t)min(p0 + it * 4 + grp, nlast) * hd + doff, kr[it]);
#pragma unroll
    for (int it = 0; it < NI; it++) raw_load(vb + (size_t)min(p0 + it * 4 + grp, nlast) * hd + doff, vr[it]);
#pragma unroll
    for (int it = 0; it < NI; it++) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; j++) d += qv[j] * raw_get(kr[it], j);
      d = dval ? d : 0.f;
      d += dpp_f<0xB1>(d);
      d += dpp_f<0x4E>(d);
      d += dpp_f<0x124>(d);
      d += dpp_f<0x128>(d);
      if (dl == 0) es[w][it * 4 + grp] = d;
    }
    __builtin_amdgcn_wave_barrier();
    const int p = p0 + lane;
    const bool live = p < nk;
    const float s_me = live ? slope * (float)p + a.inv_norm * es[w][lane] : -INFINITY;
    const float m_new = fmaxf(m_run, wave_max(s_me));  // finite: the chunk's first position is < nk
    const float e = live ? __expf(s_me - m_new) : 0.f;
    const float scale = m_new == -INFINITY ? 0.f : __expf(m_run - m_new);
    l_run = l_run * scale + wave_sum(e);
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] *= scale;
    m_run = m_new;
    es[w][lane] = e;  // each lane replaces the score it alone read
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const float ep = es[w][it * 4 + grp];
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] += ep * raw_get(vr[it], j);
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float v = acc[j];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (grp == 0 && dval) pacc[w][dl * 8 + j] = v;
  }
  if (lane == 0) { pm[w] = m_run; pl[w] = l_run; }
  __syncthreads();
  const int d = threadIdx.x;
  if (d >= hd) return;
  // one online fold per context element: the prefix splits in index order, then the suffix (its waves in wave order)
  float mx = -INFINITY, o = 0.f, ls = 0.f;
  auto fold = [&](float m, float l, float v) {
    if (m == -INFINITY) return;  // a split or a wave that holds nothing
    const float nm = fmaxf(mx, m);
    const float sc = __expf(mx - nm), wgt = __expf(m - nm);  // mx = -inf before the first contribution: 0
    o = o * sc + wgt * v;
    ls = ls * sc + wgt * l;
    mx = nm;
  };
  const size_t rec = ((size_t)b * a.n_head + head) * nsplit;
  for (int s = 0; s < nsplit; s++) fold(a.part_ml[(rec + s) * 2], a.part_ml[(rec + s) * 2 + 1], a.part_acc[(rec + s) * hd + d]);
  float M = pm[0];
#pragma unroll
  for (int ww = 1; ww < WV; ww++) M = fmaxf(M, pm[ww]);
  if (M != -INFINITY) {
    float L = 0.f, so = 0.f;
#pragma unroll
    for (int ww = 0; ww < WV; ww++) {
      const float wgt = __expf(pm[ww] - M);  // idle waves: exp(-inf) = 0
      L += wgt * pl[ww];
      so += wgt * pacc[ww][d];
    }
    fold(M, L, so);
  }
  ((bf16*)a.ctx_out)[(size_t)b * a.hidden + head * hd + d] = from_f32<bf16>(o / ls);
}

template <int HDE>
void prefix_launch(const AttnArgs& a, const PrefixRow* table, hipStream_t s) {
  const dim3 g(a.n_head, a.max_chunks), blk(kPfxWaves * 64);
  if (a.B > 16) attn_prefix_kernel<HDE, 2><<<g, blk, 0, s>>>(a, table);
  else attn_prefix_kernel<HDE, 1><<<g, blk, 0, s>>>(a, table);
}

}  // namespace

int attention_prefix_splits(int n_head, int max_ctx) {
  const int chunks = (max_ctx + 63) / 64;
  // one chunk per wave of a block at the longest prefix, about one block per CU slot, and a bounded merge loop
  return std::max(1, std::min({(chunks + kPfxWaves - 1) / kPfxWaves, std::max(1, 256 / n_head), kPrefixMaxSplits}));
}

void launch_prefix_table(PrefixRow* table, int slot, int count, int src_slot, int npos, hipStream_t s) {
  prefix_table_kernel<<<(count + 63) / 64, 64, 0, s>>>(table, slot, count, PrefixRow{src_slot, npos});
}

void launch_attention_prefix(const AttnArgs& a, const PrefixRow* table, hipStream_t s) {
  if (a.head_dim <= 64) prefix_launch<64>(a, table, s);
  else if (a.head_dim <= 96) prefix_launch<96>(a, table, s);
  else prefix_launch<128>(a, table, s);
  attn_suffix_merge_kernel<<<dim3(a.n_head, a.B), kPfxWaves * 64, 0, s>>>(a, table);
}
