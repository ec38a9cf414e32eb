// attn_ragged.hip — ragged prefill attention (bs_forward_ragged): the rows of one pass differ in length and in how
// many positions their KV rows already hold.  bf16 stages, head_dim % 8 == 0 and <= 128 (padded to 64 / 96 / 128).
// Compiled like attn_prefix.hip (build.py): the P.V accumulators stay in VGPRs, no packed fp32 arithmetic.
//
// The pass's tokens are packed in row order (row b owns tokens [t0_b, t0_b + S_b)); its QKV epilogue has written q
// to [T][hidden] and the new K / V to two staging buffers [n_head][T][hd].  One launch does the attention of every
// row AND moves the new K / V into the cache:
//
//  * work list: grid (items, n_head), an item = one 64-query tile of one row (the host builds the list, longest key
//    walk first), so short rows cost one block per head and no grid is sized by the longest row.  4 waves; wave w
//    owns queries 64 qt + 16 w .. + 15 of the tile and walks ALL of the tile's keys on its own: Q stays in registers,
//    K fragments come from global memory straight into the A operand, V goes by LDS-DMA into the wave's own two-stage
//    ring -- no block barrier anywhere, and a wave whose 16 queries lie past S_b leaves at once (a one-token row is
//    one live wave with 15 padded queries: zero, never stored).  The four waves of a tile read the same K / V; the
//    re-reads hit L2, and the route's target is many short rows, where most tiles hold one or two live waves.
//  * two slabs, walked in turn in 64-key tiles: the cached past cache[slot_b][head][0, past_b), then the pass's own
//    positions staging[head][t0_b, t0_b + S_b) under the causal mask.  A tile never straddles the slabs: per tile
//    the (wave-uniform) base pointer and byte bound of its slab go into the buffer descriptor, and everything past
//    the slab's end reads 0 through that bound -- the kernel never reads a cache position >= past_b of any row.
//  * scores = slope_h * (absolute position) + q.k / sqrt(hd) in fp32, S^T = K.Q^T on v_mfma_f32_16x16x32_bf16, one
//    fp32 online softmax per query (lane (r, g) holds 16 of the tile's scores of query r; the four g lanes meet by
//    v_permlane swaps); a tile that holds nothing live for a query leaves its state alone (m_new == -inf).
//  * P.V as attn_prefill.hip does it: O^T = V^T . P^T, P = bf16(p) + bf16(p - bf16(p)) as two B operands, V out of
//    the swizzled [64][128 x 16-bit] image with ds_read_b64_tr_b16.  The next tile's K loads and V DMA are issued
//    behind the tile's score MFMAs and stay in flight through its softmax and P.V.
//  * cache write in the same launch: the block of query tile 0 of each (row, head) copies the row's S_b x hd new K
//    and V values from staging to cache[slot_b][head][past_b, past_b + S_b), 16 B per lane.  No block of the launch
//    reads those cache positions (they are read from staging), the next launch sees them across the kernel boundary:
//    no scatter launch, no ticket.  Nothing at or beyond past_b + S_b is written, no other row is touched.
// Bit-identical from run to run: no atomics, every query's keys are folded in position order by one wave.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kRagWaves = 4;

__device__ __forceinline__ int rag_tr_off(int row, int ch) {  // attn_prefill.hip attn_tr_off: the [64][128] bf16 image
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
__device__ __forceinline__ float rag_xmax(float v) {  // over the lanes l, l ^ 16, l ^ 32, l ^ 48
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float rag_xsum(float v) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int HDE>
__global__ __launch_bounds__(kRagWaves * 64) void attn_ragged_kernel(RaggedArgs a) {
  constexpr int KT = 64, QB = 64, TILEB = KT * 256, NSTG = 2;
  constexpr int KSE = HDE / 32, NTE = HDE / 16;
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  typedef __attribute__((address_space(3))) void lds_void;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kRagWaves * NSTG * TILEB];
  const int head = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const RaggedWork item = a.work[blockIdx.x];
  const RaggedRow row = a.rows[item.row];
  const int qt = item.qtile, S = row.S, past = row.past;
  const int hd = a.head_dim, nch = hd >> 3;
  // the two slabs of this (row, head): elements
  const size_t cbase = (((size_t)row.slot * a.n_head + head) * a.max_ctx) * hd;
  const size_t sbase = ((size_t)head * a.T + row.t0) * hd;
  const bf16* kpast = (const bf16*)a.k_cache + cbase;
  const bf16* vpast = (const bf16*)a.v_cache + cbase;
  const bf16* knew = (const bf16*)a.k_stage + sbase;
  const bf16* vnew = (const bf16*)a.v_stage + sbase;

  // ---- the in-launch cache write: query tile 0's block moves the row's new K / V, 16 B per lane
  if (qt == 0) {
    const int n16 = S * nch;  // 16-byte pieces of one of K / V
    uint4* kd = reinterpret_cast<uint4*>((bf16*)a.k_cache + cbase + (size_t)past * hd);
    uint4* vd = reinterpret_cast<uint4*>((bf16*)a.v_cache + cbase + (size_t)past * hd);
    const uint4* ks = reinterpret_cast<const uint4*>(knew);
    const uint4* vs = reinterpret_cast<const uint4*>(vnew);
    for (int i = tid; i < n16; i += kRagWaves * 64) {
      const uint4 kk = ks[i], vv = vs[i];
      kd[i] = kk;
      vd[i] = vv;
    }
  }
  const int q0 = qt * QB + w * 16;  // the wave's first query (index among the row's new tokens)
  if (q0 >= S) return;              // nothing of this wave's is stored; the kernel has no block barrier

  unsigned char* ring = smem + w * NSTG * TILEB;  // this wave's V stages
  // V DMA: piece pc (1 KB = 4 rows) of a tile; lane l writes LDS chunk l & 15 of row 4 pc + (l >> 4) and fetches that
  // row's logical chunk (l & 15) ^ swz(row).  The lane offsets repeat every 4 pieces (16 rows).
  uint32_t voff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int rw = 4 * i + (lane >> 4);
    const int x = (lane & 15) ^ (((lane >> 4) << 2) | i);
    voff[i] = (uint32_t)(rw * hd * 2 + min(x, nch - 1) * 16);
  }
  // tile i of the walk: past tiles 0 .. npt - 1, then the new positions' tiles 0 .. qt
  const int npt = (past + KT - 1) / KT;
  const int ntile = npt + qt + 1;
  auto slab_k = [&](int i) {  // bounded at the slab's end: rows past it read 0
    const bool p = i < npt;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p ? kpast : knew), (short)0, (p ? past : S) * hd * 2,
                                             0x00020000);
  };
  auto slab_v = [&](int i) {
    const bool p = i < npt;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p ? vpast : vnew), (short)0, (p ? past : S) * hd * 2,
                                             0x00020000);
  };
  auto tile_k0 = [&](int i) { return (i < npt ? i : i - npt) * KT; };  // first key of the tile inside its slab
  auto issue_v = [&](int st, int i) {
    const __amdgpu_buffer_rsrc_t rv = slab_v(i);
    const int k0 = tile_k0(i);
#pragma unroll
    for (int pc = 0; pc < 16; pc++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_void*)(ring + st * TILEB + pc * 1024), 16, voff[pc & 3],
                                               (k0 + (pc >> 2) * 16) * hd * 2, 0, 0);
  };
  // A row r of subtile t is key 16 t + arow (the permutation that makes the transposed V reads conflict-free)
  const int pg4 = ((g & 1) << 1) | (g >> 1);
  const int arow = ((((r >> 2) & 1) << 1) | (r >> 3)) * 4 + (r & 3);
  bf16x8 kf[4][KSE];
  auto load_k = [&](int i) {
    const __amdgpu_buffer_rsrc_t rk = slab_k(i);
    const int k0 = tile_k0(i);
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
  // Q of query q0 + r (zero past S and past head_dim)
  const int qrel = q0 + r;
  bf16x8 qf[KSE];
  {
    const bf16* qp = (const bf16*)a.q + (size_t)(row.t0 + min(qrel, S - 1)) * a.hidden + head * hd;
#pragma unroll
    for (int ks = 0; ks < KSE; ks++) {
      const int d = ks * 32 + 8 * g;
      qf[ks] = (d < hd && qrel < S) ? *reinterpret_cast<const bf16x8*>(qp + d) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const float slope = a.slopes[head];
  load_k(0);
  issue_v(0, 0);
  float m_q = -INFINITY, l_q = 0.f;
  f32x4 o[NTE];  // o[t][i]: unnormalised context of query q0 + r, dim 16 t + 4 g + i
#pragma unroll
  for (int t = 0; t < NTE; t++) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int qq = r >> 2, pp = r & 3;
  for (int it = 0; it < ntile; it++) {
    const int st = it & 1, k0 = tile_k0(it);
    const bool inpast = it < npt;
    // the tile's K registers and V stage have landed; the other stage's reads (tile it - 1) have retired
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    f32x4 sacc[4];  // sacc[t][i]: key k0 + 16 t + 4 perm(g) + i of the slab against query q0 + r
#pragma unroll
    for (int t = 0; t < 4; t++) {
      sacc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSE; ks++)
        sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[ks], sacc[t], 0, 0, 0);
    }
    // past slab: every key precedes every query, masked at past; new slab: key j <= query i, masked at S.
    // apos: the absolute position of the slab's key 0
    const int klim = inpast ? past : S, apos = inpast ? 0 : past;
    const int qlim = inpast ? 0x7fffffff : qrel;
    const bool full = k0 + KT <= klim && (inpast || k0 + KT - 1 <= q0);  // wave-uniform: no element is masked
    float sv[4][4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        sv[t][i] = fmaf(a.inv_norm, sacc[t][i], slope * (float)(apos + k0 + t * 16 + 4 * pg4 + i));
    if (!full) {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int kk = k0 + t * 16 + 4 * pg4 + i;
          sv[t][i] = (kk < klim) & (kk <= qlim) ? sv[t][i] : -INFINITY;
        }
    }
    // the next tile: K into the registers the MFMAs above have consumed, V into the other stage
    asm volatile("" ::: "memory");
    if (it + 1 < ntile) {
      load_k(it + 1);
      issue_v(st ^ 1, it + 1);
    }
    float rmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) rmax = fmaxf(rmax, sv[t][i]);
    rmax = rag_xmax(rmax);
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
    rs = rag_xsum(rs);
    l_q = l_q * scale_q + rs;
    m_q = m_new;
#pragma unroll
    for (int t = 0; t < NTE; t++) o[t] *= scale_q;
    // P^T (B operand of step kb): element e = key 32 kb + 16 (e >> 2) + 4 perm(g) + (e & 3) of query r; hi + lo
    bf16x8 ph[2], pl[2];
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float p = sv[2 * kb + (e >> 2)][e & 3];
        const bf16 hi = (bf16)p;
        ph[kb][e] = hi;
        pl[kb][e] = (bf16)(p - (float)hi);
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
            (lds_s16x4*)(vs_ + rag_tr_off(rw0, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_s16x4*)(vs_ + rag_tr_off(rw0 + 16, 2 * t + (pp >> 1)) + 8 * (pp & 1)));
        const bf16x8 vf = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, ph[kb], o[t], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pl[kb], o[t], 0, 0, 0);
      }
  }
  // ---- context rows through the wave's own LDS (16 x 128 bf16 in its stage 0), then 16-B row stores
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the last tile's transposed reads have retired
  bf16* cs = reinterpret_cast<bf16*>(ring);
  {
    const float inv = 1.0f / l_q;  // a padded query may hold l = 0: never stored
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int t = 0; t < NTE; t++) {
      bf16x4 v4;
#pragma unroll
      for (int i = 0; i < 4; i++) v4[i] = (bf16)(o[t][i] * inv);
      *reinterpret_cast<bf16x4*>(cs + r * 128 + t * 16 + 4 * g) = v4;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own LDS writes before its reads
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int c = i * 64 + lane, ql = c >> 4, ch = c & 15, q = q0 + ql;
    if (ch < nch && q < S)
      *reinterpret_cast<bf16x8*>((bf16*)a.ctx_out + (size_t)(row.t0 + q) * a.hidden + head * hd + ch * 8) =
          *reinterpret_cast<const bf16x8*>(cs + ql * 128 + ch * 8);
  }
}

// out[b][0..h) = x[last[b]][0..h): the last-token hidden rows of the pass, 16 B per lane (h % 4 == 0)
__global__ void ragged_gather_kernel(const float* x, const RaggedRow* rows, float* out, int h4) {
  const RaggedRow rw = rows[blockIdx.x];
  const float4* src = reinterpret_cast<const float4*>(x) + (size_t)(rw.t0 + rw.S - 1) * h4;
  float4* dst = reinterpret_cast<float4*>(out) + (size_t)blockIdx.x * h4;
  for (int i = threadIdx.x; i < h4; i += blockDim.x) dst[i] = src[i];
}

}  // namespace

void launch_attention_ragged(const RaggedArgs& a, hipStream_t s) {
  const dim3 g(a.nwork, a.n_head), blk(kRagWaves * 64);
  if (a.head_dim <= 64) attn_ragged_kernel<64><<<g, blk, 0, s>>>(a);
  else if (a.head_dim <= 96) attn_ragged_kernel<96><<<g, blk, 0, s>>>(a);
  else attn_ragged_kernel<128><<<g, blk, 0, s>>>(a);
}

void launch_ragged_gather(const float* x, const RaggedRow* rows, float* out, int B, int hidden, hipStream_t s) {
  ragged_gather_kernel<<<B, 256, 0, s>>>(x, rows, out, hidden / 4);
}
