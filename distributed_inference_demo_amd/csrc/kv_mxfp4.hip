// kv_mxfp4.hip — BS_FLAG_MXFP4_KV (include/bloomstage.h): the KV cache as OCP MXFP4 along
// head_dim, one 16-byte record of 32 E2M1 codes and one E8M0 byte per block of 32 dims of a (position, head) vector.
// Codes [slot][head][pos][hd / 2], dim d of a vector in nibble d & 1 of byte d >> 1; scales [slot][head][pos][hd / 32].
// Three kernels:
//   attn_decode_fp4_kernel  S == 1: attention over the 4-bit cache; the call's own position comes from the bf16 staging
//                           row the QKV epilogue wrote, and one wave per (row, head) quantises that row into the cache
//   kv_dequant_fp4_kernel   S > 1 on rows with cached positions: cache [0, past_b) -> bf16 staging (exact)
//   kv_quant_fp4_kernel     S > 1: the call's S new staging rows -> cache
// A dequantised value is +-grid * 2^(E - 127): exact in bf16, so all three see the same numbers.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "mx4.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t fp4_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)0xFFFFFFFF, 0x00020000);
}

__device__ __forceinline__ float e8m0_f32(uint32_t E) { return __uint_as_float(E << 23); }  // 2^(E - 127)
__device__ __forceinline__ float bf16_lo(uint32_t pair) { return __uint_as_float(pair << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t pair) { return __uint_as_float(pair & 0xFFFF0000u); }
__device__ __forceinline__ bf16x2 as_bf16x2(uint32_t pair) { return __builtin_bit_cast(bf16x2, pair); }

// Sum over the 4 lanes that share a position (lanes 4g .. 4g+3).
__device__ __forceinline__ float sum4(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  return v;
}

// 32 bf16 values (16 dwords of pairs) -> the block's record and exponent byte.
__device__ __forceinline__ uint32_t quant_block(const u32x4* x, u32x4& rec) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t p = x[i][j];
      amax = fmaxf(amax, fmaxf(fabsf(bf16_lo(p)), fabsf(bf16_hi(p))));
    }
  float inv;
  const uint32_t E = mx4_block_exp(amax, inv);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t p = x[i][j];
      v |= (mx4_code(bf16_lo(p), inv) | (mx4_code(bf16_hi(p), inv) << 4)) << (8 * j);
    }
    rec[i] = v;
  }
  return E;
}

// Decode (S == 1) over the MXFP4 cache: attn_decode_kernel's grids, online softmax, partial format and three finishes
// (kernels.hip), with a work split of its own:
//   * a lane owns one 32-dim block of one position: one 16-B record and one exponent byte.  4 lanes hold a position
//     (hd = 64 / 96 mask the lanes past hd), so a load instruction of the wave covers 16 positions;
//   * a wave's chunk is CH = 128 positions (64 under the 8-wave split grid): CH / 16 record loads each for K and V,
//     16 KB of codes in flight per wave at CH = 128 -- what the int8 kernel holds for 64 positions;
//   * a byte of two codes becomes two scaled bf16 values (v_cvt_scalef32_pk_bf16_fp4, 2^(E - 127) the operand) and
//     meets q, held as 16 bf16 pairs in registers, on v_dot2c_f32_bf16; the 4 lanes' sums meet by DPP;
//   * P.V in fp32 per owned dim from v_cvt_scalef32_pk_f32_fp4; the wave's 16 position groups are summed at the end;
//   * position past_b (the new token) is taken from the bf16 staging row [B][head][hd], never from the cache;
//   * wave 0 of split 0 quantises that row into the cache at past_b (read by the NEXT launch): a lane takes a pair of
//     dims, a 16-lane DPP row is a block (amax by DPP, one exponent, two ladder codes, one byte per lane).
// past_len, the slope and q go out first as vector loads; the first chunk follows before past_len is known, clamped
// to the cache: positions past the context are masked (p = 0) and every record dequantises to a finite value
// (zero-initialised: code 0 under any exponent is 0; written from finite vectors: E <= 252), so they add exactly 0.
// A K / V vector that holds inf or NaN is outside that argument (E = 253, 6 * 2^126 overflows fp32, 0 * inf = NaN), as
// a non-finite vector is outside the int8 cache's; the rule in mx4.h is the weight quantiser's and is not clamped here.
template <int WV, int CH>
__global__ __launch_bounds__(WV * 64) void attn_decode_fp4_kernel(AttnArgs a, KvMx4 kq) {
  constexpr int NI = CH / 16;  // record loads per chunk and operand
  constexpr int PP = CH / 64;  // positions per lane in the softmax
  __shared__ float es[WV][CH];
  __shared__ float pm[WV], pl[WV];
  __shared__ float pacc[WV][128];
  __shared__ int last;
  const int head = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hd = a.head_dim, nb = hd >> 5, cb = hd >> 1;  // blocks and code bytes per position
  const size_t rowbase = ((size_t)(a.slot + b) * a.n_head + head) * a.max_ctx;
  uint8_t* kb = (uint8_t*)const_cast<void*>(a.k_cache) + rowbase * cb;
  uint8_t* vb = (uint8_t*)const_cast<void*>(a.v_cache) + rowbase * cb;
  uint8_t* ksb = kq.k_scale + rowbase * nb;
  uint8_t* vsb = kq.v_scale + rowbase * nb;
  const int grp = lane >> 2, dl = lane & 3;
  const bool dval = dl < nb;
  const int blk = dval ? dl : 0;  // masked lanes re-read block 0 of their own position (never summed)
  u32x4 kr[NI], vr[NI];
  uint32_t ke[NI], ve[NI];
  auto load_chunk = [&](int c, int lim) {
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const int pr = min(c * CH + it * 16 + grp, lim);
      kr[it] = *reinterpret_cast<const u32x4*>(kb + (size_t)pr * cb + blk * 16);
    }
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const int pr = min(c * CH + it * 16 + grp, lim);
      vr[it] = *reinterpret_cast<const u32x4*>(vb + (size_t)pr * cb + blk * 16);
    }
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const int pr = min(c * CH + it * 16 + grp, lim);
      ke[it] = ksb[(size_t)pr * nb + blk];
      ve[it] = vsb[(size_t)pr * nb + blk];
    }
  };
  // past_len, the slope and the lane's 32 q dims (bf16 pairs, kept as loaded) as vector loads (common.h lane_zero)
  int past_v = a.past;
  if (a.past_dev) past_v = a.past_dev[b + lane_zero()];
  const float slope = a.slopes[head + lane_zero()];
  u32x4 qr[4];
  {
    const u32x4* qp = reinterpret_cast<const u32x4*>((const bf16*)a.q + (size_t)b * a.hidden + head * hd + blk * 32);
#pragma unroll
    for (int i = 0; i < 4; i++) qr[i] = qp[i];
  }
  // the first chunk behind them, unconditional and clamped to the cache (a wave whose first chunk lies past the cache
  // re-reads its last position and never uses it); the scheduling barriers keep that order
  __builtin_amdgcn_sched_barrier(0);
  int c = w + WV * sp;
  load_chunk(c, a.max_ctx - 1);
  __builtin_amdgcn_sched_barrier(0);
  // wave 0 of split 0 (one per (row, head)) owns the new token: its bf16 K / V from the staging row, as this lane's
  // block (every position group holds the same row) and, to quantise it, as a pair of dims per lane
  const size_t srow = ((size_t)b * a.n_head + head) * hd;
  const bool owner = sp == 0 && w == 0;  // wave-uniform
  const bool qval = 2 * lane < hd;
  u32x4 kn[4], vn[4];
  uint32_t xk = 0, xv = 0;
  if (owner) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      kn[i] = reinterpret_cast<const u32x4*>(kq.k_stage + srow + blk * 32)[i];
      vn[i] = reinterpret_cast<const u32x4*>(kq.v_stage + srow + blk * 32)[i];
    }
    const int d = qval ? 2 * lane : 0;
    xk = *reinterpret_cast<const uint32_t*>(kq.k_stage + srow + d);
    xv = *reinterpret_cast<const uint32_t*>(kq.v_stage + srow + d);
  }
  const int past = __builtin_amdgcn_readfirstlane(past_v);  // uniform again: the chunk loop's bound stays scalar
  const int nch = (past + CH - 1) / CH;                     // chunks of cached positions [0, past)
  float m_run = -INFINITY, l_run = 0.f;
  f32x2 acc[16];  // the lane's 32 dims as the conversion's pairs: packed fp32 multiply-adds
#pragma unroll
  for (int j = 0; j < 16; j++) acc[j] = (f32x2){0.f, 0.f};
  if (owner) {
    // the online softmax starts from the new token (position past, weight e^0 = 1), at bf16; its V is counted once,
    // by position group 0.  kn / vn are dead before the chunk loop.
    float dnew = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t k0 = kn[i][0], k1 = kn[i][1], k2 = kn[i][2], k3 = kn[i][3];
      const uint32_t q0 = qr[i][0], q1 = qr[i][1], q2 = qr[i][2], q3 = qr[i][3];
      dnew = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(k0), as_bf16x2(q0), dnew, false);
      dnew = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(k1), as_bf16x2(q1), dnew, false);
      dnew = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(k2), as_bf16x2(q2), dnew, false);
      dnew = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(k3), as_bf16x2(q3), dnew, false);
    }
    m_run = slope * (float)past + a.inv_norm * sum4(dval ? dnew : 0.f);
    l_run = 1.f;
    if (grp == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t p = vn[i][j];
          acc[4 * i + j] = (f32x2){bf16_lo(p), bf16_hi(p)};
        }
    }
    // and the cache takes it, for the NEXT launch to read (this launch masks position past of the cache)
#pragma unroll
    for (int wch = 0; wch < 2; wch++) {
      const uint32_t x = wch ? xv : xk;
      float amax = qval ? fmaxf(fabsf(bf16_lo(x)), fabsf(bf16_hi(x))) : 0.f;
      amax = fmaxf(amax, dpp_f<0xB1>(amax));  // the block = the 16-lane DPP row (hd % 32 == 0: all valid or none)
      amax = fmaxf(amax, dpp_f<0x4E>(amax));
      amax = fmaxf(amax, dpp_f<0x124>(amax));
      amax = fmaxf(amax, dpp_f<0x128>(amax));
      float inv;
      const uint32_t E = mx4_block_exp(amax, inv);
      const uint32_t byte = mx4_code(bf16_lo(x), inv) | (mx4_code(bf16_hi(x), inv) << 4);
      if (qval) (wch ? vb : kb)[(size_t)past * cb + lane] = (uint8_t)byte;
      if (qval && (lane & 15) == 0) (wch ? vsb : ksb)[(size_t)past * nb + (lane >> 4)] = (uint8_t)E;
    }
  }
  for (; c < nch; c += WV * nsplit) {  // every visited chunk holds a cached position, so m_new below is finite
    if (c != w + WV * sp) load_chunk(c, past - 1);
    float sc[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const float ksf = e8m0_f32(ke[it]);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t codes = kr[it][i];
        const uint32_t q0 = qr[i][0], q1 = qr[i][1], q2 = qr[i][2], q3 = qr[i][3];
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, ksf, 0), as_bf16x2(q0), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, ksf, 1), as_bf16x2(q1), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, ksf, 2), as_bf16x2(q2), d, false);
        d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, ksf, 3), as_bf16x2(q3), d, false);
      }
      sc[it] = sum4(dval ? d : 0.f);
      __builtin_amdgcn_sched_barrier(0);  // one record at a time (the unrolled loop otherwise keeps every record's
    }                                     // converted values live at once and spills)
    if (dl == 0) {
#pragma unroll
      for (int it = 0; it < NI; it++) es[w][it * 16 + grp] = sc[it];
    }
    __builtin_amdgcn_wave_barrier();
    float s_me[PP], e[PP];
    float m_loc = -INFINITY;
#pragma unroll
    for (int u = 0; u < PP; u++) {
      const int p = c * CH + u * 64 + lane;
      s_me[u] = p < past ? slope * (float)p + a.inv_norm * es[w][u * 64 + lane] : -INFINITY;
      m_loc = fmaxf(m_loc, s_me[u]);
    }
    const float m_new = fmaxf(m_run, wave_max(m_loc));
    float e_sum = 0.f;
#pragma unroll
    for (int u = 0; u < PP; u++) {
      e[u] = __expf(s_me[u] - m_new);  // masked: exp(-inf) = 0
      e_sum += e[u];
    }
    const float scale = __expf(m_run - m_new);  // 0 on a first chunk (m_run = -inf)
    l_run = l_run * scale + wave_sum(e_sum);
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] *= scale;
    m_run = m_new;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < PP; u++) es[w][u * 64 + lane] = e[u];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const float ep = es[w][it * 16 + grp];
      const float vsf = e8m0_f32(ve[it]);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t codes = vr[it][i];
        acc[4 * i + 0] += ep * __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes, vsf, 0);
        acc[4 * i + 1] += ep * __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes, vsf, 1);
        acc[4 * i + 2] += ep * __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes, vsf, 2);
        acc[4 * i + 3] += ep * __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes, vsf, 3);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int j = 0; j < 32; j++) {  // sum over the wave's 16 position groups (lane bits 2..5)
    float v = acc[j >> 1][j & 1];
    v += dpp_f<0x124>(v);  // row_ror:4, row_ror:8: the 4 groups of a 16-lane row
    v += dpp_f<0x128>(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (grp == 0 && dval) pacc[w][dl * 32 + j] = v;
  }
  if (lane == 0) { pm[w] = m_run; pl[w] = l_run; }
  __syncthreads();
  // ---- the block's waves, then the three finishes: attn_decode_block's (kernels.hip), as in kv_int8.hip
  float M = -INFINITY, L = 0.f, o = 0.f;
  if (threadIdx.x < hd) {
    M = pm[0];
#pragma unroll
    for (int ww = 1; ww < WV; ww++) M = fmaxf(M, pm[ww]);
    if (M != -INFINITY) {  // a split past the context end holds no chunk
#pragma unroll
      for (int ww = 0; ww < WV; ww++) {
        const float wgt = __expf(pm[ww] - M);  // idle waves: exp(-inf) = 0
        L += wgt * pl[ww];
        o += wgt * pacc[ww][threadIdx.x];
      }
    }
  }
  bf16* ctx = (bf16*)a.ctx_out + (size_t)b * a.hidden + head * hd;
  if (nsplit == 1) {
    if (threadIdx.x < hd) ctx[threadIdx.x] = from_f32<bf16>(o / L);
    return;
  }
  const size_t pair = (size_t)(a.slot + b) * a.n_head + head;
  float* pacc_g = a.part_acc + pair * a.max_chunks * hd;  // [nsplit][hd]
  float* pml_g = a.part_ml + pair * a.max_chunks * 2;     // [nsplit][2]
  if (a.defer_merge) {  // the consumer merges (attn_merge.h): plain stores, the kernel boundary publishes
    if (threadIdx.x < hd) pacc_g[sp * hd + threadIdx.x] = o;
    if (threadIdx.x == 0) { pml_g[sp * 2] = M; pml_g[sp * 2 + 1] = L; }
    return;
  }
  // split partial (sc1 write-through), ticket, last arriver merges
  if (threadIdx.x < hd)
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), fp4_rsrc(pacc_g), (uint32_t)(sp * hd + threadIdx.x) * 4, 0, 16);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(M), fp4_rsrc(pml_g), (uint32_t)sp * 8, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(L), fp4_rsrc(pml_g), (uint32_t)sp * 8 + 4, 0, 16);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    typedef __attribute__((address_space(1))) unsigned gu32;
    const unsigned old = __hip_atomic_fetch_add((gu32*)(a.tickets + pair), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == (unsigned)(nsplit - 1);
    if (last) __hip_atomic_store((gu32*)(a.tickets + pair), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < hd) {
    float mx = -INFINITY, acc2 = 0.f, lsum = 0.f;
    for (int t0 = 0; t0 < nsplit; t0 += 16) {
      float m8[16], l8[16], o8[16];  // all of a group's loads in flight together
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int t = min(t0 + u, nsplit - 1);
        m8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(fp4_rsrc(pml_g), (uint32_t)t * 8, 0, 16));
        l8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(fp4_rsrc(pml_g), (uint32_t)t * 8 + 4, 0, 16));
        o8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(fp4_rsrc(pacc_g), (uint32_t)(t * hd + threadIdx.x) * 4, 0, 16));
      }
      float gm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 16; u++) gm = t0 + u < nsplit ? fmaxf(gm, m8[u]) : gm;
      const float nm = fmaxf(mx, gm);
      if (nm != -INFINITY) {
        const float sc2 = __expf(mx - nm);  // mx = -inf on the first group: 0
        acc2 *= sc2;
        lsum *= sc2;
#pragma unroll
        for (int u = 0; u < 16; u++) {
          if (t0 + u < nsplit && m8[u] != -INFINITY) {
            const float wgt = __expf(m8[u] - nm);
            acc2 += wgt * o8[u];
            lsum += wgt * l8[u];
          }
        }
        mx = nm;
      }
    }
    ctx[threadIdx.x] = from_f32<bf16>(acc2 / lsum);
  }
}

// Cache positions [0, past_b) of row b -> bf16 staging [B][head][lmax][hd] (the prefill attention's operand), exact.
// A thread owns one block of one position; block = 64 positions x 4 blocks; grid (head, b, ceil(max past / 64)).
__global__ __launch_bounds__(256) void kv_dequant_fp4_kernel(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                             KvMx4 kq, const int* __restrict__ past_dev, int slot,
                                                             int n_head, int hd, int max_ctx, int lmax) {
  const int head = blockIdx.x, b = blockIdx.y;
  const int pos = blockIdx.z * 64 + (threadIdx.x >> 2), dl = threadIdx.x & 3, nb = hd >> 5;
  if (pos >= past_dev[b] || dl >= nb) return;
  const size_t crow = ((size_t)(slot + b) * n_head + head) * max_ctx + pos;
  const size_t srow = ((size_t)b * n_head + head) * lmax + pos;
#pragma unroll
  for (int wch = 0; wch < 2; wch++) {
    const u32x4 rec = *reinterpret_cast<const u32x4*>((wch ? vc : kc) + crow * (hd >> 1) + dl * 16);
    const float sf = e8m0_f32((wch ? kq.v_scale : kq.k_scale)[crow * nb + dl]);
    u32x4* dst = reinterpret_cast<u32x4*>((wch ? kq.v_stage : kq.k_stage) + srow * hd + dl * 32);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t codes = rec[i];
      u32x4 o;
      o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sf, 0));
      o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sf, 1));
      o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sf, 2));
      o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sf, 3));
      dst[i] = o;
    }
  }
}

// Staging positions past_b .. past_b + S - 1 of every (row, head) -> records and exponent bytes at the same cache
// positions.  A thread owns one block of one vector (no cross-lane step); grid (head, b, ceil(S / 64)).
__global__ __launch_bounds__(256) void kv_quant_fp4_kernel(uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, KvMx4 kq,
                                                           const int* __restrict__ past_dev, int S, int slot, int n_head,
                                                           int hd, int max_ctx, int lmax) {
  const int head = blockIdx.x, b = blockIdx.y;
  const int t = blockIdx.z * 64 + (threadIdx.x >> 2), dl = threadIdx.x & 3, nb = hd >> 5;
  if (t >= S || dl >= nb) return;
  const int pos = past_dev[b] + t;
  const size_t crow = ((size_t)(slot + b) * n_head + head) * max_ctx + pos;
  const size_t srow = ((size_t)b * n_head + head) * lmax + pos;
#pragma unroll
  for (int wch = 0; wch < 2; wch++) {
    const u32x4* src = reinterpret_cast<const u32x4*>((wch ? kq.v_stage : kq.k_stage) + srow * hd + dl * 32);
    u32x4 x[4];
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = src[i];
    u32x4 rec;
    const uint32_t E = quant_block(x, rec);
    *reinterpret_cast<u32x4*>((wch ? vc : kc) + crow * (hd >> 1) + dl * 16) = rec;
    (wch ? kq.v_scale : kq.k_scale)[crow * nb + dl] = (uint8_t)E;
  }
}

}  // namespace

void launch_attention_fp4(const AttnArgs& a, const KvMx4& kq, hipStream_t s) {
  // attn_decode_kernel's grids (launch_attention, S == 1), twice its chunk: see the kernel's header
  const int nsplit = attention_decode_splits(a.B, a.n_head, a.max_chunks);
  if (nsplit == 1) {
    dim3 g(a.n_head, a.B, 1);
    if (a.B * a.n_head > 256) attn_decode_fp4_kernel<4, 128><<<g, 256, 0, s>>>(a, kq);
    else attn_decode_fp4_kernel<8, 128><<<g, 512, 0, s>>>(a, kq);
  } else if (a.defer_merge) {
    dim3 g(a.n_head, a.B, nsplit);
    attn_decode_fp4_kernel<8, 64><<<g, 512, 0, s>>>(a, kq);
  } else {
    dim3 g(a.n_head, a.B, nsplit);
    attn_decode_fp4_kernel<4, 128><<<g, 256, 0, s>>>(a, kq);
  }
}

void launch_kv_dequant_fp4(const void* k_codes, const void* v_codes, const KvMx4& kq, const int* past_dev, int B,
                           int slot, int n_head, int head_dim, int max_ctx, int lmax, int past_max, hipStream_t s) {
  if (past_max <= 0) return;
  dim3 g(n_head, B, (past_max + 63) / 64);
  kv_dequant_fp4_kernel<<<g, 256, 0, s>>>((const uint8_t*)k_codes, (const uint8_t*)v_codes, kq, past_dev, slot, n_head,
                                          head_dim, max_ctx, lmax);
}

void launch_kv_quant_fp4(void* k_codes, void* v_codes, const KvMx4& kq, const int* past_dev, int B, int S, int slot,
                         int n_head, int head_dim, int max_ctx, int lmax, hipStream_t s) {
  dim3 g(n_head, B, (S + 63) / 64);
  kv_quant_fp4_kernel<<<g, 256, 0, s>>>((uint8_t*)k_codes, (uint8_t*)v_codes, kq, past_dev, S, slot, n_head, head_dim,
                                        max_ctx, lmax);
}
