// kv_int8.hip — BS_FLAG_INT8_KV (include/bloomstage.h): the KV cache as int8 codes + one fp32 scale per
// (position, head) vector.  Three kernels:
//   attn_decode_q8_kernel  S == 1: attention over the int8 cache; the call's own position comes from the bf16 staging
//                          row the QKV epilogue wrote, and one block per (row, head) quantises that row into the cache
//   kv_dequant_kernel      S > 1 on rows with cached positions: cache [0, past_b) -> bf16 staging
//   kv_quant_kernel        S > 1: the call's S new staging rows -> cache
// Rule (quantize_rows_kernel's arithmetic): scale = amax > 0 ? amax / 127.f : 1.f, q = clamp(rintf(x / scale), +-127),
// value = (float)q * scale.  head_dim % 16 == 0: a lane owns 16 dims (one 16-B load of codes), 8 lanes one hd = 128 row.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ __amdgpu_buffer_rsrc_t q8_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)0xFFFFFFFF, 0x00020000);
}

typedef int i32x4q __attribute__((ext_vector_type(4)));

// Reductions over the 8 lanes that share a row (lanes 8g .. 8g+7): xor 1, xor 2, then the half-row mirror.
__device__ __forceinline__ float sum8(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);  // row_half_mirror
  return v;
}
__device__ __forceinline__ float max8(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  return v;
}

__device__ __forceinline__ float code_f32(const i32x4q& r, int j) {  // code j of 16, sign-extended
  return (float)((r[j >> 2] << (24 - 8 * (j & 3))) >> 24);
}

// 16 bf16 values of a staging row as fp32
__device__ __forceinline__ void load16(const bf16* p, float* o) {
  load8(p, o);
  load8(p + 8, o + 8);
}

// The lane's 16 values -> codes under the 8-lane group's scale; returns the scale.
__device__ __forceinline__ float quant16(const float* x, bool valid, i32x4q& q) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; j++) amax = fmaxf(amax, fabsf(x[j]));
  amax = max8(valid ? amax : 0.f);
  const float sc = amax > 0.f ? amax / 127.f : 1.f;  // IEEE division (no fast-math in this build)
  q = (i32x4q){0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int c = (int)fminf(fmaxf(rintf(x[j] / sc), -127.f), 127.f);
    q[j >> 2] |= (c & 0xFF) << (8 * (j & 3));
  }
  return sc;
}

// Decode (S == 1) over the int8 cache: attn_decode_kernel's grid, chunk walk, online softmax, partial format and
// three finishes (kernels.hip), with
//   * codes streamed as whole rows, 16 B per lane: 8 rows per load instruction, CH / 8 instructions per chunk;
//   * one fp32 scale per position and lane, K's applied to the finished dot product, V's folded into p;
//   * position past_b (the new token) taken from the bf16 staging row [B][head][hd], never from the cache;
//   * wave 0 of split 0 quantising that staging row into the cache at past_b (read by the NEXT launch).
// The first chunk's codes and scales go out before past_len is known, clamped to the cache: positions past the
// context are masked (score -inf, p = 0) and every scale is finite (zero-initialised or written finite), so they add 0.
template <int WV, int CH>
__global__ __launch_bounds__(WV * 64) void attn_decode_q8_kernel(AttnArgs a, KvQ8 kq) {
  constexpr int NI = CH / 8;
  __shared__ __attribute__((aligned(16))) float qs[128];
  __shared__ float es[WV][64];
  __shared__ float enew[WV];
  __shared__ float pm[WV], pl[WV];
  __shared__ float pacc[WV][128];
  __shared__ int last;
  const int head = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hd = a.head_dim;
  const size_t rowbase = ((size_t)(a.slot + b) * a.n_head + head) * a.max_ctx;
  int8_t* kb = (int8_t*)const_cast<void*>(a.k_cache) + rowbase * hd;
  int8_t* vb = (int8_t*)const_cast<void*>(a.v_cache) + rowbase * hd;
  float* ksb = kq.k_scale + rowbase;
  float* vsb = kq.v_scale + rowbase;
  const int grp = lane >> 3, dl = lane & 7;
  const bool dval = dl * 16 < hd;
  const int doff = dval ? dl * 16 : 0;  // masked lanes re-read dims 0..15 of their own row (never summed)
  i32x4q kr[NI], vr[NI];
  float ksc = 0.f, vsc = 0.f;
  auto load_chunk = [&](int c, int lim) {
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const int pr = min(c * CH + it * 8 + grp, lim);
      kr[it] = *reinterpret_cast<const i32x4q*>(kb + (size_t)pr * hd + doff);
    }
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const int pr = min(c * CH + it * 8 + grp, lim);
      vr[it] = *reinterpret_cast<const i32x4q*>(vb + (size_t)pr * hd + doff);
    }
    const int ps = min(c * CH + (lane & (CH - 1)), lim);
    ksc = ksb[ps];
    vsc = vsb[ps];
  };
  int c = w + WV * sp;
  if (c * CH < a.max_ctx) load_chunk(c, a.max_ctx - 1);
  // the new token's bf16 K / V (this lane's 16 dims), q, the slope and past_len: all in flight with the first chunk
  const size_t srow = ((size_t)b * a.n_head + head) * hd;
  float kn[16], vn[16];
  load16(kq.k_stage + srow + doff, kn);
  load16(kq.v_stage + srow + doff, vn);
  // wave 0 of split 0 (one per (row, head)) also takes that row one or two elements per lane, to quantise it
  const bool quantiser = sp == 0 && w == 0;
  float xq[4] = {0.f, 0.f, 0.f, 0.f};
  if (quantiser) {
    const int d0 = min(lane, hd - 1), d1 = min(lane + 64, hd - 1);
    xq[0] = to_f32(kq.k_stage[srow + d0]); xq[1] = to_f32(kq.k_stage[srow + d1]);
    xq[2] = to_f32(kq.v_stage[srow + d0]); xq[3] = to_f32(kq.v_stage[srow + d1]);
  }
  const float slope = a.slopes[head];
  const float qreg =
      threadIdx.x < hd ? to_f32(((const bf16*)a.q)[(size_t)b * a.hidden + head * hd + threadIdx.x]) : 0.f;
  const int past = a.past_dev ? a.past_dev[b] : a.past;
  const int nk = past + 1, nlast = nk - 1;
  const int nch = (nk + CH - 1) / CH;
  if (threadIdx.x < hd) qs[threadIdx.x] = qreg;  // hd <= 128 <= WV * 64
  __syncthreads();
  // the cache takes the new token (while the wave's first chunk is still on the way): two divisions per lane and
  // vector; nobody reads position past_b from the cache in this launch, the next launch does
  if (quantiser) {
#pragma unroll
    for (int wch = 0; wch < 2; wch++) {
      const float x0 = lane < hd ? xq[2 * wch] : 0.f, x1 = lane + 64 < hd ? xq[2 * wch + 1] : 0.f;
      const float amax = wave_max(fmaxf(fabsf(x0), fabsf(x1)));
      const float sc = amax > 0.f ? amax / 127.f : 1.f;  // IEEE division (no fast-math in this build)
      int8_t* cb = (wch ? vb : kb) + (size_t)nlast * hd;
      if (lane < hd) cb[lane] = (int8_t)(int)fminf(fmaxf(rintf(x0 / sc), -127.f), 127.f);
      if (lane + 64 < hd) cb[lane + 64] = (int8_t)(int)fminf(fmaxf(rintf(x1 / sc), -127.f), 127.f);
      if (lane == 0) (wch ? vsb : ksb)[nlast] = sc;
    }
  }
  float qv[16];
#pragma unroll
  for (int j = 0; j < 16; j += 4) {
    const float4 t = *reinterpret_cast<const float4*>(&qs[doff + j]);
    qv[j] = t.x; qv[j + 1] = t.y; qv[j + 2] = t.z; qv[j + 3] = t.w;
  }
  float m_run = -INFINITY, l_run = 0.f;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; j++) acc[j] = 0.f;
  for (; c < nch; c += WV * nsplit) {
    if (c != w + WV * sp) load_chunk(c, nlast);
    const bool has_new = nlast >= c * CH && nlast < (c + 1) * CH;  // wave-uniform: this chunk holds the new token
    float sc[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++) d += qv[j] * code_f32(kr[it], j);
      sc[it] = sum8(dval ? d : 0.f);
    }
    if (dl == 0) {
#pragma unroll
      for (int it = 0; it < NI; it++) es[w][it * 8 + grp] = sc[it];
    }
    float dnew = 0.f;
    if (has_new) {  // q . k_new at bf16: every 8-lane group holds the same row
#pragma unroll
      for (int j = 0; j < 16; j++) dnew += qv[j] * kn[j];
      dnew = sum8(dval ? dnew : 0.f);
    }
    __builtin_amdgcn_wave_barrier();
    const int p = c * CH + lane;
    const bool live = lane < CH && p < nk;
    const bool is_new = live && p == nlast;
    const float dot = is_new ? dnew : es[w][lane & (CH - 1)] * ksc;
    const float s_me = live ? slope * (float)p + a.inv_norm * dot : -INFINITY;
    const float m_new = fmaxf(m_run, wave_max(s_me));
    const float e = live ? __expf(s_me - m_new) : 0.f;
    const float scale = __expf(m_run - m_new);  // 0 on the first chunk (m_run = -inf)
    l_run = l_run * scale + wave_sum(e);
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] *= scale;
    m_run = m_new;
    __builtin_amdgcn_wave_barrier();
    es[w][lane] = is_new ? 0.f : e * vsc;  // masked: 0 * finite scale
    if (is_new) enew[w] = e;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < NI; it++) {
      const float ep = es[w][it * 8 + grp];
#pragma unroll
      for (int j = 0; j < 16; j++) acc[j] += ep * code_f32(vr[it], j);
    }
    if (has_new) {  // counted once: group 0's lanes
      const float en = grp == 0 ? enew[w] : 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++) acc[j] += en * vn[j];
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int j = 0; j < 16; j++) {  // sum over the wave's 8 row groups (lane bits 3..5)
    acc[j] += dpp_f<0x128>(acc[j]);  // row_ror:8 == xor 8 inside a 16-lane row
    acc[j] += __shfl_xor(acc[j], 16, 64);
    acc[j] += __shfl_xor(acc[j], 32, 64);
  }
  if (grp == 0 && dval) {
#pragma unroll
    for (int j = 0; j < 16; j++) pacc[w][dl * 16 + j] = acc[j];
  }
  if (lane == 0) { pm[w] = m_run; pl[w] = l_run; }
  __syncthreads();
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
  // ---- split partial (sc1 write-through), ticket, last arriver merges (attn_decode_block's protocol)
  if (threadIdx.x < hd)
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), q8_rsrc(pacc_g), (uint32_t)(sp * hd + threadIdx.x) * 4, 0, 16);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(M), q8_rsrc(pml_g), (uint32_t)sp * 8, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(L), q8_rsrc(pml_g), (uint32_t)sp * 8 + 4, 0, 16);
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
        m8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(q8_rsrc(pml_g), (uint32_t)t * 8, 0, 16));
        l8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(q8_rsrc(pml_g), (uint32_t)t * 8 + 4, 0, 16));
        o8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(q8_rsrc(pacc_g), (uint32_t)(t * hd + threadIdx.x) * 4, 0, 16));
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

// Cache positions [0, past_b) of row b -> bf16 staging [B][head][lmax][hd] (the prefill attention's operand).
// Block = 32 positions x 8 lanes of 16 dims; grid (head, b, ceil(max past / 32)).
__global__ __launch_bounds__(256) void kv_dequant_kernel(const int8_t* __restrict__ kc, const int8_t* __restrict__ vc,
                                                         KvQ8 kq, const int* __restrict__ past_dev, int slot,
                                                         int n_head, int hd, int max_ctx, int lmax) {
  const int head = blockIdx.x, b = blockIdx.y;
  const int pos = blockIdx.z * 32 + (threadIdx.x >> 3), dl = threadIdx.x & 7;
  if (pos >= past_dev[b] || dl * 16 >= hd) return;
  const size_t crow = ((size_t)(slot + b) * n_head + head) * max_ctx + pos;
  const size_t srow = ((size_t)b * n_head + head) * lmax + pos;
#pragma unroll
  for (int wch = 0; wch < 2; wch++) {
    const i32x4q q = *reinterpret_cast<const i32x4q*>((wch ? vc : kc) + crow * hd + dl * 16);
    const float sc = (wch ? kq.v_scale : kq.k_scale)[crow];
    bf16* dst = (wch ? kq.v_stage : kq.k_stage) + srow * hd + dl * 16;
    u16x8 o[2];
#pragma unroll
    for (int j = 0; j < 16; j++) o[j >> 3][j & 7] = __builtin_bit_cast(unsigned short, (bf16)(code_f32(q, j) * sc));
    *reinterpret_cast<u16x8*>(dst) = o[0];
    *reinterpret_cast<u16x8*>(dst + 8) = o[1];
  }
}

// Staging positions past_b .. past_b + S - 1 of every (row, head) -> codes and scales at the same cache positions.
// Block = 32 vectors x 8 lanes; grid (head, b, ceil(S / 32)).
__global__ __launch_bounds__(256) void kv_quant_kernel(int8_t* __restrict__ kc, int8_t* __restrict__ vc, KvQ8 kq,
                                                       const int* __restrict__ past_dev, int S, int slot, int n_head,
                                                       int hd, int max_ctx, int lmax) {
  const int head = blockIdx.x, b = blockIdx.y;
  const int t = blockIdx.z * 32 + (threadIdx.x >> 3), dl = threadIdx.x & 7;
  const bool tval = t < S, dval = dl * 16 < hd;
  const int pos = past_dev[b] + (tval ? t : 0);  // idle groups re-read vector 0 (the group reductions need every lane)
  const size_t crow = ((size_t)(slot + b) * n_head + head) * max_ctx + pos;
  const size_t srow = ((size_t)b * n_head + head) * lmax + pos;
  const int doff = dval ? dl * 16 : 0;
#pragma unroll
  for (int wch = 0; wch < 2; wch++) {
    float x[16];
    load16((wch ? kq.v_stage : kq.k_stage) + srow * hd + doff, x);
    i32x4q q;
    const float sc = quant16(x, dval, q);
    if (tval && dval) *reinterpret_cast<i32x4q*>((wch ? vc : kc) + crow * hd + doff) = q;
    if (tval && dl == 0) (wch ? kq.v_scale : kq.k_scale)[crow] = sc;
  }
}

}  // namespace

void launch_attention_q8(const AttnArgs& a, const KvQ8& kq, hipStream_t s) {
  // attn_decode_kernel's grids (launch_attention, S == 1)
  const int nsplit = attention_decode_splits(a.B, a.n_head, a.max_chunks);
  if (nsplit == 1) {
    dim3 g(a.n_head, a.B, 1);
    if (a.B * a.n_head > 256) attn_decode_q8_kernel<4, 64><<<g, 256, 0, s>>>(a, kq);
    else attn_decode_q8_kernel<8, 64><<<g, 512, 0, s>>>(a, kq);
  } else if (a.defer_merge) {
    dim3 g(a.n_head, a.B, nsplit);
    attn_decode_q8_kernel<8, 32><<<g, 512, 0, s>>>(a, kq);
  } else {
    dim3 g(a.n_head, a.B, nsplit);
    attn_decode_q8_kernel<4, 64><<<g, 256, 0, s>>>(a, kq);
  }
}

void launch_kv_dequant(const void* k_codes, const void* v_codes, const KvQ8& kq, const int* past_dev, int B, int slot,
                       int n_head, int head_dim, int max_ctx, int lmax, int past_max, hipStream_t s) {
  if (past_max <= 0) return;
  dim3 g(n_head, B, (past_max + 31) / 32);
  kv_dequant_kernel<<<g, 256, 0, s>>>((const int8_t*)k_codes, (const int8_t*)v_codes, kq, past_dev, slot, n_head,
                                      head_dim, max_ctx, lmax);
}

void launch_kv_quant(void* k_codes, void* v_codes, const KvQ8& kq, const int* past_dev, int B, int S, int slot,
                     int n_head, int head_dim, int max_ctx, int lmax, hipStream_t s) {
  dim3 g(n_head, B, (S + 31) / 32);
  kv_quant_kernel<<<g, 256, 0, s>>>((int8_t*)k_codes, (int8_t*)v_codes, kq, past_dev, S, slot, n_head, head_dim,
                                    max_ctx, lmax);
}
