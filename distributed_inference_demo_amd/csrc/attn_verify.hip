// attn_verify.hip — short-query attention of a verify pass (bs_step.flags & BS_STEP_VERIFY): 2 <= S <= 8 new
// queries per row over a warm KV cache, on a grid that depends on nothing the host knows only per call.
//
// Block (head, row b, split sp) of 4 waves, the decode kernel's shape (kernels.hip attn_decode_block): wave w of split
// sp takes the CH-position chunks c = w + 4 * (sp + nsplit * j).  16 lanes cover one 8-dim slice each of a key/value
// row, so a load instruction reads 4 whole rows; a chunk's K and V rows are loaded ONCE and used by all S queries
// (the cache stream is the cost of a short pass; the S-fold arithmetic rides on it).  Query t of row b sits at
// position past_b + t and attends positions <= past_b + t: the QKV epilogue has already written the pass's own K / V
// rows at past_b .. past_b + S - 1.  past_b comes from past_dev, and no position >= past_b + S is ever read (rows
// past the end of a chunk re-read position past_b + S - 1 with probability 0), so whatever a rolled-back row still
// holds beyond its position cannot reach the result.
// Scores = slope_h * key_pos + q.k / sqrt(hd); one fp32 online softmax per query and wave; the waves' partials meet
// in LDS.  nsplit == 1: the block writes ctx.  Otherwise it publishes its S (max, sum, context) partials
// write-through (sc1), every storing wave drains its stores, and one lane takes a ticket behind the block's barrier;
// the block that draws the last ticket of its (row, head) folds splits 0 .. nsplit - 1 in index order with sc1 loads
// and writes ctx -- the decode kernel's ticket path (MI355X_MICROARCH.md "Valid forms", the counter form whose last
// adder reads).  No floating-point atomics: the result does not depend on which block arrives last.
#include <algorithm>
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ __amdgpu_buffer_rsrc_t verify_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)0xFFFFFFFF, 0x00020000);
}
__device__ __forceinline__ void store_sc1(float v, float* base, uint32_t elem) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), verify_rsrc(base), elem * 4, 0, 16);
}
__device__ __forceinline__ float load_sc1(const float* base, uint32_t elem) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(verify_rsrc(base), elem * 4, 0, 16));
}

constexpr int kVerifyWaves = 4;

// a.part_acc / a.part_ml: the verify partials [B * S][n_head][a.max_chunks (= the split stride)][hd] and [..][2].
template <typename T, int S, int CH>
__global__ __launch_bounds__(kVerifyWaves * 64) void attn_verify_kernel(AttnArgs a) {
  constexpr int WV = kVerifyWaves, NI = CH / 4;
  __shared__ __attribute__((aligned(16))) float qs[S][128];
  __shared__ float es[WV][S][64];
  __shared__ float pm[WV][S], pl[WV][S];
  __shared__ float pacc[WV][S][128];
  __shared__ int last;
  const int head = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hd = a.head_dim;
  const size_t rowbase = ((size_t)(a.slot + b) * a.n_head + head) * a.max_ctx;
  const T* kb = (const T*)a.k_cache + rowbase * hd;
  const T* vb = (const T*)a.v_cache + rowbase * hd;
  const int grp = lane >> 4, dl = lane & 15;
  const bool dval = dl * 8 < hd;
  const int doff = dval ? dl * 8 : 0;  // masked lanes re-read dims 0..7 (their products are dropped)
  const float slope = a.slopes[head];
  const int past = a.past_dev ? a.past_dev[b] : a.past;
  const int nk = min(past + S, a.max_ctx);  // positions the pass's last query attends (the host checked the sum)
  const int nlast = nk - 1;
  const int nch = (nk + CH - 1) / CH;
  for (int i = threadIdx.x; i < S * hd; i += WV * 64) {
    const int t = i / hd, d = i - t * hd;
    qs[t][d] = to_f32(((const T*)a.q)[(size_t)(b * S + t) * a.hidden + head * hd + d]);
  }
  __syncthreads();
  typedef typename Raw8<T>::type R8;
  float m_run[S], l_run[S], acc[S][8];
#pragma unroll
  for (int t = 0; t < S; t++) {
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) acc[t][j] = 0.f;
  }
  for (int c = w + WV * sp; c < nch; c += WV * nsplit) {
    R8 kr[NI], vr[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) raw_load(kb + (size_t)min(c * CH + it * 4 + grp, nlast) * hd + doff, kr[it]);
#pragma unroll
    for (int it = 0; it < NI; it++) raw_load(vb + (size_t)min(c * CH + it * 4 + grp, nlast) * hd + doff, vr[it]);
    // q.k of every query against the chunk's rows: the 16 lanes of a row sum their slices (one DPP row)
#pragma unroll
    for (int t = 0; t < S; t++) {
      const float4 q0 = *reinterpret_cast<const float4*>(&qs[t][doff]);
      const float4 q1 = *reinterpret_cast<const float4*>(&qs[t][doff + 4]);
      const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
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
        if (dl == 0) es[w][t][it * 4 + grp] = d;
      }
    }
    __builtin_amdgcn_wave_barrier();
    const int p = c * CH + lane;
#pragma unroll
    for (int t = 0; t < S; t++) {
      const bool live = lane < CH && p <= past + t && p < nk;  // causal: query t sits at past + t
      const float s_me = live ? slope * (float)p + a.inv_norm * es[w][t][lane] : -INFINITY;
      const float m_new = fmaxf(m_run[t], wave_max(s_me));
      // a chunk that holds nothing for this query yet (its positions all lie behind the query) leaves the state alone
      const float e = live ? __expf(s_me - m_new) : 0.f;
      const float scale = m_new == -INFINITY ? 0.f : __expf(m_run[t] - m_new);
      l_run[t] = l_run[t] * scale + wave_sum(e);
#pragma unroll
      for (int j = 0; j < 8; j++) acc[t][j] *= scale;
      m_run[t] = m_new;
      es[w][t][lane] = e;  // each lane replaces the score it alone read
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < NI; it++) {
#pragma unroll
      for (int t = 0; t < S; t++) {
        const float ep = es[w][t][it * 4 + grp];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[t][j] += ep * raw_get(vr[it], j);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int t = 0; t < S; t++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float v = acc[t][j];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (grp == 0 && dval) pacc[w][t][dl * 8 + j] = v;
    }
    if (lane == 0) { pm[w][t] = m_run[t]; pl[w][t] = l_run[t]; }
  }
  __syncthreads();
  // the block's partial of (query t, dim d): the waves folded in wave order
  const size_t pairq = (size_t)(b * S) * a.n_head + head;  // + t * n_head per query
  for (int i = threadIdx.x; i < S * hd; i += WV * 64) {
    const int t = i / hd, d = i - t * hd;
    float M = pm[0][t];
#pragma unroll
    for (int ww = 1; ww < WV; ww++) M = fmaxf(M, pm[ww][t]);
    float L = 0.f, o = 0.f;
    if (M != -INFINITY) {  // a split past the query's context holds no chunk
#pragma unroll
      for (int ww = 0; ww < WV; ww++) {
        const float wgt = __expf(pm[ww][t] - M);  // idle waves: exp(-inf) = 0
        L += wgt * pl[ww][t];
        o += wgt * pacc[ww][t][d];
      }
    }
    if (nsplit == 1) {
      ((T*)a.ctx_out)[(size_t)(b * S + t) * a.hidden + head * hd + d] = from_f32<T>(o / L);
    } else {
      const size_t pq = (pairq + (size_t)t * a.n_head) * a.max_chunks;
      store_sc1(o, a.part_acc + pq * hd, (uint32_t)(sp * hd + d));
      if (d == 0) {
        store_sc1(M, a.part_ml + pq * 2, (uint32_t)sp * 2);
        store_sc1(L, a.part_ml + pq * 2, (uint32_t)sp * 2 + 1);
      }
    }
  }
  if (nsplit == 1) return;
  // ---- every storing wave drains its write-through stores, then one lane takes the (row, head) ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    typedef __attribute__((address_space(1))) unsigned gu32;
    unsigned* tk = a.tickets + (size_t)(a.slot + b) * a.n_head + head;
    const unsigned old = __hip_atomic_fetch_add((gu32*)tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == (unsigned)(nsplit - 1);
    if (last) __hip_atomic_store((gu32*)tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // zero between launches
  }
  __syncthreads();
  if (!last) return;
  // ---- the last arriver folds splits 0 .. nsplit - 1 in index order (sc1 loads, a group's loads in flight together)
  for (int i = threadIdx.x; i < S * hd; i += WV * 64) {
    const int t = i / hd, d = i - t * hd;
    const size_t pq = (pairq + (size_t)t * a.n_head) * a.max_chunks;
    const float* pacc_g = a.part_acc + pq * hd;
    const float* pml_g = a.part_ml + pq * 2;
    float mx = -INFINITY, acc2 = 0.f, lsum = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float m8[8], l8[8], o8[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int s = min(s0 + u, nsplit - 1);
        m8[u] = load_sc1(pml_g, (uint32_t)s * 2);
        l8[u] = load_sc1(pml_g, (uint32_t)s * 2 + 1);
        o8[u] = load_sc1(pacc_g, (uint32_t)(s * hd + d));
      }
      float gm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; u++) gm = s0 + u < nsplit ? fmaxf(gm, m8[u]) : gm;
      const float nm = fmaxf(mx, gm);
      if (nm != -INFINITY) {
        const float sc = __expf(mx - nm);  // mx = -inf before the first split that holds a chunk: 0
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
    ((T*)a.ctx_out)[(size_t)(b * S + t) * a.hidden + head * hd + d] = from_f32<T>(acc2 / lsum);
  }
}

template <typename T, int CH>
void verify_launch(const AttnArgs& a, int nsplit, hipStream_t s) {
  const dim3 g(a.n_head, a.B, nsplit), blk(kVerifyWaves * 64);
  switch (a.S) {
    case 2: attn_verify_kernel<T, 2, CH><<<g, blk, 0, s>>>(a); break;
    case 3: attn_verify_kernel<T, 3, CH><<<g, blk, 0, s>>>(a); break;
    case 4: attn_verify_kernel<T, 4, CH><<<g, blk, 0, s>>>(a); break;
    case 5: attn_verify_kernel<T, 5, CH><<<g, blk, 0, s>>>(a); break;
    case 6: attn_verify_kernel<T, 6, CH><<<g, blk, 0, s>>>(a); break;
    case 7: attn_verify_kernel<T, 7, CH><<<g, blk, 0, s>>>(a); break;
    default: attn_verify_kernel<T, 8, CH><<<g, blk, 0, s>>>(a); break;
  }
}

}  // namespace

int attention_verify_split_stride(int n_head, int max_chunks) {
  return attention_decode_splits(1, n_head, max_chunks);  // the rule's largest value: it does not grow with B
}

void launch_attention_verify(int is_bf16, const AttnArgs& a, hipStream_t s) {
  // a.max_chunks carries the split stride of the partials; the chunk count of the cache sizes the split rule
  const int chunks = (a.max_ctx + 63) / 64;
  const int nsplit = std::min(attention_decode_splits(a.B, a.n_head, chunks), a.max_chunks);
  if (is_bf16) verify_launch<bf16, 64>(a, nsplit, s);
  else verify_launch<float, 32>(a, nsplit, s);
}
