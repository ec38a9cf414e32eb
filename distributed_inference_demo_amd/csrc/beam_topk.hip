// beam_topk.hip — the top-k log-prob tail (bs_forward_topk): from the fp32 logits [B][ld] the
// full head wrote, the k <= 16 best tokens of each row with their log-probabilities and the row's log-sum-exp.
//
// Two launches on grids that are a function of (B, V) only, nothing a block waits for, no atomics:
//   (a) topk_slice_kernel, grid (slices, B), 256 threads: a block owns kTopkSlice = 2048 consecutive logits of one
//       row (the last slice of a row is short), 8 per lane as two 16-byte loads.  It writes one partial record per
//       (row, slice): the slice max m_s, sum_s = sum expf(l - m_s) and the slice's k best as the argmax keys
//       (order(l + 0.0f) << 32) | ~index -- larger logit first, the lower index first on equal logits, -0.0 == +0.0.
//       The k best come from k rounds of "largest key below the previous one" (keys are unique: they hold the index).
//   (b) topk_fold_kernel, one block of 256 threads per row: M = max m_s, S = sum_s sum_s * expf(m_s - M),
//       lse = M + logf(S); the k best of the slices' candidates by the same rounds; logprob = l - lse (l back from the
//       key, exact).  Thread 0 then advances past_adv[row] by seq: the pass's last kernel, like argmax_finalize_kernel.
//
// Order of the fp32 sums, fixed by the code and the same for every row, batch and launch mode: a lane adds its 8
// terms in index order (7 additions), wave_sum's butterfly adds 6 levels, the four waves add as (w0 + w1) + (w2 + w3)
// (2); in (b) thread t adds the terms of slices t, t + 256, ... in that order (at most 3 additions: kTopkMaxSlices =
// 1024) and a shared-memory tree over the 256 threads adds 8 levels.
//   D = 7 + 6 + 2 + 3 + 8 = 26: the longest chain of fp32 additions a term of the sum passes through.
// Maxima are exact in any order.  expf / logf are the accurate library functions, not the fast intrinsics.
// Lanes beyond the row's end hold -inf (expf(-inf) = +0, an exact addend) and key 0 (below every real key).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkPer = 8;  // logits per lane

typedef unsigned long long u64;

__device__ __forceinline__ u64 topk_key(float l, uint32_t index) {
  return ((u64)f32_order_key(l + 0.0f) << 32) | (u64)(0xFFFFFFFFu - index);
}
__device__ __forceinline__ float topk_key_logit(u64 key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// The block's largest value of v; sh: 4 entries.  Every thread returns it.
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* sh) {
  v = wave_max_u64(v);
  __syncthreads();  // sh may still be read from the previous round
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const u64 a = sh[0] > sh[1] ? sh[0] : sh[1], b = sh[2] > sh[3] ? sh[2] : sh[3];
  return a > b ? a : b;
}

__global__ __launch_bounds__(kTopkThreads) void topk_slice_kernel(const float* __restrict__ logits, int ld, int V, int k,
                                                                  int nslices, float* __restrict__ pmax,
                                                                  float* __restrict__ psum, u64* __restrict__ pkeys) {
  __shared__ u64 sh[4];
  __shared__ float shf[4];
  const int slice = blockIdx.x, row = blockIdx.y;
  const float* lr = logits + (size_t)row * ld;
  const int i0 = slice * kTopkSlice + (int)threadIdx.x * 4;  // this lane's two float4: i0 and i0 + 1024
  float l[kTopkPer];
  u64 key[kTopkPer];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int i = i0 + u * (kTopkThreads * 4);
    if (i < V) {  // V % 4 == 0: a float4 is inside the row or beyond it
      const float4 v = *reinterpret_cast<const float4*>(lr + i);
      l[4 * u] = v.x; l[4 * u + 1] = v.y; l[4 * u + 2] = v.z; l[4 * u + 3] = v.w;
#pragma unroll
      for (int j = 0; j < 4; j++) key[4 * u + j] = topk_key(l[4 * u + j], (uint32_t)(i + j));
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) { l[4 * u + j] = -INFINITY; key[4 * u + j] = 0ull; }
    }
  }
  // slice max (exact), then the sum in the header's order
  float m = l[0];
#pragma unroll
  for (int j = 1; j < kTopkPer; j++) m = fmaxf(m, l[j]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
  __syncthreads();
  float sum = expf(l[0] - m);
#pragma unroll
  for (int j = 1; j < kTopkPer; j++) sum += expf(l[j] - m);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = sum;
  __syncthreads();
  const size_t rec = (size_t)row * nslices + slice;
  if (threadIdx.x == 0) {
    pmax[rec] = m;
    psum[rec] = (shf[0] + shf[1]) + (shf[2] + shf[3]);
  }
  // the slice's k best, best first
  u64 prev = ~0ull;
  for (int r = 0; r < k; r++) {
    u64 best = 0ull;
#pragma unroll
    for (int j = 0; j < kTopkPer; j++) best = (key[j] < prev && key[j] > best) ? key[j] : best;
    prev = block_max_u64(best, sh);
    if (threadIdx.x == 0) pkeys[rec * kTopkMaxK + r] = prev;
  }
}

__global__ __launch_bounds__(kTopkThreads) void topk_fold_kernel(const float* __restrict__ pmax,
                                                                 const float* __restrict__ psum,
                                                                 const u64* __restrict__ pkeys, int nslices, int k,
                                                                 int* __restrict__ ids, float* __restrict__ logprobs,
                                                                 float* __restrict__ lse_out, int* past_adv, int seq) {
  __shared__ u64 sh[4];
  __shared__ float shf[kTopkThreads];
  __shared__ u64 win[kTopkMaxK];
  const int row = blockIdx.x, t = threadIdx.x;
  const float* pm = pmax + (size_t)row * nslices;
  const float* ps = psum + (size_t)row * nslices;
  float m = -INFINITY;
  for (int s = t; s < nslices; s += kTopkThreads) m = fmaxf(m, pm[s]);
  m = wave_max(m);
  if ((t & 63) == 0) shf[t >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
  __syncthreads();
  float sum = 0.f;  // 0 + x is exact: the thread's first term starts its chain
  for (int s = t; s < nslices; s += kTopkThreads) sum += ps[s] * expf(pm[s] - m);
  shf[t] = sum;
  __syncthreads();
#pragma unroll
  for (int o = kTopkThreads / 2; o >= 1; o >>= 1) {
    if (t < o) shf[t] += shf[t + o];
    __syncthreads();
  }
  const float lse = m + logf(shf[0]);
  // the k best of the slices' candidates (k per slice), best first
  const u64* pk = pkeys + (size_t)row * nslices * kTopkMaxK;
  const int ncand = nslices * k;
  u64 prev = ~0ull;
  for (int r = 0; r < k; r++) {
    u64 best = 0ull;
    for (int c = t; c < ncand; c += kTopkThreads) {
      const u64 key = pk[(size_t)(c / k) * kTopkMaxK + (c % k)];
      best = (key < prev && key > best) ? key : best;
    }
    prev = block_max_u64(best, sh);
    if (t == 0) win[r] = prev;
  }
  __syncthreads();
  if (t < k) {
    const u64 key = win[t];
    ids[(size_t)row * k + t] = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
    logprobs[(size_t)row * k + t] = topk_key_logit(key) - lse;
  }
  if (t == 0) {
    if (lse_out) lse_out[row] = lse;
    if (past_adv) past_adv[row] += seq;
  }
}

}  // namespace

int topk_slices(int V) { return (V + kTopkSlice - 1) / kTopkSlice; }

void launch_topk_logprobs(const float* logits, int ld, int V, int B, int k, float* pmax, float* psum,
                          unsigned long long* pkeys, int* ids, float* logprobs, float* lse, int* past_adv, int seq,
                          hipStream_t s) {
  const int ns = topk_slices(V);
  topk_slice_kernel<<<dim3(ns, B), kTopkThreads, 0, s>>>(logits, ld, V, k, ns, pmax, psum, pkeys);
  topk_fold_kernel<<<B, kTopkThreads, 0, s>>>(pmax, psum, pkeys, ns, k, ids, logprobs, lse, past_adv, seq);
}
