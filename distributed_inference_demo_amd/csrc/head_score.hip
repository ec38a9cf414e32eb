// head_score.hip — teacher-forced scoring head (include/bloomstage.h bs_forward_score): the tied lm_head fused with
// a log-softmax, so no logit is ever stored.
//
// head_score_kernel is a bf16 GEMM on v_mfma_f32_32x32x16_bf16 of the head W [V][K] (the A operand) against the
// normalised positions xn [M][K] (the B operand): the accumulator then holds one POSITION per lane (column
// lane & 31) and 16 vocabulary rows per 32 x 32 fragment in its registers, so the per-position running statistics
//   best  = the largest logit so far (it is also the softmax's running max),
//   bidx  = the first vocabulary index that reached it,
//   ssum  = sum of exp(logit - best),
//   tl    = the logit of the position's target token (-inf until its tile comes by)
// are plain per-lane loops over registers, in increasing vocabulary order, with no cross-lane traffic per tile.
// Block = 512 threads = 2 (vocabulary) x 4 (position) waves of 64 x 32 on a 128 x 128 tile, BK = 64, staged as
// gemm_mfma3_kernel stages its operands (kernels.hip): LDS-DMA into 3 stages, the XOR swizzle applied on the global
// side, one raw s_barrier per K-step.  A block owns one 128-position row tile and a contiguous run of vocabulary
// tiles and carries its statistics across them; the K-steps of the run form one pipeline (the next tile's first
// stages land while the current tile's statistics are taken).  The two lane halves and the two vocabulary waves of
// a position are combined once, through LDS, when the run ends: partials are [splits][M], 20 bytes each.
// head_score_merge_kernel folds the splits of every position in split order and writes top_ids / scores; it is the
// pass's last kernel and advances the device copy of the rows' cached lengths.
// Every order is fixed (registers, lane halves, waves, splits) and there is no floating-point atomic: results are
// bit-identical from run to run.  expf / logf are the full-precision library functions.
//
// Bounds: the buffer descriptors are re-based per tile (head rows [n0, n0 + rows), positions [m0, m0 + rows)) and
// bounded to it, so a row past V or M reads zeros instead of a neighbour; vocabulary rows past V are masked to -inf
// before the statistics, positions past M are never written.  K % 32 == 0: the last K-step of a K % 64 == 32 operand
// runs its first two 16-deep MFMA steps only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int BV = 128, BP = 128, BK = 64, NSTG = 3, NTH = 512;
constexpr int CA = BV * BK / 8 / NTH, CB = BP * BK / 8 / NTH;  // 16-B chunks per thread per stage
constexpr int STAGE = (BV + BP) * BK;                          // bf16 elements of one LDS stage
static_assert(CA * NTH * 8 == BV * BK && CB * NTH * 8 == BP * BK, "every staged chunk has one lane");

struct ScoreParts {
  u64* key;   // [splits][M] argmax key (order(best) << 32) | ~bidx, 0: nothing seen
  float* m;   // [splits][M] best
  float* s;   // [splits][M] sum of exp(logit - best)
  float* tl;  // [splits][M] target logit or -inf
};

__device__ __forceinline__ u64 score_key(float best, int bidx) {
  // -0 and +0 compare equal as logits: both take +0's key, so the lower index wins between them
  return best > -INFINITY ? (((u64)f32_order_key(best + 0.f) << 32) | (0xFFFFFFFFu - (uint32_t)bidx)) : 0ull;
}

// Fold (m2, s2) into (m, s): sums of exponentials relative to their own maxima.
__device__ __forceinline__ void lse_fold(float& m, float& s, float m2, float s2) {
  if (!(m2 > -INFINITY)) return;
  if (m2 > m) {
    s = s * expf(m - m2) + s2;  // m == -inf: s is 0 and expf(-inf) is 0
    m = m2;
  } else {
    s += s2 * expf(m2 - m);
  }
}

__global__ __launch_bounds__(NTH) void head_score_kernel(const bf16* __restrict__ W, const bf16* __restrict__ X,
                                                         const int* __restrict__ targets, int M, int V, int K,
                                                         int splits, int tiles_m, ScoreParts part) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) bf16 smem[NSTG * STAGE];  // 96 KB, the only LDS object
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 2, wn = w & 3, r = lane & 31, h = lane >> 5;  // wave tile: 64 vocabulary rows x 32 positions
  // blocks are dispatched round-robin over the 8 XCDs: with splits % 8 == 0 the blocks that share a vocabulary run
  // (the row tiles of one split) are consecutive virtual blocks of one XCD, so the head leaves HBM once
  const int G = gridDim.x;
  const int vb = splits % 8 ? (int)blockIdx.x : (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8);
  const int sp = vb / tiles_m, tm = vb - sp * tiles_m;
  const int tiles_v = (V + BV - 1) / BV;
  const int t0 = (int)((long)sp * tiles_v / splits), t1 = (int)((long)(sp + 1) * tiles_v / splits);
  const int m0 = tm * BP, nk = (K + BK - 1) / BK;
  const bool ktail = (K % BK) != 0;

  // this lane's position and its target
  const int pos = m0 + wn * 32 + r;
  int tgt = (targets && pos < M) ? targets[pos] : -1;
  asm volatile("" : "+v"(tgt));  // the load has retired before the DMA pipeline starts counting vmcnt
  float best = -INFINITY, ssum = 0.f, tl = -INFINITY;
  int bidx = 0;

  if (t1 > t0) {
    auto sw = [](int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 3); };
    auto As = [&](int buf) { return smem + buf * STAGE; };
    auto Bs = [&](int buf) { return smem + buf * STAGE + BV * BK; };
    // an LDS-DMA instruction writes 64 consecutive 16-B slots, so the lane filling slot s of row `row` fetches
    // logical chunk s ^ f(row); byte offsets inside the tile (127 rows of K <= 16384 bf16 fit 32 bits easily)
    uint32_t oa[CA], ob[CB];
#pragma unroll
    for (int i = 0; i < CA; i++) {
      const int c = i * NTH + w * 64 + lane, row = c >> 3, ch = (c & 7) ^ ((row >> 1) & 7);
      oa[i] = (uint32_t)(((size_t)row * K + ch * 8) * 2);
    }
#pragma unroll
    for (int i = 0; i < CB; i++) {
      const int c = i * NTH + w * 64 + lane, row = c >> 3, ch = (c & 7) ^ ((row >> 1) & 7);
      ob[i] = (uint32_t)(((size_t)row * K + ch * 8) * 2);
    }
    auto rsrc_rows = [&](const bf16* base, int row0, int nrows) {
      const int rows = min(BV, nrows - row0);
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(base + (size_t)row0 * K), (short)0,
                                               (int)(uint32_t)((size_t)rows * K * 2), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rb = rsrc_rows(X, m0, M);
    __amdgpu_buffer_rsrc_t ra = rsrc_rows(W, t0 * BV, V);
    typedef __attribute__((address_space(3))) void lds_void;
    int lt = t0, lk = 0;  // the load cursor: (vocabulary tile, K-step); past the run's end it re-loads the last step
    auto gload = [&](int buf) {
      const int off = lk * BK * 2;
#pragma unroll
      for (int i = 0; i < CA; i++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(As(buf) + (i * NTH + w * 64) * 8), 16, oa[i], off, 0, 0);
#pragma unroll
      for (int i = 0; i < CB; i++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(Bs(buf) + (i * NTH + w * 64) * 8), 16, ob[i], off, 0, 0);
      if (lk + 1 < nk) {
        lk++;
      } else if (lt + 1 < t1) {
        lt++;
        lk = 0;
        ra = rsrc_rows(W, lt * BV, V);
      }
    };
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][e] = 0.f;
    auto ktile = [&](int buf, bool tail) {
#pragma unroll
      for (int ks = 0; ks < BK / 16; ks++) {
        if (tail && ks >= 2) break;  // K % 64 == 32: the step's upper half lies past the rows
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(As(buf) + sw(wm * 64 + r, ks * 2 + h));
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(As(buf) + sw(wm * 64 + 32 + r, ks * 2 + h));
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Bs(buf) + sw(wn * 32 + r, ks * 2 + h));
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1], 0, 0, 0);
      }
    };
    // one vocabulary tile's 32 logits of this lane's position, in increasing vocabulary order
    auto stats = [&](int t) {
      const int nb = t * BV + wm * 64 + 4 * h;  // accumulator register e of fragment i: row nb + 32 i + (e & 3) + 8 (e >> 2)
      const bool edge = t * BV + BV > V;
      const float old = best;
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int idx = nb + i * 32 + (e & 3) + 8 * (e >> 2);
          float v = acc[i][e];
          if (edge && idx >= V) v = -INFINITY;
          acc[i][e] = v;
          if (v > best) { best = v; bidx = idx; }  // strict: the first index keeps a tie
          tl = idx == tgt ? v : tl;
        }
      if (best > -INFINITY) {  // else every row of this lane so far lay past V
        float add = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int e = 0; e < 16; e++) add += expf(acc[i][e] - best);
        ssum = ssum * expf(old - best) + add;  // old == -inf: ssum is 0 and expf(-inf) is 0
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[i][e] = 0.f;
    };
    // Step g: this wave's DMA of step g retired (vmcnt(CA + CB) leaves step g + 1's in flight) -> barrier (every
    // wave's part of step g has landed, every wave is done reading step g - 1) -> DMA of step g + 2 into step g - 1's
    // stage -> MFMAs of step g.  Raw s_barrier: __syncthreads() would drain the DMA in flight.
    const int total = (t1 - t0) * nk;
    gload(0);
    gload(1);
    int buf = 0, nbuf = NSTG - 1, ck = 0, ct = t0;
    for (int g = 0; g < total; g++) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTG - 2) * (CA + CB)) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      gload(nbuf);
      const bool last = ck == nk - 1;
      ktile(buf, ktail && last);
      if (last) {
        stats(ct);
        ct++;
        ck = 0;
      } else {
        ck++;
      }
      buf = buf == NSTG - 1 ? 0 : buf + 1;
      nbuf = nbuf == NSTG - 1 ? 0 : nbuf + 1;
    }
    // the re-loads past the end land before the LDS is reused
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // combine the four holders of a position (vocabulary wave wm, lane half h) in that order
  float* cm = reinterpret_cast<float*>(smem);  // [4][BP]
  float* cs = cm + 4 * BP;
  float* ctl = cs + 4 * BP;
  u64* ckey = reinterpret_cast<u64*>(ctl + 4 * BP);
  {
    const int c = wm * 2 + h, p = wn * 32 + r;
    cm[c * BP + p] = best;
    cs[c * BP + p] = ssum;
    ctl[c * BP + p] = tl;
    ckey[c * BP + p] = score_key(best, bidx);
  }
  __syncthreads();
  if (tid < BP && m0 + tid < M) {
    float m = -INFINITY, s = 0.f, t = -INFINITY;
    u64 key = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      lse_fold(m, s, cm[c * BP + tid], cs[c * BP + tid]);
      t = fmaxf(t, ctl[c * BP + tid]);
      const u64 k2 = ckey[c * BP + tid];
      key = k2 > key ? k2 : key;
    }
    const size_t o = (size_t)sp * M + m0 + tid;
    part.key[o] = key;
    part.m[o] = m;
    part.s[o] = s;
    part.tl[o] = t;
  }
#endif
}

__global__ __launch_bounds__(256) void head_score_merge_kernel(ScoreParts part, int splits, int M, int V,
                                                               const int* __restrict__ targets,
                                                               int* __restrict__ top_ids, float* __restrict__ scores,
                                                               int* past_adv, int B, int seq) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos < M) {
    float m = -INFINITY, s = 0.f, t = -INFINITY;
    u64 key = 0;
    for (int sp = 0; sp < splits; sp++) {
      const size_t o = (size_t)sp * M + pos;
      lse_fold(m, s, part.m[o], part.s[o]);
      t = fmaxf(t, part.tl[o]);
      const u64 k2 = part.key[o];
      key = k2 > key ? k2 : key;
    }
    const float lse = m + logf(s);
    if (top_ids) top_ids[pos] = (int)(0xFFFFFFFFu - (uint32_t)key);
    if (scores) {
      const bool has = targets && (unsigned)targets[pos] < (unsigned)V;
      scores[3 * pos + 0] = has ? t - lse : 0.0f;
      scores[3 * pos + 1] = m - lse;  // the largest logit is the running max
      scores[3 * pos + 2] = lse;
    }
  }
  if (past_adv && blockIdx.x == 0)
    for (int b = threadIdx.x; b < B; b += 256) past_adv[b] += seq;
}

}  // namespace

// Vocabulary splits of a scoring launch over M positions: one block per (split, 128-position row tile), about one
// block per CU, never more splits than 128-row vocabulary tiles; a multiple of 8 (one run per XCD) when it can be.
int head_score_splits(int M, int V, int cus) {
  const int tiles_m = (M + BP - 1) / BP, tiles_v = (V + BV - 1) / BV;
  int sp = std::max(1, std::min(tiles_v, std::max(1, cus) / std::max(1, tiles_m)));
  if (sp >= 8) sp -= sp % 8;
  return sp;
}

size_t head_score_partial_bytes(int M, int V, int cus) { return (size_t)head_score_splits(M, V, cus) * M * 20; }

void launch_head_score(const void* xn, const void* W, const int* targets, int M, int V, int K, int cus, void* parts,
                       int* top_ids, float* scores, int* past_adv, int B, int seq, hipStream_t s) {
  const int splits = head_score_splits(M, V, cus), tiles_m = (M + BP - 1) / BP;
  const size_t n = (size_t)splits * M;
  ScoreParts p;
  p.key = (u64*)parts;
  p.m = (float*)((char*)parts + n * 8);
  p.s = p.m + n;
  p.tl = p.s + n;
  head_score_kernel<<<splits * tiles_m, NTH, 0, s>>>((const bf16*)W, (const bf16*)xn, targets, M, V, K, splits,
                                                     tiles_m, p);
  head_score_merge_kernel<<<(M + 255) / 256, 256, 0, s>>>(p, splits, M, V, targets, top_ids, scores, past_adv, B, seq);
}
