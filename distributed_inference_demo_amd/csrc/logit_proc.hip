// logit_proc.hip — per-row logit processors (include/bloomstage.h "Per-row logit processors").
//
// Bias, repetition penalty, no-repeat n-gram, banned tokens and the minimum-new-tokens EOS ban, applied to a row's fp32
// logits between the head and the pick.  The rule depends on every token the row has seen, so the history lives on the
// device, per KV row:
//   hist      int32 [cap]    the tokens in order (cap = max_ctx + 1)
//   seen      uint32 [words] one bit per vocabulary entry (words = ceil(V / 32))
//   distinct  int32 [cap]    each seen token once; the order is whatever the atomics made it, and nothing reads it
//                            as an order: the penalty touches each entry exactly once
//   counts    int32 [4]      history length, distinct tokens, generated tokens
// Three kernels, one block per row, no block ever waits for another:
//   set    writes the table entry and empties the row: zeroes the seen WORD of every distinct token (a word holds only
//          bits of distinct tokens, so whole words may go), then the counts -- O(tokens noted), never O(V)
//   note   appends tokens in call order (a block-wide prefix count drops ids outside [0, V)); atomicOr on the seen
//          word, and the thread that newly set the bit takes the next distinct slot with an integer atomicAdd
//   apply  five phases in the rule's order, a block barrier between two phases because one token can be in several
//          lists; within a phase each logit has one writer, or every writer stores the same value
// Work is O(history length + bias entries); no launch reads or writes V logits.  Integer atomics only, no
// floating-point atomics, so given the logits and the history the result is the same bits in every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kNoteArgIds = 512;  // host ids travel by kernel arguments, this many a launch
constexpr int kSetArgRows = 4;    // table rows a set launch carries by kernel arguments

struct LpRows { RowProcDev v[kSetArgRows]; };
struct LpIds { int v[kNoteArgIds]; };

__global__ void __launch_bounds__(kThreads) logit_proc_set_kernel(LogitProcBufs lp, int slot, LpRows rows) {
  const int row = slot + blockIdx.x, tid = threadIdx.x;
  int* cnt = lp.counts + (size_t)row * 4;
  const int nd = min(cnt[1], lp.cap);
  const int* dl = lp.distinct + (size_t)row * lp.cap;
  uint32_t* seen = lp.seen + (size_t)row * lp.words;
  for (int i = tid; i < nd; i += kThreads) seen[dl[i] >> 5] = 0u;  // in range: only the note kernel writes the list
  const int* src = reinterpret_cast<const int*>(&rows.v[blockIdx.x]);
  int* dst = reinterpret_cast<int*>(lp.table + row);
  for (int i = tid; i < (int)(sizeof(RowProcDev) / 4); i += kThreads) dst[i] = src[i];
  __syncthreads();  // every thread has read the old distinct count
  if (tid < 4) cnt[tid] = 0;
}

// Append ids[0..n) to `row`: called by every thread of the block.  Tokens outside [0, V) are dropped, as is whatever
// does not fit below cap.  wsum: LDS [kThreads / 64 + 1].
__device__ void lp_append(const LogitProcBufs& lp, int row, const int* ids, int n, int generated, int* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* cnt = lp.counts + (size_t)row * 4;
  int* hist = lp.hist + (size_t)row * lp.cap;
  int* dl = lp.distinct + (size_t)row * lp.cap;
  uint32_t* seen = lp.seen + (size_t)row * lp.words;
  int len = cnt[0];
  const int len0 = len;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    const int v = i < n ? ids[i] : -1;
    const bool ok = v >= 0 && v < lp.V;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kThreads / 64; w++) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    const int at = len + before + __popcll(m & ((1ull << lane) - 1ull));
    if (ok && at < lp.cap) {
      hist[at] = v;
      const uint32_t bit = 1u << (v & 31);
      if (!(atomicOr(seen + (v >> 5), bit) & bit)) {
        const int k = atomicAdd(cnt + 1, 1);  // at most one winner per distinct token: k < cap
        if (k < lp.cap) dl[k] = v;
      }
    }
    len = min(len + total, lp.cap);
    __syncthreads();  // wsum is reused by the next chunk
  }
  if (tid == 0) {
    cnt[0] = len;
    if (generated) cnt[2] += len - len0;
  }
}

__global__ void __launch_bounds__(kThreads) logit_proc_note_args_kernel(LogitProcBufs lp, int row, LpIds ids, int n,
                                                                         int generated) {
  __shared__ int wsum[kThreads / 64 + 1];
  __shared__ int sid[kNoteArgIds];
  for (int i = threadIdx.x; i < kNoteArgIds; i += kThreads) sid[i] = ids.v[i];
  __syncthreads();
  if (!lp.table[row].active) return;
  lp_append(lp, row, sid, min(n, kNoteArgIds), generated, wsum);
}

// stride 0, grid 1: n device ids into one row.  stride 1, n 1: the tail's note, block b appends tokens[b] to row
// slot + b.  A row without state returns at once.
__global__ void __launch_bounds__(kThreads) logit_proc_note_dev_kernel(LogitProcBufs lp, int slot, const int* ids,
                                                                        int stride, int n, int generated) {
  __shared__ int wsum[kThreads / 64 + 1];
  const int row = slot + blockIdx.x;
  if (!lp.table[row].active) return;
  lp_append(lp, row, ids + (size_t)blockIdx.x * stride, n, generated, wsum);
}

__global__ void __launch_bounds__(kThreads) logit_proc_apply_kernel(LogitProcBufs lp, float* logits, int ld, int slot) {
  __shared__ RowProcDev p;
  __shared__ int tail[32];  // the last n - 1 tokens of the history
  const int row = slot + blockIdx.x, tid = threadIdx.x;
  if (!lp.table[row].active) return;  // uniform over the block
  {
    const int* src = reinterpret_cast<const int*>(lp.table + row);
    int* dst = reinterpret_cast<int*>(&p);
    for (int i = tid; i < (int)(sizeof(RowProcDev) / 4); i += kThreads) dst[i] = src[i];
  }
  const int* cnt = lp.counts + (size_t)row * 4;
  const int L = min(cnt[0], lp.cap), nd = min(cnt[1], lp.cap), ngen = cnt[2];
  const int* hist = lp.hist + (size_t)row * lp.cap;
  const int* dl = lp.distinct + (size_t)row * lp.cap;
  float* l = logits + (size_t)blockIdx.x * ld;
  __syncthreads();
  const int V = lp.V;
  const int nb = min(max(p.n_bias, 0), kRowBiasMax), n = p.ngram;
  // 1. bias: the first entry of a token adds every finite value of that token, in entry order (one writer a logit)
  if (tid < nb) {
    const int v = p.bias_ids[tid];
    bool first = v >= 0 && v < V;
    for (int j = 0; j < tid && first; j++) first = p.bias_ids[j] != v;
    if (first) {
      float x = l[v];
      bool any = false;
      for (int j = tid; j < nb; j++)
        if (p.bias_ids[j] == v && isfinite(p.bias_values[j])) { x = __fadd_rn(x, p.bias_values[j]); any = true; }
      if (any) l[v] = x;
    }
  }
  __syncthreads();
  // 2. repetition penalty: once per distinct token (x * 1 and x / 1 are x: r == 1 is skipped)
  if (p.penalty != 1.0f) {
    for (int i = tid; i < nd; i += kThreads) {
      const int v = dl[i];
      if (v < 0 || v >= V) continue;
      const float x = l[v];
      l[v] = x < 0.f ? __fmul_rn(x, p.penalty) : __fdiv_rn(x, p.penalty);
    }
  }
  __syncthreads();
  // 3. no-repeat n-gram: every position whose n - 1 tokens equal the history's last n - 1 bans its successor
  if (n >= 1 && n <= 32 && L + 1 >= n) {
    if (tid < n - 1) tail[tid] = hist[L - (n - 1) + tid];
    __syncthreads();
    for (int i = tid; i + n - 1 < L; i += kThreads) {
      bool eq = true;
      for (int j = 0; j < n - 1 && eq; j++) eq = hist[i + j] == tail[j];
      if (eq) {
        const int v = hist[i + n - 1];
        if (v >= 0 && v < V) l[v] = -FLT_MAX;
      }
    }
  }
  __syncthreads();
  // 4. banned tokens: an entry of -inf
  if (tid < nb) {
    const int v = p.bias_ids[tid];
    if (v >= 0 && v < V && p.bias_values[tid] == -INFINITY) l[v] = -FLT_MAX;
  }
  __syncthreads();
  // 5. minimum new tokens
  if (tid == 0 && p.eos >= 0 && p.eos < V && ngen < p.min_new) l[p.eos] = -FLT_MAX;
}

}  // namespace

void launch_logit_proc_set(const LogitProcBufs& lp, int slot, const RowProcDev* rows, int n, hipStream_t s) {
  for (int i = 0; i < n; i += kSetArgRows) {
    LpRows r{};
    const int c = std::min(kSetArgRows, n - i);
    for (int j = 0; j < c; j++) r.v[j] = rows[i + j];
    logit_proc_set_kernel<<<c, kThreads, 0, s>>>(lp, slot + i, r);
  }
}

void launch_logit_proc_note(const LogitProcBufs& lp, int slot, const int* ids_host, const int* ids_dev, int n,
                            int generated, hipStream_t s) {
  if (n <= 0) return;
  if (!ids_host) {
    logit_proc_note_dev_kernel<<<1, kThreads, 0, s>>>(lp, slot, ids_dev, 0, n, generated);
    return;
  }
  for (int i = 0; i < n; i += kNoteArgIds) {
    LpIds a;
    const int c = std::min(kNoteArgIds, n - i);
    for (int j = 0; j < kNoteArgIds; j++) a.v[j] = j < c ? ids_host[i + j] : -1;
    logit_proc_note_args_kernel<<<1, kThreads, 0, s>>>(lp, slot, a, c, generated);
  }
}

void launch_logit_proc_note_picks(const LogitProcBufs& lp, int slot, int B, const int* tokens, hipStream_t s) {
  if (B <= 0) return;
  logit_proc_note_dev_kernel<<<B, kThreads, 0, s>>>(lp, slot, tokens, 1, 1, 1);
}

void launch_logit_proc_apply(const LogitProcBufs& lp, float* logits, int ld, int slot, int B, hipStream_t s) {
  if (B <= 0) return;
  logit_proc_apply_kernel<<<B, kThreads, 0, s>>>(lp, logits, ld, slot);
}
