// kernels.h — host-side launch wrappers for the stage kernels (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Epilogue of every weight GEMM/GEMV: y[m][n] = sum_k X[m][k] * W[n][k] (+ what `kind` says).
enum EpiKind : int {
  EPI_QKV = 0,     // + bias; q -> q_out (T) [M][h]; k,v -> KV cache (T) at (slot+b, past+t)
  EPI_RESID = 1,   // out_f32[m][n] = (y + bias) + resid[m][n]
  EPI_GELU = 2,    // out_act[m][n] = T(gelu(y + bias))
  EPI_ARGMAX = 3,  // no bias; 64-bit atomicMax of (order(y), ~n) into keys[m]; optional logits
};

struct Epi {
  int kind;
  const void* bias;       // T [N]
  float* out_f32;         // EPI_RESID output [M][ldo]
  void* out_act;          // EPI_GELU output (T) [M][ldo]
  const float* resid;     // EPI_RESID residual [M][ldo]
  int ldo;                // leading dim of out/resid (= N)
  // EPI_QKV
  void* q_out;            // T [M][hidden]
  void* k_cache;          // T, layer base of K: [max_batch][heads][max_ctx][hd]
  void* v_cache;
  int hidden, head_dim, max_ctx, n_head;
  int seq, slot;
  const int* past_dev;    // device past_len per row b = m / seq (graph-replayable); used when non-null
  int past;               // host past_len of every row otherwise
  // EPI_ARGMAX
  unsigned long long* keys;  // [M][N/16]: max over each 16-column tile
  float* logits;          // optional [M][ldo]
  int col_offset;         // vocabulary index of column 0 (head slices)
  int key_hi_index;       // 0: keys rank equal logits by the LOWER index (greedy, torch.argmax);
                          // 1: by the HIGHER index (top-k sampling, decoding.cpp:44-45 std::greater)
  // split-K workspace of the batched GEMV (gemv_tiles): fp32 partials [ks][M][N] (capacity in
  // floats) and one arrival ticket per 16-column tile (zero between launches).  Null: no split-K.
  float* sk_ws;
  unsigned* sk_tickets;
  size_t sk_cap;
  int sk_ntickets;
  // int8 weights: y[m][n] *= col_scale[n] before the epilogue (the weight operand held Q, not
  // Q * scale).  Null otherwise.  Not applied by EPI_ARGMAX.
  const float* col_scale;
};

// dtype tag: 0 = fp32, 1 = bf16
void launch_gen_fill(void* dst, int is_bf16, uint64_t n, uint64_t key, int kind, hipStream_t s,
                     uint64_t index_offset = 0);
void launch_convert_f32(void* dst, int is_bf16, const float* src, uint64_t n, hipStream_t s);

// LayerNorm rows: out[m] (T, or fp32 when out_f32) = LN(x[m*row_stride + row_offset]) with
// gamma/beta (T); x is fp32 [.][K].  If ids != null, row m is instead gathered from the
// embedding table `x` (T) [vocab][K] at ids[m] (word_embeddings + word_embeddings_layernorm).
void launch_layernorm(int is_bf16, const void* x, const int* ids, int row_stride, int row_offset,
                      const void* gamma, const void* beta, void* out, int out_f32, int M, int K,
                      float eps, hipStream_t s);

// Weight GEMM: X (T) [M][K] x W (T) [N][K]^T with epilogue.
void launch_linear(int is_bf16, const void* X, const void* W, int M, int N, int K, const Epi& ep,
                   hipStream_t s);

// LayerNorm(x rows) followed by a weight GEMM; fused into one kernel on the bf16 decode path.
void launch_linear_ln(int is_bf16, const float* x, int row_stride, int row_offset, const void* gamma,
                      const void* beta, float eps, void* xn_scratch, const void* W, int M, int N, int K,
                      const Epi& ep, hipStream_t s);

// The first stage's layer 0 at M <= 2 (bf16): word_embeddings[ids] -> word_embeddings_layernorm (fp32,
// stored to x_out: the residual stream) -> LN_in -> weight GEMV, one kernel.  False: not launched.
bool launch_linear_emb(const int* ids, const void* wemb, const void* emb_g, const void* emb_b, float* x_out,
                       const void* gamma, const void* beta, float eps, const void* W, int M, int N, int K,
                       const Epi& ep, hipStream_t s);

// Attention over the KV cache for B rows x S new queries per row (causal, ALiBi).
struct AttnArgs {
  const void* q;       // T [B*S][hidden]
  const void* k_cache; // T layer base
  const void* v_cache;
  void* ctx_out;       // T [B*S][hidden]
  const float* slopes; // [n_head]
  int B, S, slot;
  const int* past_dev; // device past_len per row [B] (graph-replayable) or null
  int past;
  int n_head, head_dim, max_ctx, hidden;
  float inv_norm;
  float* part_acc;     // workspace [max_batch][n_head][max_chunks][head_dim] (row = slot + b)
  float* part_ml;      // workspace [max_batch][n_head][max_chunks][2]
  int max_chunks;
  int chunk;           // positions per chunk (decode) = 64
  unsigned* tickets;   // [max_batch][n_head] split-merge tickets (zero between launches)
  int defer_merge;     // decode split > 1: leave the partials for the consumer (launch_linear_parts)
  // prefill (S > 1) split-KV: key tiles of a 64-query tile spread over blocks of `pf_tiles` 64-key
  // tiles each (0: no split); partials [item][split][64 queries][4 + head_dim] in pf_ws (pf_cap floats), one
  // ticket per (row, head, query tile) in pf_tickets (zero between launches, pf_ntickets of them)
  int pf_tiles;
  float* pf_ws;
  size_t pf_cap;
  unsigned* pf_tickets;
  int pf_ntickets;
  int pf_past_max;     // largest past_len of the call's rows (sizes the split grid)
};
void launch_attention(int is_bf16, const AttnArgs& a, hipStream_t s);
// S > 1, bf16, head_dim <= 128 (attn_prefill.hip): NSTG LDS stages (2 or 3), split-KV over blocks of pf_tiles key tiles
// (-1: a.pf_tiles) when the grid has fewer than max_units blocks; kgroups key groups per block (1 or 2; -1: by shape);
// qgroups query groups of 16 per wave (1 or 2 = 128-query blocks, no key split; -1: by shape).
void attn_prefill_tr_launch(const AttnArgs& a, hipStream_t s, int nstg = 2, int pf_tiles = -1, int max_units = 256,
                            int kgroups = -1, int qgroups = -1);
size_t attention_workspace_floats(int B, int n_head, int head_dim, int max_ctx, int* max_chunks, int* chunk);
// Context splits per (row, head) of a decode attention launch (1 = the block writes ctx itself).
int attention_decode_splits(int B, int n_head, int max_chunks);

// ---- Verify pass (BS_STEP_VERIFY; attn_verify.hip) ----
// Attention of 2 <= a.S <= 8 queries per row, a.B * a.S <= kVerifyMaxTokens, head_dim <= 128, over the warm cache:
// grid (n_head, B, nsplit) with nsplit = attention_decode_splits(B, n_head, chunks of max_ctx), every row's length
// from a.past_dev -- nothing per call on the host side, so the launch can be captured.  a.part_acc / a.part_ml are
// the verify partials ([B * S][n_head][stride][head_dim] and [..][2], sized for kVerifyMaxTokens positions) and
// a.max_chunks their split stride (attention_verify_split_stride); a.tickets as for the decode kernel.  Split
// partials are folded in index order by the last block of each (row, head); bit-identical from run to run.
constexpr int kVerifyMaxTokens = 32;
int attention_verify_split_stride(int n_head, int max_chunks);
void launch_attention_verify(int is_bf16, const AttnArgs& a, hipStream_t s);

// ---- Int8 KV cache (bf16 stages with BS_FLAG_INT8_KV; kv_int8.hip) ----
// The fp32 scales beside the int8 codes of one layer ([max_batch][heads][max_ctx], K and V), and the bf16 staging
// buffers the QKV epilogue writes a call's new K / V rows to ([B][heads][lmax][hd], slot 0).
struct KvQ8 {
  float* k_scale;
  float* v_scale;
  __bf16* k_stage;
  __bf16* v_stage;
};
// S == 1: decode attention over the int8 cache (a.k_cache / a.v_cache = the layer's codes); the new token comes from
// staging [B][heads][1][hd] and is quantised into the cache at past_b by one block per (row, head).  Grids, partials
// and finishes are launch_attention's.
void launch_attention_q8(const AttnArgs& a, const KvQ8& kq, hipStream_t s);
// S > 1: cache positions [0, past_b) of rows slot.. -> staging (bf16((float)q * scale)); past_max = max_b past_b.
void launch_kv_dequant(const void* k_codes, const void* v_codes, const KvQ8& kq, const int* past_dev, int B, int slot,
                       int n_head, int head_dim, int max_ctx, int lmax, int past_max, hipStream_t s);
// S > 1: staging positions past_b .. past_b + S - 1 -> codes and scales at the same cache positions.
void launch_kv_quant(void* k_codes, void* v_codes, const KvQ8& kq, const int* past_dev, int B, int S, int slot,
                     int n_head, int head_dim, int max_ctx, int lmax, hipStream_t s);

// ---- KV row fork (bs_fork_kv; kv_fork.hip) ----
// Copy the first npos positions of cache row src_slot to rows [dst_slot, dst_slot + count) in one launch: `base` holds
// n_lw = layers * 2 images [max_batch][n_head][max_ctx] of pos_bytes each (the codes or values of the whole stage, or
// the fp32 scales of an int8 cache with pos_bytes = 4); every source chunk of chunk_bytes (16, or 4 for the scales;
// it divides npos * pos_bytes and the alignment of every segment start) is loaded once and stored count times.  Grid:
// one block per 1024 chunks, at most 8 per CU (cus), grid-stride beyond.  The row ranges must not overlap.
bool kv_fork_supported(int npos, size_t pos_bytes);
void launch_kv_fork(void* base, int chunk_bytes, int n_lw, int n_head, int max_batch, int max_ctx, size_t pos_bytes,
                    int src_slot, int dst_slot, int count, int npos, int cus, hipStream_t s);

// ---- Top-k log-prob tail (bs_forward_topk; beam_topk.hip) ----
// From fp32 logits [B][ld] (V columns each, ld % 4 == 0, 16-byte aligned): per row the k <= kTopkMaxK best token ids
// (larger logit first, the lower index first on equal logits) -> ids [B][k], their log-probabilities -> logprobs
// [B][k] and the row's log-sum-exp -> lse [B] (optional).  Two launches; the partials are one record per (row, slice
// of kTopkSlice logits): pmax, psum [B][topk_slices(V)] and pkeys [B][topk_slices(V)][kTopkMaxK].  The second launch
// does past_adv[b] += seq (optional): the pass's last kernel.  V <= kTopkSlice * kTopkMaxSlices.
constexpr int kTopkMaxK = 16;
constexpr int kTopkSlice = 2048;
constexpr int kTopkMaxSlices = 1024;
int topk_slices(int V);
void launch_topk_logprobs(const float* logits, int ld, int V, int B, int k, float* pmax, float* psum,
                          unsigned long long* pkeys, int* ids, float* logprobs, float* lse, int* past_adv, int seq,
                          hipStream_t s);

// Split-attention partials as the consumer reads them (attn_merge.h).
struct AttnParts {
  const float* acc;  // AttnArgs::part_acc
  const float* ml;   // AttnArgs::part_ml
  int nsplit, n_head, head_dim, max_chunks, slot;
};
// Can launch_linear_parts run M rows of a K-wide ctx split `nsplit` ways?
bool linear_parts_supported(int M, int K, int head_dim, int nsplit);
// Weight GEMV on ctx = merge(partials) (bf16): the dense projection after a deferred-merge attention.
void launch_linear_parts(const AttnParts& p, const void* W, int M, int N, int K, const Epi& ep, hipStream_t s);

// keys -> token ids
// Reduce the per-tile keys of each row (and keys_in[m] if given) -> keys_out[m] / tokens[m] (either optional).
// past_adv (optional): past_adv[m] += seq for every row (the decode step's last kernel advances the
// device copy of the cached lengths; stage.hip skips set_past when the host's next step matches it).
// adv_rows >= 0: only rows m < adv_rows advance (a verify pass reduces B * S positions of B rows).
void launch_argmax_finalize(const unsigned long long* keys, int M, int ntiles, const unsigned long long* keys_in,
                            unsigned long long* keys_out, int* tokens, hipStream_t s, int* past_adv = nullptr,
                            int seq = 0, int adv_rows = -1);
// ---- Greedy lm_head screening (bf16 stages, M <= 2, K <= 4096; kernels.hip "Greedy lm_head screening") ----
// The int8 shadow copy of the tied embedding with its per-row bound constants (made once at stage init) and the
// per-step buffers of the screened tail; ntiles = V / 16.
struct HeadScreen {
  const int8_t* Q;     // [V][K], launch_quantize_rows of the bf16 embedding
  const float* scale;  // [V]
  const float* cb;     // [V] launch_head_bound: |exact logit - int8 logit| <= ||x~|| * cb[n]
  float* hilo;         // [M][ntiles][2]: max(s^ + E), max(s^ - E) of each 16-row tile
  float* rnorm;        // [M] inflated ||x~_m||
  float* lstar;        // [M] max over tiles of lo
  int* list;           // [M][ntiles] candidate tiles (unordered)
  int* count;          // [M]
};
bool head_screen_supported(int M, int K);
// cb[n] >= ||w_n - scale_n Q_n||_2 + 2^-10 (||w_n||_2 + ||scale_n Q_n||_2), rounded up (fp64 sums).
void launch_head_bound(const void* W_bf16, const int8_t* Q, const float* scale, float* cb, int N, int K, hipStream_t s);
// (a) ln_f of rows x[m * row_stride + row_offset] + the int8 pass over Qh -> hilo, rnorm.  cus: CUs of the device.
void launch_head_screen(const HeadScreen& hs, const float* x, int row_stride, int row_offset, const void* gamma,
                        const void* beta, float eps, int M, int V, int K, int cus, hipStream_t s);
// (b) select the candidate tiles, (c) re-score them with the exact head's block body (ep: the EPI_ARGMAX epilogue
// of the full head, logits null), (d) reduce the listed keys -> tokens[m]; past_adv[m] += seq (the step's last kernel).
void launch_head_pick(const HeadScreen& hs, const float* x, int row_stride, int row_offset, const void* gamma,
                      const void* beta, float eps, const void* W, int M, int V, int K, const Epi& ep, int cus,
                      int* tokens, int* past_adv, int seq, hipStream_t s);
// Sequence-classification head: xn (T) [M][K] . score (T) [n_labels][K] -> logits fp32 [M][n_labels] (optional),
// cls[m] = first maximal label (inference.cpp:57-69); past_adv[m] += seq (optional).  n_labels <= 64, K % 8 == 0.
void launch_classify(int is_bf16, const void* xn, const void* score, int M, int n_labels, int K, float* logits,
                     int* cls, int* past_adv, int seq, hipStream_t s);
// past_dev[0..n) = values[0..n) (host), stream ordered, by kernel arguments (graph-capturable).
// Seeded top-k sampling (include/bloomstage.h bs_set_sampling; decoding.cpp:24-66) of M rows from the
// per-16-column tile keys (key_hi_index = 1) and the logits they came from ([M][ldl], column = vocab index).
// Row b's draw is keyed by (seed, KV row slot + b, position past_dev[b] + seq).
void launch_topk_sample(const unsigned long long* keys, int ntiles, const float* logits, int ldl, int M, int k,
                        float inv_temp, uint64_t seed, int slot, const int* past_dev, int seq, int* tokens,
                        hipStream_t s, int* past_adv = nullptr);
void launch_set_past(int* past_dev, const int* values, int n, hipStream_t s);

// ---- Per-row nucleus sampling (include/bloomstage.h "Per-row sampling"; row_sample.hip) ----
struct RowSamplerDev {  // one entry of the device table [max_batch]
  int top_k;
  float top_p;
  float temperature;
  int active;           // 0: the row takes the first index of its largest logit
  uint64_t seed;
};
struct RowDrawDev {     // the layout of bs_row_draw
  float threshold;
  int n_nucleus, n_candidates;
  uint32_t u24;
  uint64_t mass_nucleus, mass_candidates;
  int token, position;
};
struct RsState;
// The table is indexed by KV row; everything else by scratch lane.  The plain tail and bs_sample_logits use lane =
// KV row (one selection per row); a verify-draw pass has its own scratch of kVerifyMaxTokens lanes, one per position.
struct RowSampleBufs {
  RowSamplerDev* table;        // [max_batch]
  unsigned long long* rowmax;  // [lanes] max (key << 32 | ~index) of the step (zero between steps)
  uint32_t* hcnt;              // [lanes][6][2048] count histograms of the six digit passes (zero between steps)
  unsigned long long* hmass;   // [lanes][3][2048] fixed-point mass histograms of the last three
  RowDrawDev* draw;            // [lanes] read-out of each lane's last draw
  RsState* st;                 // [lanes][6] what one launch hands to the next
  int* pos;                    // [lanes] draw positions of a verify-draw pass (null in the per-row scratch)
};
// Bytes of all of the above but pos for `lanes` lanes (and a table of as many rows); offsets[6] receives where each
// array starts.  The buffer must be zero before the first launch.
size_t row_sample_bytes(int max_batch, size_t* offsets);
RowSampleBufs row_sample_bufs(char* base, const size_t* offsets);
// The scratch of a verify-draw pass: row_sample_bytes(kVerifyMaxTokens) plus the positions; row_sample_verify_bufs
// takes the table from `rows`.
size_t row_sample_verify_bytes(size_t* offsets);
RowSampleBufs row_sample_verify_bufs(const RowSampleBufs& rows, char* base, const size_t* offsets);
// table[slot .. slot + n) = rows[0..n) (host), stream ordered, by kernel arguments (set_past_kernel's pattern).
void launch_row_table(const RowSampleBufs& rb, int slot, const RowSamplerDev* rows, int n, hipStream_t s);
// Sample (or, for rows without state, take the first index of the largest logit of) rows [slot, slot + B) from
// logits [B][ld], V columns each.  Row b's position is positions[b] (host, passed by value) or, when positions is
// null, past_dev[b] + seq.  The last launch writes tokens[b], the row's read-out and past_adv[b] += seq (optional).
void launch_row_sample(const RowSampleBufs& rb, const float* logits, int ld, int V, int slot, int B,
                       const int* positions, const int* past_dev, int seq, int* tokens, int* past_adv, hipStream_t s);
// The tail of a verify-draw pass: M = B * S <= kVerifyMaxTokens selections, the same seven launches.  Selection m
// reads logits row m with the state of table row slot + m / S, works in lane m of `vb` (row_sample_verify_bufs) and
// draws at position past_dev[m / S] + m % S + 1 (fixed by the first launch in vb.pos, so the last one may advance
// past_dev); tokens[m] and vb.draw[m] receive the result.  One thread per KV row does past_adv[b] += S (optional).
void launch_row_sample_verify(const RowSampleBufs& vb, const float* logits, int ld, int V, int slot, int B, int S,
                              const int* past_dev, int* tokens, int* past_adv, hipStream_t s);

// ---- Per-row logit processors (include/bloomstage.h "Per-row logit processors"; logit_proc.hip) ----
constexpr int kRowBiasMax = 64;  // BS_ROW_BIAS_MAX
struct RowProcDev {  // one entry of the device table [max_batch]; bs_row_processor plus `active`
  float penalty;
  int ngram, min_new, eos, n_bias;
  int active;  // 0: the launches return at once for this row
  int bias_ids[kRowBiasMax];
  float bias_values[kRowBiasMax];
};
// Everything is indexed by KV row.  cap = max_ctx + 1 tokens a row; words = ceil(V / 32).
struct LogitProcBufs {
  RowProcDev* table;   // [max_batch]
  int* hist;           // [max_batch][cap] the ordered token history
  int* distinct;       // [max_batch][cap] each token of the history once, in no particular order
  uint32_t* seen;      // [max_batch][words] bit v: token v is in the history
  int* counts;         // [max_batch][4] = {history length, distinct tokens, generated tokens, unused}
  int cap, words, V;
};
// table[slot .. slot + n) = rows[0..n) (host, by kernel arguments) and the rows' histories emptied: the seen words of
// the distinct tokens back to zero (O(tokens noted)), the counts to zero.  Stream ordered.
void launch_logit_proc_set(const LogitProcBufs& lp, int slot, const RowProcDev* rows, int n, hipStream_t s);
// Append n tokens to row `slot`'s history, in order; ids outside [0, V) and tokens beyond cap are dropped.  ids_host:
// read now and passed by kernel arguments; else ids_dev is read on the stream.  generated: also count them as generated.
void launch_logit_proc_note(const LogitProcBufs& lp, int slot, const int* ids_host, const int* ids_dev, int n,
                            int generated, hipStream_t s);
// The tail's note: row slot + b with state appends tokens[b] and counts it as generated; rows without state return.
void launch_logit_proc_note_picks(const LogitProcBufs& lp, int slot, int B, const int* tokens, hipStream_t s);
// The rule in place on logits [B][ld] (V columns each) for rows [slot, slot + B); rows without state return at once.
void launch_logit_proc_apply(const LogitProcBufs& lp, float* logits, int ld, int slot, int B, hipStream_t s);

// ---- Guided decoding (include/bloomstage.h "Guided decoding"; guide.hip) ----
constexpr int kGuideMax = 16;      // BS_GUIDE_MAX
constexpr int kGuideSlice = 4096;  // BS_GUIDE_SLICE: vocabulary entries one block of the apply kernel owns
struct GuideDev {  // one entry of the device table [kGuideMax]; n_states == 0: not loaded
  const int* row_ptr;       // [n_states + 1]
  const int* edge_token;    // [edges] strictly ascending inside a state, in [0, V)
  const int* edge_next;     // [edges] in [-1, n_states)
  const int* default_next;  // [n_states] in [-1, n_states)
  int n_states, start;
};
struct GuideRowDev { int guide, state, n_steps, n_rejected; };  // one entry per KV row; guide < 0: no state
struct GuideBufs {
  GuideDev* guides;   // [kGuideMax]
  GuideRowDev* rows;  // [max_batch]
  int V;
};
// rows[slot .. slot + n) = {guide, states[i], 0, 0} (states: host, by kernel arguments; guide < 0 clears).  Stream ordered.
void launch_guide_set(const GuideBufs& gb, int slot, int n, int guide, const int* states, hipStream_t s);
// The rule in place on logits [B][ld] (V columns each) for rows [slot, slot + B): one launch of a (V slices, B) grid,
// every logit has one writer; rows without state return at once.
void launch_guide_apply(const GuideBufs& gb, float* logits, int ld, int slot, int B, hipStream_t s);
// The tail's advance: row slot + b with state steps by tokens[b]; rows without state return.  One launch.
void launch_guide_advance_picks(const GuideBufs& gb, int slot, int B, const int* tokens, hipStream_t s);
// Walk n tokens through row `slot`, in order.  ids_host: read now and passed by kernel arguments (one launch per
// guide_advance_arg_ids() of them); else ids_dev is read on the stream (one launch).
void launch_guide_advance(const GuideBufs& gb, int slot, const int* ids_host, const int* ids_dev, int n, hipStream_t s);
int guide_advance_arg_ids();

// ---- Weight-only int8 (bf16 stages with BS_FLAG_INT8_WEIGHTS; kernels.hip "Weight-only int8") ----
// Q[n][k] = rne(W[n][k] / scale[n]), scale[n] = max_k |W[n][k]| / 127 (1 for a zero row); W bf16 [N][K].
void launch_quantize_rows(const void* W_bf16, int8_t* Q, float* scale, int N, int K, hipStream_t s);
// out bf16 [N][K] = Q * scale (row-wise).
void launch_dequant_rows(const int8_t* Q, const float* scale, void* out_bf16, int N, int K, hipStream_t s);
// ---- Weight-only MXFP4 (bf16 stages with BS_FLAG_MXFP4_WEIGHTS; kernels.hip "Weight-only MXFP4") ----
// W bf16 [N][K], K % 32 == 0 -> E2M1 codes Q (N * K / 2 bytes, 16-B block records) + E8M0 scales SC [N][K / 32]
// by the rule of include/bloomstage.h.
void launch_quantize_mx4(const void* W_bf16, uint8_t* Q, uint8_t* SC, int N, int K, hipStream_t s);
// out bf16 [N][K] = the dequantised weights (exact in bf16).
void launch_dequant_mx4(const uint8_t* Q, const uint8_t* SC, void* out_bf16, int N, int K, hipStream_t s);

// ---- A block matrix as the stage holds it ----
// w: T [N][K] and both scales null; or int8 [N][K] with row_scale fp32 [N] (weight-only int8); or MXFP4 code
// records with blk_scale E8M0 [N][K / 32] (weight-only MXFP4).  The quantised formats belong to bf16 stages and
// never take EPI_ARGMAX (the tied lm_head stays bf16).  Epi::col_scale is set by the launches.
struct WMat {
  const void* w;
  const float* row_scale = nullptr;
  const uint8_t* blk_scale = nullptr;
};
// Does launch_wmat stream the stored weights for M rows (a decode GEMV, bound by wmat_stream_bytes), or run a
// GEMM (MXFP4 beyond its GEMV shapes and quantised prefill: on the weights dequantised into w_scratch)?
bool wmat_streams(int is_bf16, const WMat& w, int M, int N, int K);
// Weight and scale bytes of the matrix as a decode GEMV streams them.
double wmat_stream_bytes(const WMat& w, int N, int K, size_t esz);
// X (T; bf16 for a quantised w) [M][K] x W^T with epilogue; w_scratch: bf16 [N][K] for the dequantised weights.
void launch_wmat(int is_bf16, const void* X, const WMat& w, void* w_scratch, int M, int N, int K, const Epi& ep,
                 hipStream_t s);
// Does launch_wmat_ln take these rows?  Unquantised: always (launch_linear_ln).  Quantised: M <= 4, K <= 4096, the
// LayerNorm fused into the GEMV prologue; otherwise the caller runs launch_ln_rows, then launch_wmat.
bool wmat_takes_ln(const WMat& w, int M, int K);
void launch_wmat_ln(int is_bf16, const float* x, int row_stride, int row_offset, const void* gamma, const void* beta,
                    float eps, void* xn_scratch, const WMat& w, int M, int N, int K, const Epi& ep, hipStream_t s);
// The dense GEMV on ctx = merge(split-attention partials): can it run M rows of a K-wide ctx split `nsplit` ways?
bool wmat_parts_supported(const WMat& w, int M, int K, int head_dim, int nsplit);
void launch_wmat_parts(const AttnParts& p, const WMat& w, int M, int N, int K, const Epi& ep, hipStream_t s);
// LayerNorm of M fp32 rows -> bf16 (register-resident one-block-per-row kernel when K <= 4096).
void launch_ln_rows(const float* x, int row_stride, int row_offset, const void* gamma, const void* beta, float eps,
                    void* out_bf16, int M, int K, hipStream_t s);

// ---- Teacher-forced scoring head (bf16, K % 32 == 0, V % 16 == 0; head_score.hip) ----
// The tied lm_head W [V][K] against xn [M][K] fused with a log-softmax: per position the first index of the largest
// logit -> top_ids[m] and {logit[target] - lse (0 without a target), logit[top] - lse, lse} -> scores[m][3] (either
// output may be null; targets null or outside [0, V): no target).  No logit is stored: the GEMM blocks keep running
// statistics over their run of vocabulary tiles and leave head_score_partial_bytes(M, V, cus) bytes of partials in
// `parts`, folded per position in a fixed order by the second kernel, which also does past_adv[b] += seq for b < B
// (the pass's last kernel).  cus: CUs of the device (sizes the vocabulary splits).
int head_score_splits(int M, int V, int cus);
size_t head_score_partial_bytes(int M, int V, int cus);
void launch_head_score(const void* xn, const void* W, const int* targets, int M, int V, int K, int cus, void* parts,
                       int* top_ids, float* scores, int* past_adv, int B, int seq, hipStream_t s);
