/*
 * bloomstage.h — C-ABI of libbloomstage.so, the MI355X-native per-stage BLOOM forward.
 *
 * Drop-in boundary for the reference's JNI stage library.  Every entry
 * point below names the reference interface it replaces:
 *
 *   bs_init_stage      <- Java_..._Communication_createSession (native-lib.cpp:671-678)
 *                         + SessionCache ctor (session_cache.h:26-35): load one module
 *   bs_release         <- Java_..._Communication_releaseSession (native-lib.cpp:1290-1303)
 *   bs_forward         <- runInferenceMasterResidual (native-lib.cpp:942-1034, header stage),
 *                         runInferenceWorkerResidual (:1036-1194, middle stage),
 *                         runInferenceWorkerResidualLastGeneration (:1368-1443, tail stage),
 *                         all of which end in inference::run_inference (inference.cpp:145-218)
 *   bs_reset_kv        <- (none: the reference has no KV cache; new sample == new slot)
 *   bs_fork_kv         <- (none: no KV cache, so no shared prompt prefix to reuse)
 *   bs_copy_kv         <- (none: no KV cache, so no hypotheses' rows to reorder)
 *   bs_forward_score   <- (none: the reference has no scoring task)
 *   bs_forward_topk    <- (none: the reference's tail returns one token, decoding.cpp:24-66, never ranked candidates)
 *   bs_last_error      <- (none: the reference throws C++ exceptions across JNI,
 *                         native-lib.cpp:986-988; here errors are status codes + this string)
 *   bs_forward on a BS_FLAG_CLASSIFIER stage
 *                      <- runInferenceWorkerResidualLastClassification (native-lib.cpp:1305-1366)
 *                         -> inference::run_inference_with_binary_classification (inference.cpp:220-270)
 *   bs_binary_classify <- Java_..._binaryClassify (native-lib.cpp:128-160) -> inference::binary_classify
 *                         (inference.cpp:57-69)
 *   bs_codec_*         <- utils::SerializeTensorVectorToBytes / DeserializeTensorVectorFromBytes
 *                         (utils.cpp:124-264 / :266-368), byte-exact wire format
 *   bs_serialize_int / bs_deserialize_int
 *                      <- utils::SerializeInt / DeserializeInt (utils.cpp:11-25),
 *                         Java_..._deserializeInt (native-lib.cpp:1445-1471)
 *
 * Conventions: no exceptions cross this ABI; every int-returning call returns BS_OK (0)
 * or a negative bs_status and sets a thread-local message readable via bs_last_error().
 * Plain pointers and sizes only.  Device pointers live on the stage's device.
 */
#ifndef BLOOMSTAGE_H
#define BLOOMSTAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BS_ABI_VERSION 5

typedef enum {
  BS_OK = 0,
  BS_ERR_INVALID = -1,   /* bad argument / shape outside the stage's capacity */
  BS_ERR_DEVICE = -2,    /* HIP runtime error */
  BS_ERR_OOM = -3,       /* device allocation failed */
  BS_ERR_STATE = -4,     /* call not valid in the stage's current state */
  BS_ERR_UNSUPPORTED = -5/* e.g. wire dtype the reference codec does not carry */
} bs_status;

/* Element types: values are ONNXTensorElementDataType (onnxruntime_c_api.h:175-191). */
typedef enum {
  BS_DT_FLOAT = 1, BS_DT_UINT8 = 2, BS_DT_INT8 = 3, BS_DT_UINT16 = 4, BS_DT_INT16 = 5,
  BS_DT_INT32 = 6, BS_DT_INT64 = 7, BS_DT_BOOL = 9, BS_DT_DOUBLE = 11, BS_DT_UINT32 = 12,
  BS_DT_UINT64 = 13, BS_DT_BFLOAT16 = 16
} bs_dtype;

typedef enum {
  BS_WEIGHTS_SYNTHETIC = 0, /* repo generator (DESIGN.md "Synthetic weights"), built on device */
  BS_WEIGHTS_HOST = 1       /* fp32 host buffer in canonical stage order (bs_stage_weight_count) */
} bs_weight_source;

/* desc->flags.  BS_FLAG_INT8_WEIGHTS (bf16 stages): weight-only int8 for the four block matrices
 * (qkv, dense, fc1, fc2) -- the reference's bloom*-int8 model variants (server.py:796-799,
 * data/Data.kt:19-30).  Per output row n: scale[n] = max_k |W[n][k]| / 127 (1 for a zero row),
 * Q[n][k] = round-half-even(W[n][k] / scale[n]) in [-127, 127], W = the bf16 weight.  Embeddings,
 * LayerNorms, biases and the tied lm_head stay bf16; activations stay bf16/fp32 (weight-only).
 * bs_read_weights returns Q * scale for the quantized matrices. */
#define BS_FLAG_INT8_WEIGHTS 1
/* desc->flags.  BS_FLAG_CLASSIFIER (last stage): the tail of a BLOOM sequence classifier -- the reference's
 * classification task (task_type "classification", Communication.java:532, :596) whose tail sub-model ends in
 * logits that inference::binary_classify reduces to a class (inference.cpp:57-69, :220-270).  The head is HF
 * BloomForSequenceClassification's: ln_f on each row's last position (the pooled token of an unpadded row), then
 * score = Linear(hidden, n_labels, bias=False) -- checkpoint tensor "score.weight" [n_labels][hidden], canonical
 * order after ln_f -- instead of the tied lm_head.  bs_forward's out is an int32 class per row, the FIRST index
 * of the largest logit (binary_classify's strict > scan); logits (BS_STEP_LOGITS) are fp32 [B][n_labels].
 * desc->n_labels in [1, 64] (the reference reads 2).  The stage holds word_embeddings only if it is also first;
 * no head slice, no top-k sampling. */
#define BS_FLAG_CLASSIFIER 2
/* desc->flags.  BS_FLAG_INT8_KV (bf16 stages; BS_ERR_INVALID on an fp32 stage; head_dim a multiple of 16, else
 * BS_ERR_UNSUPPORTED): the KV cache holds int8 codes with one fp32 scale per (position, head) vector.  Orthogonal
 * to BS_FLAG_INT8_WEIGHTS and BS_FLAG_CLASSIFIER.
 *   Storage: codes [layer][K|V][slot][head][pos][hd] int8, scales [layer][K|V][slot][head][pos] fp32, both zero at
 *   init and after bs_reset_kv (a zero scale is finite: a masked position contributes exactly 0).
 *   Rule, per vector x of hd bf16 values (the BS_FLAG_INT8_WEIGHTS arithmetic): amax = max|x|,
 *   scale = amax > 0 ? amax / 127.f : 1.f (IEEE fp32 division), q = clamp(rintf(x / scale), -127, 127); the
 *   dequantised value is (float)q * scale (fp32 product).
 *   A call attends its own new positions at bf16 (the values its QKV epilogue produced) and every earlier cached
 *   position through the int8 cache, for seq == 1 and seq > 1 alike: a prompt prefilled in one call sees no
 *   quantisation.  A call with seq > 1 on rows that hold cached positions attends them as bf16((float)q * scale)
 *   (the prefill attention reads a bf16 staging copy); seq == 1 reads the codes and applies the fp32 scales.
 *   Staging: two bf16 buffers (K, V) of cap * hidden elements, cap = max(max_tokens as resolved, max_ctx), shared
 *   by the layers and counted under workspace_bytes.  A call with seq > 1 needs
 *   batch * (max past_len + seq) <= cap (BS_ERR_UNSUPPORTED otherwise; one row always fits).
 *   bs_read_kv returns the dequantised fp32 values; bs_stage_info reports
 *   kv_bytes = layers * 2 * max_batch * n_head * max_ctx * (head_dim + 4). */
#define BS_FLAG_INT8_KV 4
/* desc->flags.  BS_FLAG_MXFP4_WEIGHTS (bf16 stages; BS_ERR_UNSUPPORTED on an fp32 stage or when hidden is not a
 * multiple of 32; BS_ERR_INVALID together with BS_FLAG_INT8_WEIGHTS): weight-only OCP MXFP4 for the four block
 * matrices (qkv, dense, fc1, fc2): 4-bit E2M1 codes with one E8M0 scale byte per block of 32 weights, 0.53125 bytes
 * per weight.  Orthogonal to BS_FLAG_CLASSIFIER and BS_FLAG_INT8_KV.  Embeddings, LayerNorms, biases, the tied
 * lm_head (with its int8 screening copy) and the classifier score matrix stay bf16; activations stay bf16/fp32.
 *   Rule (OCP Microscaling Formats v1.0, round to nearest without calibration), per block = 32 consecutive k of one
 *   output row of the bf16 weight W: amax = max|W| over the block.  amax < 2^-100: E = 127 and every code is 0.
 *   Otherwise E = (biased fp32 exponent field of amax) - 2, i.e. floor(log2 amax) - emax with emax = 2 for E2M1.
 *   X = 2^(E - 127); |W| / X (exact) is rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even
 *   code, anything above 6 saturates to 6.  A code is the 3-bit grid index plus a sign bit (bit 3); the sign of a
 *   zero code is unspecified.  The dequantised value +-grid[index] * X is exact in bf16, so the stage computes the
 *   bf16 model whose host weights are the dequantised values.
 *   bs_read_weights returns the dequantised values; bs_stage_info reports the real storage under weight_bytes.  The
 *   device layout is private to the library. */
#define BS_FLAG_MXFP4_WEIGHTS 8

typedef struct bs_stage_desc {
  /* model (HF BloomConfig fields) */
  int32_t hidden;        /* hidden_size */
  int32_t n_head;        /* n_head */
  int32_t n_layer;       /* n_layer (whole model) */
  int32_t vocab;         /* vocab_size */
  float ln_eps;          /* layer_norm_epsilon */
  /* stage = contiguous layer range (server.py:893-905 assignment) */
  int32_t layer_begin;
  int32_t layer_end;     /* exclusive */
  int32_t is_first;      /* owns word_embeddings + word_embeddings_layernorm */
  int32_t is_last;       /* owns ln_f + tied lm_head + token pick */
  /* storage */
  int32_t dtype;         /* BS_DT_BFLOAT16 (weights + KV in bf16) or BS_DT_FLOAT */
  int32_t device;        /* HIP device ordinal */
  int32_t max_batch;     /* KV-cache rows (slots) */
  int32_t max_ctx;       /* positions per KV row */
  int32_t max_tokens;    /* max B*S per bs_forward call (0 -> max_batch*128) */
  /* weights */
  int32_t weight_source; /* bs_weight_source */
  uint64_t seed;         /* BS_WEIGHTS_SYNTHETIC */
  const float *host_weights;  /* BS_WEIGHTS_HOST */
  uint64_t host_weight_count; /* floats in host_weights */
  /* vocabulary-parallel head slice: lm_head rows [head_vocab_begin, head_vocab_end) + ln_f
   * (0, 0 = none).  Used by pipelines that spread the tied lm_head over all stages. */
  int32_t head_vocab_begin;
  int32_t head_vocab_end;
  int32_t flags;         /* BS_FLAG_* (0 = none) */
  int32_t n_labels;      /* BS_FLAG_CLASSIFIER: classes of the score head (else ignored) */
} bs_stage_desc;

typedef struct bs_stage bs_stage;

/* One forward call over B rows x S new tokens.  Every KV row (slot) keeps its own position:
 * the reference keeps core_pool_size samples in flight, each at its own position
 * (Communication.java:418-464, :621-651), so rows of one call may sit at different positions. */
typedef struct bs_step {
  int32_t batch;     /* B rows */
  int32_t seq;       /* S new tokens per row */
  int32_t slot;      /* first KV-cache row used by these B rows */
  int32_t past_len;  /* positions already cached in every row (used when past_lens is NULL) */
  int32_t flags;     /* BS_STEP_* */
  const int32_t *past_lens;  /* host [B]: positions already cached in row slot+b (per-row context
                                lengths, SURVEY.md §8b ctx_lens); NULL = past_len for all rows */
} bs_step;

#define BS_STEP_HOST_IO 1  /* in/out/logits are host pointers (copied in/out, stream-synchronous) */
#define BS_STEP_LOGITS 2   /* last stage also writes fp32 logits [B][vocab] of each row's last position */
/* step->flags.  BS_STEP_VERIFY (bs_forward, every stage of a generation model): a short pass of 2 <= seq <= 8 new
 * tokens per row with batch * seq <= 32 (BS_ERR_INVALID otherwise) over a warm cache -- the verify step of speculative
 * decoding: the row is fed [last token, draft_1 .. draft_k] and the greedy token of EVERY position comes back.
 *   in : as any forward.  out: a non-last stage writes fp32 hidden [B][S][hidden] as always; the last stage writes
 *        int32 ids [B][S], entry (b, t) = the first index of the largest logit of position past_b + t (the greedy
 *        rule).  logits (BS_STEP_LOGITS): fp32 [B][S][vocab].  BS_STEP_HOST_IO as for any forward.
 *   The pass appends S positions to the KV rows and its last kernel advances the device copy of each row's position
 *   by S, as every forward does.  Rolling a row back is the caller passing a smaller past_lens next time: a cache
 *   entry at or beyond a row's position is never read, by this pass or any other, so rejected drafts need no cleanup.
 *   The linears are the unflagged pass's (batched GEMVs on M = B * S rows; BS_FLAG_INT8_WEIGHTS and
 *   BS_FLAG_MXFP4_WEIGHTS stages work), so the K / V rows written equal the unflagged pass's of the same shape bit
 *   for bit; the attention is a short-query split-context kernel on a grid that is a static function of (B, n_head,
 *   max_ctx), the tail scores all B * S positions with the exact head (never screened:
 *   bs_read_head_screen reports *count = -1).  Results are bit-identical from run to run.  On device buffers the pass
 *   is captured and replayed like a decode step (bs_set_graphs).
 *   The first verify call allocates the attention's split partials and the per-position keys (counted under
 *   workspace_bytes from then on).
 *   BS_ERR_UNSUPPORTED on a BS_FLAG_INT8_KV stage; BS_ERR_STATE on a classifier stage, after bs_set_sampling chose
 *   top_k > 1, and on a last stage without the whole lm_head.  bs_forward_score rejects the flag (BS_ERR_INVALID). */
#define BS_STEP_VERIFY 4
/* step->flags.  BS_STEP_VERIFY_DRAW (only together with BS_STEP_VERIFY, else BS_ERR_INVALID; bs_forward_score rejects
 * it with BS_ERR_INVALID): the verify step of SAMPLED speculative decoding.  A draw of the per-row sampler depends on
 * (seed, position, logits) only, so the pass draws the row's own token at every position and the caller keeps the
 * prefix of its draft that agrees, as with greedy ids: every emitted token is the target's own draw, and the output
 * distribution is plain sampling's.
 *   A non-last stage accepts the flag and ignores it (a chain passes one set of flags to every stage).  On the last
 *   stage, out entry (b, t) of [B][S] is the row sampler's draw (bs_set_row_sampler's rule) on the fp32 logits of
 *   position past_b + t -- the values BS_STEP_LOGITS returns for it -- with the state of KV row slot + b at draw
 *   position past_b + t + 1, the index of the token being generated: what a plain seq == 1 step fed at past_b + t
 *   draws.  Rows of the call without state get the first index of their largest logit at every position.  A call
 *   none of whose rows holds state is the unflagged verify pass bit for bit (the argmax tail, not the sampler).
 *   The pass appends S positions; its last kernel (the sampler's pick) advances the device copy of each of the B
 *   rows' positions by S exactly once.  Rolling back, capture and replay are BS_STEP_VERIFY's: the launches and grids
 *   are a static function of (B, S, vocab), no launch argument is a per-call host value, and a bs_set_row_sampler
 *   between two replays takes effect without a recapture.  The pass works in sampler scratch of its own, one lane
 *   per position: the per-row scratch of plain sampled steps and bs_read_row_draw's read-outs are untouched.
 *   Every other condition is BS_STEP_VERIFY's: the shape limits, BS_ERR_UNSUPPORTED on an int8 KV cache, BS_ERR_STATE
 *   on a classifier, without the whole lm_head and after bs_set_sampling chose top_k > 1.  BS_STEP_VERIFY without
 *   this flag on a row with state stays BS_ERR_STATE.
 *   Workspace (counted under workspace_bytes from then on): the first pass that runs the sampler allocates the
 *   per-position scratch for 32 positions (max key, the six count and three mass histograms, launch-to-launch
 *   states, read-outs, positions; about 3 MB); the first such pass that is given no logits buffer allocates fp32
 *   logits of max(max_batch, 32) x vocab (a pass with BS_STEP_LOGITS writes and reads the caller's buffer, or with
 *   BS_STEP_HOST_IO the logits staging). */
#define BS_STEP_VERIFY_DRAW 8

/* Create a stage on desc->device: allocates weights, KV cache and workspace in HBM. */
int bs_init_stage(const bs_stage_desc *desc, bs_stage **out);

/* createSession(model_path) (native-lib.cpp:671-678 -> SessionCache, session_cache.h:26-35): create a
 * stage whose weights come from a checkpoint file instead of desc->weight_source.  `path` is a
 * safetensors file or a sharded checkpoint's *.index.json ({"weight_map": {name: shard}}, shards
 * beside it) holding HF BloomModel tensors ("h.<i>.self_attention.query_key_value.weight", ...;
 * a "transformer." prefix is accepted; "lm_head.weight" stands in for a missing
 * "word_embeddings.weight").  The file is memory-mapped and only the stage's own tensors are read;
 * F32/F16/BF16 are accepted and stored in desc->dtype (bf16 from fp32 rounds to nearest even,
 * exactly as BS_WEIGHTS_HOST).  A missing or mis-shaped tensor fails before any allocation. */
int bs_init_stage_file(const bs_stage_desc *desc, const char *path, bs_stage **out);
/* Model dimensions a checkpoint implies (hidden and vocab from word_embeddings, n_layer = 1 + the
 * highest block index); -1 where the file does not say.  Host only, no device needed. */
int bs_weights_file_probe(const char *path, int32_t *hidden, int32_t *n_layer, int32_t *vocab);

/* Stage forward, stream-ordered on `stream` (hipStream_t, NULL = the stage's own stream).
 * One stage is single-producer: its forwards share the stage's workspace, so a caller that moves a
 * stage from one stream to another must order the new stream behind the old one (an event wait);
 * the library then re-writes every row's position on the new stream itself.
 *  in : first stage -> int32 token ids [B][S]; otherwise fp32 hidden [B][S][hidden]
 *  out: last stage  -> int32 token ids [B] (greedy argmax of each row's last position; a BS_FLAG_CLASSIFIER
 *       stage: int32 class ids [B]); otherwise fp32 hidden [B][S][hidden]
 *  logits: fp32 [B][vocab] ([B][n_labels] on a classifier) when step->flags & BS_STEP_LOGITS (last stage
 *       only), else NULL.
 * Appends S positions to KV rows [slot, slot+B): row b's new positions are p_b .. p_b+S-1 with
 * p_b = past_lens[b] (or past_len).  The last stage's token pick is greedy argmax unless
 * bs_set_sampling selected top-k sampling. */
int bs_forward(bs_stage *stage, const bs_step *step, const void *in, void *out, float *logits,
               void *stream);

/* Teacher-forced scoring pass (last stage of a generation model, bf16): log-probabilities and greedy ids at every
 * position instead of a token at each row's last one -- perplexity, ranking by log-likelihood, and the verify step of
 * speculative decoding.  `step` and `in` are bs_forward's (B rows x S new tokens, per-row past_lens; ids on a
 * first + last stage, fp32 hidden otherwise); BS_STEP_HOST_IO covers in, targets, top_ids and scores; BS_STEP_LOGITS
 * is BS_ERR_INVALID.  Like bs_forward it appends S positions to the KV rows, and its last kernel advances the device
 * copy of each row's position by S, so a bs_forward (or another scoring chunk with past_len) on the same stream
 * continues from it.  Always launched eagerly; bs_read_head_screen reports the full head afterwards.
 *  Logits: for position (b, t), l[v] = the fp32-accumulated dot of bf16(ln_f(hidden[b][t])) with bf16 row v of the
 *       tied lm_head (the operands of bs_forward's head); lse = log sum_v exp(l[v]).  No logit is stored.
 *  targets: int32 [B][S], the token whose probability is wanted at that position's output; a value outside
 *       [0, vocab) (use -1) means none; NULL = none anywhere.
 *  top_ids: int32 [B][S], the first index of the largest l[v] (the greedy rule); may be NULL.
 *  scores: fp32 [B][S][3] = {l[target] - lse (0.0f without a target), l[top_id] - lse, lse}; may be NULL (not
 *       both).
 * Results are bit-identical from run to run (no floating-point atomics, partials folded in a fixed order).
 * BS_ERR_STATE on a classifier stage or a stage without ln_f and the whole lm_head (not last); BS_ERR_UNSUPPORTED on
 * an fp32 stage; BS_FLAG_INT8_WEIGHTS / BS_FLAG_MXFP4_WEIGHTS / BS_FLAG_INT8_KV stages score (the head stays bf16).  batch * seq <=
 * max_tokens.  The first scoring call allocates the head's per-split partials and the host-I/O staging (well under
 * max_tokens * vocab bytes; no buffer grows with batch * seq * vocab), counted under workspace_bytes from then on. */
int bs_forward_score(bs_stage *stage, const bs_step *step, const void *in, const int32_t *targets,
                     int32_t *top_ids, float *scores, void *stream);

/* Top-k log-prob pass (last stage of a generation model with the whole lm_head; bf16 and fp32, and BS_FLAG_INT8_WEIGHTS /
 * BS_FLAG_MXFP4_WEIGHTS / BS_FLAG_INT8_KV stages: the layers are bs_forward's): the k best tokens of each row's last
 * position with their log-probabilities -- the step of beam search and of any "logprobs / n-best" request (DESIGN.md
 * section 5i).  `step` and `in` are bs_forward's (B rows x S new tokens, per-row past_lens); BS_STEP_HOST_IO covers in,
 * ids, logprobs, lse and logits.  Like bs_forward it appends S positions to the KV rows and its last kernel advances
 * the device copy of each row's position by S; S == 1 on device buffers is captured and replayed like a decode step.
 * bs_read_head_screen reports the full head afterwards (*count = -1).
 *  With l[0..V) the fp32 logits of row b's last position (the values BS_STEP_LOGITS returns; every one finite):
 *  ids: int32 [B][k], ids[b][j] = the index of the j-th largest logit; equal logits rank by the lower index first,
 *       -0.0 and +0.0 are equal.  1 <= k <= 16.
 *  lse: fp32 [B], m + logf(sum_v expf(l_v - m)) with m = max l; may be NULL.
 *  logprobs: fp32 [B][k], l[ids[b][j]] - lse[b] (an fp32 subtraction).
 *  logits: fp32 [B][V] (a device buffer is 16-byte aligned); NULL = not wanted.
 * Given the logits the results are bit-identical from run to run and between graph replay and eager launch, and do
 * not depend on the row index, the batch or the grid: no floating-point atomics, the partial sums are folded in a
 * fixed order in which a term passes through at most 26 fp32 additions (beam_topk.hip).
 * BS_ERR_INVALID: k outside [1, 16], NULL ids or logprobs, BS_STEP_VERIFY / BS_STEP_VERIFY_DRAW / BS_STEP_LOGITS in
 * step->flags, bs_forward's shape checks.  BS_ERR_STATE: a classifier stage, a stage without the whole lm_head, after
 * bs_set_sampling chose top_k > 1, a row of the call that holds sampler state.  BS_ERR_UNSUPPORTED: vocab > 2^21.
 * The first call allocates the per-slice partials, the host-I/O staging and, if absent, the [max_batch][vocab] logits
 * buffer of bs_set_row_sampler, counted under workspace_bytes from then on. */
int bs_forward_topk(bs_stage *stage, const bs_step *step, const void *in, int32_t k, int32_t *ids, float *logprobs,
                    float *lse, float *logits, void *stream);

/* ---- Vocabulary-parallel head (stages with a head slice, or the last stage) ----
 * Argmax keys: uint64 (order(logit) << 32) | (0xFFFFFFFF - vocab_index), where order() maps
 * fp32 monotonically to uint32; the max key is the greedy token (lowest index on ties). */
/* ln_f of each row's last position: hidden fp32 [B][S][hidden] -> xn [B][hidden] in the stage's
 * activation type (bf16 for BS_DT_BFLOAT16 stages, fp32 otherwise). */
int bs_head_norm(bs_stage *stage, const float *hidden, int32_t batch, int32_t seq, void *xn, void *stream);
/* Logits of the stage's vocabulary slice for xn [B][hidden]; writes per-row keys
 * max(keys_in[b], slice max) to keys_out (either may be NULL) and, when tokens is non-NULL,
 * the decoded token ids.  keys_out may equal keys_in (the merge is per row, in place).  Device pointers,
 * stream ordered. */
int bs_head_slice(bs_stage *stage, const void *xn, int32_t batch, const uint64_t *keys_in, uint64_t *keys_out,
                  int32_t *tokens, void *stream);

/* ---- Tail token pick (last stage) ----
 * top_k <= 1: greedy argmax (the default; lowest index on ties, like torch.argmax).
 * 2 <= top_k <= 16: seeded top-k sampling restating decoding::StaticDecoding (decoding.cpp:24-66):
 *   the top_k (logit, index) pairs of each row's last position in std::greater order (larger logit
 *   first, the HIGHER index first on equal logits: decoding.cpp:44-45), weights
 *   w_i = exp((l_i - l_0) / temperature) -- with temperature 1 exactly the reference's "normalise
 *   the top-k probabilities by their sum" (:56-57) applied to softmax probabilities -- and the pick
 *   = the first i whose running sum of w exceeds u * sum(w), u in [0, 1) from the stage's counter
 *   generator keyed by (seed, KV row, position): reproducible, unlike the reference's
 *   std::random_device seed (:61-63).  The reference never applies its temperature argument
 *   (:51-52); pass 1 to reproduce it.  Not available on vocabulary-slice (bs_head_slice) stages.
 *   The draw depends on nothing else: two requests decoded with the same seed in the same KV row
 *   draw the same u at each position, so a server gives every request its own seed (for example
 *   base_seed ^ request_id, set before the request's first sampled step). */
int bs_set_sampling(bs_stage *stage, int32_t top_k, float temperature, uint64_t seed);

/* ---- Per-row sampling: top-k / top-p (nucleus) / temperature per KV row ----
 * Every KV row may hold a sampler state {top_k, top_p, temperature, seed}; a row without one is greedy.  Setting or
 * clearing a row's state is stream-ordered, does not synchronise and keeps every captured decode graph: a server
 * sets it when it admits a request into the row.
 *
 * Rule, for a row with state, on its fp32 logits l[0..V) (the values BS_STEP_LOGITS returns; all finite):
 *   weights     w_v = exp((l_v - max l) / temperature).
 *   candidates  C = the whole vocabulary for top_k == 0 or top_k >= V; else {v : l_v >= the top_k-th largest logit
 *               value} -- a tie at the k-th value keeps the whole level.
 *   nucleus     N = {v : l_v >= t}, t = the largest logit value with mass{v in C : l_v >= t} >= top_p * mass(C):
 *               whole level sets, never a partial tie; top_p == 1 gives N = C; N always holds the top level.
 *   draw        u = u24 / 2^24, u24 = the top 24 bits of the repo's counter generator (DESIGN.md "Synthetic
 *               weights": bits(key, i) with key = sm64(seed ^ sm64(0x524F575300000000)), i = position), position =
 *               the index of the token being generated (past_b + seq).  The KV row is not in the key: a request
 *               draws the same tokens in whichever row it lands.
 *   pick        the first v in vocabulary index order, among the members of N, whose running mass exceeds
 *               u * mass(N).
 * Arithmetic: masses are 64-bit fixed point, q_v = rint(w_v * 2^40) with w_v from an IEEE fp32 subtraction and
 * division and expf (one ulp); sums of V <= 2^18 terms stay below 2^58.  -0.0 and +0.0 are one level.  Every
 * comparison is exact integer arithmetic: mass >= ceil(top_p * mass(C)) with top_p's exact binary value (128-bit
 * product), running mass > (u24 * mass(N)) >> 24.  Integer sums do not depend on their order, so given the logits a
 * draw is bit-identical from run to run, between graph replay and eager launch, and independent of the row index,
 * the batch and the grid; there are no floating-point atomics.  Against the rule evaluated in real arithmetic the
 * masses are within a relative 2^-17 (argument rounding |arg| * 2^-23 for |arg| <= 40, one ulp of expf) plus V *
 * 2^-41 of quantisation. */
typedef struct bs_row_sampler {
  int32_t top_k;      /* 0 = no top-k limit */
  float top_p;        /* (0, 1] */
  float temperature;  /* > 0 */
  uint64_t seed;
} bs_row_sampler;
/* Read-out of a row's last draw.  A row without state: threshold = its largest logit, token = the first index of
 * it, position as given, the other fields 0. */
typedef struct bs_row_draw {
  float threshold;           /* t */
  int32_t n_nucleus;         /* |N| */
  int32_t n_candidates;      /* |C| */
  uint32_t u24;
  uint64_t mass_nucleus;     /* sum of q_v over N (2^40 fixed point) */
  uint64_t mass_candidates;  /* sum of q_v over C */
  int32_t token;
  int32_t position;
} bs_row_draw;
/* Set (params != NULL: [count] states) or clear (params == NULL) the sampler of KV rows [slot, slot + count), ordered
 * on `stream` (NULL = the stage's own) like a forward.  A bs_forward on a last stage whose rows include at least one
 * row with state takes the full head (never the int8 screen) and ends in the row sampler, for seq > 1 too (a
 * prefill's first generated token is sampled); rows of that call without state get the first index of their largest
 * logit.  A call with no such row is what it was before.  bs_forward_score is unaffected.
 * BS_ERR_INVALID: top_k < 0, top_p outside (0, 1], temperature <= 0, infinite or NaN, a bad row range.
 * BS_ERR_UNSUPPORTED: a classifier, a non-last stage, or a stage without the whole lm_head.  BS_ERR_STATE: setting a
 * state while bs_set_sampling holds top_k > 1 (and bs_set_sampling(top_k > 1) while a row holds state; BS_STEP_VERIFY
 * without BS_STEP_VERIFY_DRAW on a row with state).  The first call allocates the table, the selection histograms, the read-outs and, if absent,
 * the [max_batch][vocab] logits buffer, counted under workspace_bytes from then on. */
int bs_set_row_sampler(bs_stage *stage, int32_t slot, int32_t count, const bs_row_sampler *params, void *stream);
/* Run the row sampler -- the kernels the tail runs -- on caller-given fp32 logits [batch][ld] (ld >= vocab; device, or
 * host with BS_STEP_HOST_IO in flags, then tokens is host too and the call synchronises) for rows [slot, slot +
 * batch) at positions[b] (host).  Rows without state take the first index of the largest logit.  Touches no KV row
 * and no cached position.  Statuses as bs_set_row_sampler; allocates like it on first use. */
int bs_sample_logits(bs_stage *stage, int32_t slot, int32_t batch, const int32_t *positions, const float *logits,
                     int32_t ld, int32_t *tokens, int32_t flags, void *stream);
/* Read-out of row `slot`'s last draw, for verification (synchronises the device), like bs_read_head_screen.
 * BS_ERR_STATE on a stage that never ran the row sampler. */
int bs_read_row_draw(bs_stage *stage, int32_t slot, bs_row_draw *out);
/* Read-out of position t (0 <= t < seq) of KV row `slot` in the stage's last BS_STEP_VERIFY_DRAW pass that ran the
 * sampler (synchronises the device).  A row without state reads as bs_read_row_draw describes.  BS_ERR_STATE if no
 * such pass ever ran; BS_ERR_INVALID if the row or t was not part of the last one.  bs_read_row_draw keeps its
 * meaning: the row's last plain draw. */
int bs_read_verify_draw(bs_stage *stage, int32_t slot, int32_t t, bs_row_draw *out);

/* ---- Per-row logit processors: bias, repetition penalty, no-repeat n-gram, banned tokens, minimum new tokens
 *  ----
 * Every KV row may hold a processor state: the parameters below plus, on the device, the row's token history T (the
 * tokens noted with bs_note_tokens, then every token a forward picked for the row, in order), the set of distinct
 * tokens in it and the count of generated tokens.  Setting, clearing and noting are stream-ordered, do not synchronise
 * and keep every captured decode graph; a replayed graph applies the rule and records its own pick.
 *
 * Rule, on the row's fp32 logits l[0..V) of the position being generated (the values BS_STEP_LOGITS returns), in the
 * order of transformers' GenerationMixin._get_logits_processor; every step is plain fp32 arithmetic, so given the
 * logits and T the result is defined bit for bit:
 *   1 bias      for each entry (token, value) with a finite value, in entry order: l[token] += value (one fp32 add) --
 *               length-1 sequence_bias.
 *   2 penalty   r = repetition_penalty (> 0; 1 = off): for each DISTINCT token v of T, once:
 *               l[v] = l[v] < 0 ? l[v] * r : l[v] / r (an IEEE fp32 multiply or divide; -0.0 < 0 is false).
 *   3 n-gram    n = no_repeat_ngram (0 = off; 1..32), only if len(T) + 1 >= n: for every i with T[i .. i+n-2] equal to
 *               the last n-1 tokens of T, ban T[i+n-1].  n = 1 bans every token of T.
 *   4 bans      an entry whose value is -INFINITY bans its token (length-1 bad_words_ids).
 *   5 min new   while fewer than min_new_tokens tokens were generated in this row since the state was set, ban eos_id
 *               (only if eos_id >= 0).
 * "Ban" stores -FLT_MAX, not -inf: every tail's contract says "all logits finite" and stays true.  For the sampler,
 * the argument (-FLT_MAX - max l) / temperature is either a large negative finite number or -inf (the subtraction or
 * the division may overflow for |max l| large or temperature < 1) and never a NaN, because -inf only arises from
 * finite operands and is never subtracted from or divided by an infinity; expf of either is exactly 0, so a banned
 * token carries no mass at any temperature > 0 and is never drawn.  A row whose every token is banned picks the first
 * index (all logits equal).
 * Not here: frequency / presence penalties, min-p, multi-token sequence_bias and bad_words_ids, and two exclusions with
 * reasons: beam search (transformers applies the processors to log-softmax scores without
 * renormalising: another rule) and verify passes (a different seen-set at each position of the pass, and only the
 * accepted tokens may be noted). */
#define BS_ROW_BIAS_MAX 64
typedef struct bs_row_processor {
  float repetition_penalty;  /* > 0, finite; 1 = off */
  int32_t no_repeat_ngram;   /* 0 = off, else 1..32 */
  int32_t min_new_tokens;    /* >= 0 */
  int32_t eos_id;            /* < 0 = none */
  int32_t n_bias;            /* entries used below, 0..BS_ROW_BIAS_MAX */
  int32_t bias_ids[BS_ROW_BIAS_MAX];
  float bias_values[BS_ROW_BIAS_MAX];  /* finite: added; -INFINITY: the token is banned */
} bs_row_processor;
/* Set (params != NULL: [count] states) or clear (params == NULL) the processor state of KV rows [slot, slot + count),
 * ordered on `stream` (NULL = the stage's own) like a forward.  Either way the rows' token history and generated
 * counter are emptied, at a cost proportional to the tokens the row had noted, not to vocab.
 * A bs_forward on the last stage whose rows include at least one row with processor state takes the full head with
 * its logits written (never the int8 screen; to the caller's logits buffer, or to the shared [max_batch][vocab]
 * buffer), applies the rule in place, picks with the row sampler's launches (a row without sampler state gets the first
 * index of its largest logit; a row may hold sampler state, processor state, both or neither) and then appends each
 * stateful row's pick to its history and counts it as generated -- for seq > 1 too: the first generated token of a
 * prefill is processed.  BS_STEP_LOGITS then returns the PROCESSED logits, the values the pick saw.  The launches do
 * not depend on the table's contents (rows without state return at once inside them).  A call with no stateful row is
 * what it was before, bit for bit, the screened tail included.  bs_forward_score ignores the table; bs_reset_kv,
 * bs_fork_kv and bs_copy_kv do not touch token state.
 * BS_ERR_INVALID: repetition_penalty not finite or <= 0, no_repeat_ngram outside [0, 32], min_new_tokens < 0,
 * eos_id >= vocab, n_bias outside [0, 64], a bias id outside [0, vocab), a NaN or +inf bias value, a bad row range.
 * BS_ERR_UNSUPPORTED: a classifier, a non-last stage, or a stage without the whole lm_head.  BS_ERR_STATE: setting a
 * state while bs_set_sampling holds top_k > 1 (and bs_set_sampling(top_k > 1) while a row holds state);
 * bs_forward_topk, BS_STEP_VERIFY and BS_STEP_VERIFY_DRAW on a row with processor state.
 * The first call allocates the table, per row an int32 history and distinct list of max_ctx + 1 entries each, a seen
 * bitmap of ceil(vocab / 32) words and the counters, and, if absent, bs_set_row_sampler's buffers; all counted under
 * workspace_bytes from then on. */
int bs_set_row_processor(bs_stage *stage, int32_t slot, int32_t count, const bs_row_processor *params, void *stream);
/* bs_note_tokens flag: the tokens also count as generated (min_new_tokens). */
#define BS_NOTE_GENERATED 16
/* Append n tokens to row `slot`'s history (the prompt, before its prefill pass).  flags & BS_STEP_HOST_IO: ids is a
 * host pointer, read before the call returns; otherwise a device pointer read on `stream`.  No synchronisation,
 * captured graphs stay.  BS_ERR_INVALID: the history would exceed max_ctx + 1 tokens (the host keeps the length: every
 * note, plus one per forward of a row with state), a host id outside [0, vocab), other flags.  BS_ERR_STATE: a row
 * without processor state.  The device never writes out of bounds whatever the ids are: device-side ids outside
 * [0, vocab) are dropped. */
int bs_note_tokens(bs_stage *stage, int32_t slot, const int32_t *ids, int32_t n, int32_t flags, void *stream);
/* Run the apply kernel -- the one the tail runs -- in place on caller-given fp32 logits [batch][ld] (ld >= vocab;
 * device, or host with BS_STEP_HOST_IO in flags, then the call synchronises) for rows [slot, slot + batch).  Notes
 * nothing, touches no KV row.  Statuses as bs_set_row_processor; allocates like it on first use. */
int bs_process_logits(bs_stage *stage, int32_t slot, int32_t batch, float *logits, int32_t ld, int32_t flags,
                      void *stream);
/* Read-out of row `slot`'s token state, for verification (synchronises the device): tokens[0..*n_tokens) = the ordered
 * history (room for max_ctx + 1; may be NULL), the generated counter and the number of distinct tokens (any may be
 * NULL).  BS_ERR_STATE on a stage that never used the processors. */
int bs_read_row_tokens(bs_stage *stage, int32_t slot, int32_t *tokens, int32_t *n_tokens, int32_t *n_generated,
                       int32_t *n_distinct);

/* ---- Guided decoding: per-row token automata ----
 * A guide is a DFA over token ids in CSR form: state q owns the edges row_ptr[q] .. row_ptr[q + 1), each a token
 * (strictly ascending inside a state) and a next state, and a default next state for every other token:
 *   step(q, v)  = edge_next[e] if q has an edge e with edge_token[e] == v, else default_next[q]
 *   v is ALLOWED in q  iff  step(q, v) >= 0
 * A state that allows a handful of tokens has default_next = -1 and a few edges; a state that allows nearly the whole
 * vocabulary has default_next >= 0 and edges with edge_next = -1 for the explicit bans.  This is transformers'
 * prefix_allowed_tokens_fn, and what guided-decoding front ends make of a regex or a JSON schema and a tokenizer.
 *
 * Every KV row may hold a guide state (guide id, state q, two counters) on the device.  Rule, on the row's fp32 logits
 * l[0..V) of the position being generated, after step 5 of the processor rule above and before the pick (transformers'
 * order: prefix_allowed_tokens_fn follows min_new_tokens): every v that is not allowed in q gets l[v] = -FLT_MAX (the
 * processors' "ban": all logits stay finite and a banned token carries no sampler mass at any temperature); allowed
 * logits are not touched, bit for bit.  After the pick t the row's state becomes step(q, t) if t is allowed; otherwise
 * it stays q and the row's n_rejected counter goes up (only possible when the processors banned every allowed token and
 * the pick fell to the first index).  n_steps counts both.  Given the logits and q the result is defined bit for bit.
 * Multi-token bad_words_ids are expressible as a guide.  Not here: guides in verify passes and in beam search
 * (BS_ERR_STATE, for the processors' reasons). */
#define BS_GUIDE_MAX 16               /* guides a stage holds at a time */
#define BS_GUIDE_MAX_STATES (1 << 20)
#define BS_GUIDE_SLICE 4096           /* vocabulary entries one block of the apply kernel owns */
typedef struct bs_guide_desc {
  int32_t n_states;             /* 1 .. BS_GUIDE_MAX_STATES */
  int32_t start;                /* 0 .. n_states - 1 */
  const int32_t *row_ptr;       /* [n_states + 1], row_ptr[0] = 0, non-decreasing */
  const int32_t *edge_token;    /* [row_ptr[n_states]], in [0, vocab), strictly ascending inside a state */
  const int32_t *edge_next;     /* [row_ptr[n_states]], in [-1, n_states) */
  const int32_t *default_next;  /* [n_states], in [-1, n_states) */
} bs_guide_desc;
/* Load a guide (host arrays, copied to the device; may synchronise: meant to run outside the decode loop) and return
 * its id in *guide_id (0 .. BS_GUIDE_MAX - 1); unload frees it.  The kernels read guides through a fixed device table of
 * BS_GUIDE_MAX descriptors, so loading and unloading keep every captured graph.  The tables are validated on the host
 * before anything is allocated, BS_ERR_INVALID with a message that names the offending state: n_states outside
 * [1, 2^20], start out of range, row_ptr not starting at 0 or decreasing, tokens not strictly ascending inside a state
 * or outside [0, vocab), a next state outside [-1, n_states), a state that allows no token.  The first load also makes
 * the descriptor table and the rows' guide state (16 B a row); a guide's arrays (4 * (2 * n_states + 1 + 2 * edges)
 * bytes) are counted under workspace_bytes from load to unload.  BS_ERR_STATE: a 17th guide; unloading a guide a row
 * still references, or an id that is not loaded.  BS_ERR_UNSUPPORTED: a classifier, a non-last stage, or a stage
 * without the whole lm_head. */
int bs_load_guide(bs_stage *stage, const bs_guide_desc *guide, int32_t *guide_id);
int bs_unload_guide(bs_stage *stage, int32_t guide_id);
/* Give KV rows [slot, slot + count) guide `guide_id` and a state each (states[count], host, read before the call
 * returns and passed as kernel arguments; NULL: the guide's start state), or clear them (guide_id = -1).  Either way
 * the rows' n_steps and n_rejected counters are zeroed.  Ordered on `stream` (NULL = the stage's own) like a forward;
 * no synchronisation, captured graphs stay.
 * A bs_forward on the last stage whose rows include at least one guided row runs the processors' route with two
 * launches added: the full head with its logits written, the processors' apply, the guide apply, the row sampler's
 * launches as the pick, the processors' note, the guide advance.  A row may hold any subset of sampler, processor and
 * guide state.  BS_STEP_LOGITS returns what the pick saw; seq > 1 works (the first generated token of a prefill is
 * guided from the row's current state).  A call with no guided row enqueues what it did before.  bs_forward_score
 * ignores guides; bs_reset_kv, bs_fork_kv and bs_copy_kv do not touch guide state.  The first set allocates, if absent,
 * the buffers of bs_set_row_sampler and bs_set_row_processor (their launches are part of the route).
 * BS_ERR_INVALID: a bad row range, a state outside the guide.  BS_ERR_STATE: a guide id that is not loaded; setting
 * while bs_set_sampling holds top_k > 1 (and bs_set_sampling(top_k > 1) while a row is guided); bs_forward_topk,
 * BS_STEP_VERIFY and BS_STEP_VERIFY_DRAW on a guided row.  BS_ERR_UNSUPPORTED as bs_load_guide. */
int bs_set_row_guide(bs_stage *stage, int32_t slot, int32_t count, int32_t guide_id, const int32_t *states,
                     void *stream);
/* Walk n tokens through row `slot`'s state, in order, with the step rule: a token that is not allowed leaves the state
 * and counts as rejected (forced prefixes; re-entry after a caller-side rollback).  flags & BS_STEP_HOST_IO: ids is a
 * host pointer, read before the call returns (the ids travel as kernel arguments); otherwise a device pointer read on
 * `stream`, where an id outside [0, vocab) is rejected.  No synchronisation, captured graphs stay.  BS_ERR_INVALID: a
 * host id outside [0, vocab), other flags.  BS_ERR_STATE: the row is not guided. */
int bs_advance_row_guide(bs_stage *stage, int32_t slot, const int32_t *ids, int32_t n, int32_t flags, void *stream);
/* Run the guide apply kernel -- the one the tail runs -- in place on caller-given fp32 logits [batch][ld] (ld >= vocab;
 * device, or host with BS_STEP_HOST_IO in flags, then the call synchronises) for rows [slot, slot + batch).  Advances
 * nothing.  Rows whose base address is 16-byte aligned take 16-byte stores, others 4-byte ones.  BS_ERR_STATE on a
 * stage that never loaded a guide. */
int bs_guide_logits(bs_stage *stage, int32_t slot, int32_t batch, float *logits, int32_t ld, int32_t flags,
                    void *stream);
/* Read-out of row `slot`'s guide state, for verification (synchronises the device): the guide id (-1: none), the state
 * and the two counters (any may be NULL).  BS_ERR_STATE on a stage that never loaded a guide. */
int bs_read_row_guide(bs_stage *stage, int32_t slot, int32_t *guide_id, int32_t *state, int32_t *n_steps,
                      int32_t *n_rejected);

/* Decode steps (S = 1) and BS_STEP_VERIFY passes on device buffers are captured once per shape into a hipGraph and replayed
 * (the default, on = 1); on = 0 launches them eagerly every step (same kernels, same results: for
 * debugging and A/B timing).  Drops captured graphs.  Returns BS_OK.  A stage starts with graphs off
 * when the environment holds BS_GRAPHS=0 at bs_init_stage (rocprofv3 --pmc runs). */
int bs_set_graphs(bs_stage *stage, int32_t on);

/* ---- Greedy head screening ----
 * A bf16 last stage of a generation model keeps, besides the bf16 tied lm_head, an int8 shadow copy of it (the
 * BS_FLAG_INT8_WEIGHTS rule) with one rigorous error-bound constant per vocabulary row, built once at init and
 * counted under workspace_bytes of bs_stage_info.  A greedy forward (top_k <= 1) of at most 2 rows that requests no
 * logits streams the int8 copy, marks the 16-row tiles that cannot hold the largest logit, and runs the exact bf16
 * head on the remaining tiles only: the token ids are bit-identical to the full head's (first index on ties); logits,
 * sampling and every other shape take the full head.  on = 0 always takes the full head (for A/B runs and debugging);
 * on = 1 needs the shadow copy (BS_ERR_STATE otherwise: fp32 or classifier stages, hidden > 4096, or an allocation
 * that failed at init).  Synchronizes and drops captured graphs.  A stage starts with screening on where the shadow
 * copy exists, unless the environment holds BS_HEAD_SCREEN=0 (read once per process). */
int bs_set_head_screen(bs_stage *stage, int32_t on);
/* Read-out of the stage's last forward, for verification: *count = -1 when its tail took the full head; otherwise,
 * for row `row` of that forward, hilo[vocab/16][2] = per 16-row tile (upper bound of the tile's largest logit, lower
 * bound of it), *lstar = the largest lower bound, list[0..*count) = the candidate tiles (unordered; list needs room
 * for vocab/16 entries).  hilo, lstar and list may be NULL.  Synchronizes the device. */
int bs_read_head_screen(bs_stage *stage, int32_t row, float *hilo, float *lstar, int32_t *list, int32_t *count);

/* Forget the cached positions of one KV row (slot), or of all rows when slot < 0. */
int bs_reset_kv(bs_stage *stage, int32_t slot);
/* Read back KV row `slot` of the stage's local layer `layer`, positions [pos0, pos0 + npos), as fp32
 * out[2 (K, V)][n_head][npos][head_dim].  Synchronizes the stage's own stream; the caller orders any
 * other stream it forwarded on.  For verification (parity tests hand a device cache to the checker). */
int bs_read_kv(const bs_stage *stage, int32_t layer, int32_t slot, int32_t pos0, int32_t npos, float *out);
/* KV row fork: copy cached positions [0, npos) of KV row src_slot to rows [dst_slot, dst_slot +
 * count), all layers of the stage, K and V, every head; ordered on `stream` (NULL = the stage's own) like a forward.
 * A prompt prefix prefilled once into one row serves every row that begins with it: fork, then a continuation
 * bs_forward (seq > 1 at past_len = npos) of the rest of the row's prompt.
 *   Ordering: the call enqueues and returns; it does not synchronise, allocates nothing and keeps every captured graph.
 *   The caller orders it behind the forwards that wrote the source row and ahead of the next forward on the
 *   destination rows -- the same stream, or an event; one stage is single-producer (bs_forward).  One launch whatever
 *   the layer count, one more for the scales of a BS_FLAG_INT8_KV cache.
 *   Exact copy: afterwards positions [0, npos) of every destination row hold the source row's bits -- bf16 or fp32
 *   elements; on a BS_FLAG_INT8_KV cache the int8 codes and the fp32 scales verbatim, nothing is re-quantised.
 *   Nothing else is written: positions >= npos of the destination rows, every other row and the source stay as they
 *   were, as do the bf16 staging of an int8 cache, the device copy of the rows' positions (indexed by a row's place in
 *   a call, not by slot: the next forward's past_lens says where the rows stand) and the per-row sampler table (a
 *   forked row keeps the sampler state it had; bs_set_row_sampler sets it).
 *   BS_OK and no launch for npos == 0, count == 0 or a stage without layers.  BS_ERR_INVALID: a NULL stage, a negative
 *   slot, count or npos, a slot range outside max_batch, npos > max_ctx, src_slot inside [dst_slot, dst_slot + count). */
int bs_fork_kv(bs_stage *stage, int32_t src_slot, int32_t dst_slot, int32_t count, int32_t npos, void *stream);
/* KV row pair copy: for i < count, cached positions [0, npos) of KV row src_slots[i] to row
 * dst_slots[i] (host arrays, read before the call returns: no host-to-device copy, no device buffer), all layers of
 * the stage, K and V, every head -- the reordering step of beam search, where children take over the rows of dead
 * hypotheses.  A source may appear several times.  The rest of the contract is bs_fork_kv's: stream-ordered, no
 * synchronisation, no allocation, captured graphs stay; an exact copy for bf16, fp32 and int8 caches (codes and scales
 * verbatim, the scales in a launch of their own); nothing else is written.  The copies are bs_fork_kv's launches, one
 * per run of consecutive pairs that share a source and whose destinations are consecutive rows (a one-launch
 * pair-list kernel measured slower than those launches and was dropped).
 *   BS_OK and no launch for count == 0, npos == 0 or a stage without layers.  BS_ERR_INVALID: a NULL stage, NULL lists
 *   with count > 0, count outside [0, 32], a slot outside [0, max_batch), npos outside [0, max_ctx], a destination that
 *   appears twice, a destination that is also a source (so the launches have no ordering hazard among themselves). */
int bs_copy_kv(bs_stage *stage, const int32_t *src_slots, const int32_t *dst_slots, int32_t count, int32_t npos,
               void *stream);

void bs_release(bs_stage *stage);

const char *bs_last_error(void);

/* Introspection */
int bs_stage_info(const bs_stage *stage, bs_stage_desc *out_desc, uint64_t *weight_bytes,
                  uint64_t *kv_bytes, uint64_t *workspace_bytes);
/* fp32 count for BS_WEIGHTS_HOST.  Canonical order: [word_embeddings if first, or last and not a classifier]
 * [emb LN g,b if first]{per layer: ln1 g,b, qkv w,b, dense w,b, ln2 g,b, fc1 w,b, fc2 w,b}
 * [ln_f g,b if last][score [n_labels][hidden] if a classifier]
 * [head slice rows if a slice is set and the stage is neither first nor last]
 * [ln_f g,b if a slice is set and the stage is not last]. */
uint64_t bs_stage_weight_count(const bs_stage_desc *desc);
int bs_abi_version(void);
/* Build provenance: hex SHA-256 of the library's sources (csrc files and include/bloomstage.h) stamped at
 * compile time; the Python binding refuses a library whose stamp differs from the sources beside it. */
const char *bs_build_id(void);
/* Read back `count` weights starting at element `offset` of the canonical stage order
 * (the BS_WEIGHTS_HOST layout) as fp32.  For verification of loaded/generated weights. */
int bs_read_weights(const bs_stage *stage, uint64_t offset, uint64_t count, float *out);
/* Synthetic prompt ids of the repo generator (DESIGN.md "Synthetic weights"): ids[i] for the
 * flat index i of a [B][S] prompt, uniform over [0, vocab). */
int bs_prompt_ids(uint64_t seed, int32_t n, int32_t vocab, int32_t *out);

/* Profiling: time every launch of one kernel class with HIP events on the stage stream.
 * kernel_class: 0 off, 1 weight GEMV (decode), 2 GEMM (prefill), 3 attention.
 * bs_profile_read returns accumulated milliseconds, launch count and algorithmic bytes
 * (or flops for class 2) since the last bs_profile_enable; it synchronizes the stream. */
int bs_profile_enable(bs_stage *stage, int32_t kernel_class);
int bs_profile_read(bs_stage *stage, double *total_ms, uint64_t *launches, double *algo_units);
/* Enqueue a one-thread spin of `microseconds` (<= 100000) on `stream` (hipStream_t; NULL = the
 * default stream of the current device): lets the host enqueue a whole profiled step behind it,
 * so event-timed launches are not stretched by host submission gaps. */
int bs_stream_delay(void *stream, int32_t microseconds);

/* Measurement aid (bench.py "hbm_measured"): STREAM-like HBM rates of a device, best of 10 runs over
 * `bytes` (a multiple of 1 MiB) -- read: non-temporal 16-B loads; copy: read + write bytes / time. */
int bs_hbm_probe(int32_t device, uint64_t bytes, double *read_gbps, double *copy_gbps);
/* Measurement aid (bench.py "mfma_measured"): dense bf16 matrix-core TFLOP/s of a device, best of 5 runs of
 * register-operand v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 chains (8 independent chains per wave,
 * 8 waves per CU, no memory traffic).  The measured counterpart of the vendor dense peak. */
int bs_mfma_probe(int32_t device, double *tflops_32x32x16, double *tflops_16x16x32);

/* ---- Reference wire codec (utils.cpp:124-368): size_t n; per tensor {int32 dtype,
 * size_t ndim, int64 dims[ndim], raw little-endian data}. size_t is 8 bytes (LP64). ---- */
#define BS_CODEC_MAX_DIMS 8
typedef struct bs_tensor_view {
  int32_t dtype;                     /* bs_dtype */
  int32_t ndim;
  int64_t dims[BS_CODEC_MAX_DIMS];
  const void *data;                  /* may be unaligned when it points into a wire buffer */
} bs_tensor_view;

/* Serialize n tensors. Returns the total byte count (also when out is NULL or too small:
 * then nothing is written) or a negative bs_status. */
int64_t bs_codec_serialize(const bs_tensor_view *tensors, int32_t n, void *out, uint64_t out_cap);
/* Parse a wire buffer into zero-copy views. *n_out receives the tensor count; at most
 * max_views are filled. Returns BS_OK or a negative bs_status (truncated / unsupported). */
int bs_codec_deserialize(const void *bytes, uint64_t len, bs_tensor_view *views, int32_t max_views,
                         int32_t *n_out);
int64_t bs_dtype_size(int32_t dtype);
/* binaryClassify(byte[]) (native-lib.cpp:128-160): the first tensor of a wire buffer holds logits; *cls = the
 * first index of the larger of its first two floats (inference::binary_classify, inference.cpp:57-69).  Host
 * only.  BS_ERR_INVALID for an unparsable buffer, no tensor, a non-float tensor or fewer than two elements
 * (the reference returns -1 / -2 there, or reads past a short tensor). */
int bs_binary_classify(const void *bytes, uint64_t len, int32_t *cls);
/* 4-byte native (little-endian) int, as the tail stage returns a token id. */
void bs_serialize_int(int32_t value, uint8_t out[4]);
int bs_deserialize_int(const uint8_t *bytes, uint64_t len, int32_t *value);

#ifdef __cplusplus
}
#endif
#endif /* BLOOMSTAGE_H */
