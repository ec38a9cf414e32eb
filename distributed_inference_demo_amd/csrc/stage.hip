// stage.hip — libbloomstage C-ABI (include/bloomstage.h): stage lifetime + forward orchestration.
//
// Replaces the reference's per-device stage execution:
//   SessionCache / createSession (session_cache.h:20-35, native-lib.cpp:663-678)  -> bs_init_stage
//   run_inference + JNI wrappers (inference.cpp:145-218, native-lib.cpp:942-1443)  -> bs_forward
//   releaseSession (native-lib.cpp:1290-1303)                                       -> bs_release
// Everything the ONNX sub-model computed on the CPU is here a sequence of gfx950 kernels
// (kernels.hip) over weights, KV cache and workspace resident in the stage GPU's HBM.
//
// Sections, in order:
//   errors and tracing; Carver (one device allocation cut into aligned pieces); bs_stage and the allocations it owns
//   validate, bs_stage_weight_count (the weight table is stage_weights.h), checkpoint lookup
//   init_stage: weight arena + binding, the three weight sources, head screening, KV cache, workspace
//   bs_stage_info, bs_read_weights, bs_read_kv, bs_reset_kv, bs_fork_kv, bs_copy_kv
//   profiling, bs_stream_delay, the HBM and MFMA probes
//   the forward: linear / linear_ln, Tail (which tail a pass ends in, decided once), enqueue_forward
//   head slices, sampling setters, the per-row sampler and verify-draw buffers, the graph cache
//   forward_impl (checks, lazy buffers, capture or eager enqueue), bs_forward, bs_forward_score, bs_forward_topk
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bloomstage.h"
#include "common.h"
#include "guide_table.h"
#include "kernels.h"
#include "safetensors.h"
#include "stage_weights.h"

static thread_local std::string g_err;

// BS_TRACE_CALLS=1: one stderr line (flushed) before each HIP runtime call bs_forward makes, so a host fault inside
// the runtime names the call it happened in (the round-5 SIGSEGV under rocprofv3).
static bool trace_calls() {
  static const bool on = [] { const char* e = getenv("BS_TRACE_CALLS"); return e && e[0] == '1'; }();
  return on;
}
#define BS_TRACE(...)                                         \
  do {                                                        \
    if (trace_calls()) {                                      \
      fprintf(stderr, "[bs_forward] " __VA_ARGS__);           \
      fputc('\n', stderr);                                    \
      fflush(stderr);                                         \
    }                                                         \
  } while (0)

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(BS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
  } while (0)

namespace {

struct Layer {
  void* t[T_NLAYER];
  float* sc[T_NLAYER];  // int8 stages: per-row scales of the four weight matrices (else null)
  uint8_t* mxs[T_NLAYER];  // MXFP4 stages: E8M0 block scales of the four weight matrices (else null); t[] = codes
};

// What a pass ends in.  plan_tail decides it once per call from the stage state and the step; enqueue_forward, the
// graph key, the lazy buffers and the read-out bookkeeping all take it from there.
enum TailKind {
  TAIL_NONE,           // not the last stage: hidden states out
  TAIL_CLASSIFY,       // ln_f of each row's last position, score, first maximal class
  TAIL_SCORE,          // bs_forward_score: log-softmax head over every position
  TAIL_VERIFY_ARGMAX,  // BS_STEP_VERIFY: the greedy id of every position
  TAIL_VERIFY_DRAW,    // BS_STEP_VERIFY_DRAW on rows with sampler state: the row sampler's draw at every position
  TAIL_SCREENED,       // greedy, <= 2 rows, no logits: int8 screening pass + exact re-score
  TAIL_GREEDY,         // full head, argmax
  TAIL_TOPK,           // full head, bs_set_sampling's seeded top-k
  TAIL_ROWS,           // full head, per-row sampler (a row of the call holds sampler state)
  TAIL_ROWS_PROC,      // full head with its logits written, the per-row logit processors on them, the per-row sampler as
                       // the pick, the picks noted in the rows' histories (a row of the call holds processor state)
  TAIL_ROWS_GUIDE,     // TAIL_ROWS_PROC with the guide apply ahead of the pick and the guide advance behind the note (a row
                       // of the call holds guide state)
  TAIL_TOPK_LOGPROBS,  // bs_forward_topk: full head with its logits written, the k best ids and log-probs of each row
};
struct Tail {
  TailKind kind = TAIL_NONE;
  int rows = 0;   // ids (and logits rows) the tail writes: batch, or batch * seq for the verify tails
  int width = 0;  // logits per row: n_labels or vocab
};

struct GraphKey {
  int B, seq, slot, flags;
  TailKind tail;  // row-sampler, row-processor and row-guide state change the tail of otherwise equal calls: the kind is the
                  // key's bit for the route (the setters that change it for every call drop the graphs instead)
  const void* in;
  void* out;
  float* logits;
  hipStream_t st;
  int k = 0;  // TAIL_TOPK_LOGPROBS: candidates per row, and where the log-probs and the lse go (out = the ids)
  const void* logprobs = nullptr;
  const void* lse = nullptr;
  bool operator==(const GraphKey& o) const {
    return B == o.B && seq == o.seq && slot == o.slot && flags == o.flags && tail == o.tail && in == o.in &&
           out == o.out && logits == o.logits && st == o.st && k == o.k && logprobs == o.logprobs && lse == o.lse;
  }
};

struct ProfClass {
  int cls = 0;
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  double algo = 0.0;
};

}  // namespace

// Split-K workspace of the batched decode GEMV (kernels.hip gemv_tiles_dispatch): up to 16 splits
// of 32 rows x 4096 columns, one ticket per 16-column tile.  Used only by enqueue_forward's GEMVs
// (one stream per stage); head slices on another stream never split K.
// Also the prefill GEMMs' partials: gemm_mfma3's stream-K slabs (2 per block of a grid of up to 512) and
// gemm_split_k's 64x64 split-K tiles.
constexpr size_t kSkCap = (size_t)1024 * 128 * 128;
constexpr int kSkTickets = 4096;

// BS_HEAD_SCREEN=0 (read once): stages start with the greedy head screening off (A/B runs).
static int head_screen_default() {
  static const int v = [] { const char* e = getenv("BS_HEAD_SCREEN"); return (e && e[0] == '0') ? 0 : 1; }();
  return v;
}

static int graphs_default() {
  const char* e = getenv("BS_GRAPHS");
  return (e && e[0] == '0') ? 0 : 1;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One device allocation cut into typed pieces, each 256-B aligned: piece() names where each pointer goes and its
// size, alloc() allocates once and sets the pointers (none of them on failure).
struct Carver {
  std::vector<std::pair<void**, size_t>> pieces;  // (pointer to set, offset)
  size_t total = 0;
  char* base = nullptr;
  template <typename T>
  void piece(T** p, size_t bytes) {
    pieces.push_back({(void**)p, total});
    total = align_up(total + bytes, 256);
  }
  enum { OK, NO_MEMORY, NOT_ZEROED };
  // zero_on (the stage's own stream): the pieces are zeroed there and the stream synchronised before any other stream
  // can write them (a plain hipMemset of device memory may still be running when it returns, and the caller's
  // stream is not ordered behind it).  Nothing stays allocated on failure.
  int alloc(hipStream_t zero_on = nullptr) {
    if (hipMalloc((void**)&base, total ? total : 256) != hipSuccess) return NO_MEMORY;
    if (zero_on && (hipMemsetAsync(base, 0, total, zero_on) != hipSuccess || hipStreamSynchronize(zero_on) != hipSuccess)) {
      hipFree(base);
      return NOT_ZEROED;
    }
    for (auto& p : pieces) *p.first = base + p.second;
    return OK;
  }
};

// A device allocation the stage owns; `counted` is what bs_stage_info reports of it as workspace beside `ws`.
struct OwnedAlloc {
  void* p;
  size_t counted;
};

struct bs_stage {
  bs_stage_desc d;
  int bf16 = 1;
  int q8 = 0;              // BS_FLAG_INT8_WEIGHTS: block matrices int8 + row scales
  int mx4 = 0;             // BS_FLAG_MXFP4_WEIGHTS: block matrices E2M1 codes + E8M0 block scales
  int kv8 = 0;             // BS_FLAG_INT8_KV: int8 KV codes + fp32 scales, bf16 staging (kv_int8.hip)
  size_t esz = 2;
  void* wtmp = nullptr;    // int8 / MXFP4 stages: bf16 [4h][h] staging (init) and dequantized operand (prefill)
  int hd = 0, L = 0;
  hipStream_t own = nullptr;
  // HBM
  size_t wbytes = 0;
  void* wemb = nullptr;
  void* emb_g = nullptr;
  void* emb_b = nullptr;
  void* lnf_g = nullptr;
  void* lnf_b = nullptr;
  void* hw = nullptr;     // head slice rows [hv0, hv1) of the tied lm_head (may point into wemb)
  int hv0 = 0, hv1 = 0;
  void* score = nullptr;  // BS_FLAG_CLASSIFIER: score [n_labels][hidden] (the head instead of the lm_head)
  int n_labels = 0;
  std::vector<Layer> layers;
  char* kv = nullptr;  // [L][2][max_batch][heads][max_ctx][hd]
  // BS_FLAG_INT8_KV: kv holds the int8 codes in that layout (kv_half / kv_layer_stride in bytes of codes), then the
  // fp32 scales [L][2][max_batch][heads][max_ctx] at kv_scales; kv_stage: two bf16 staging buffers (K, V) of
  // kv_stage_cap positions x hidden each, shared by the layers
  float* kv_scales = nullptr;
  size_t kv_sc_half = 0;       // scales of K (or V) of one layer
  char* kv_stage = nullptr;
  size_t kv_stage_cap = 0;
  size_t kvbytes = 0;
  size_t kv_layer_stride = 0;  // bytes per (layer) = 2 * half
  size_t kv_half = 0;          // bytes for K (or V) of one layer
  char* ws = nullptr;
  size_t wsbytes = 0;
  float* xa = nullptr;   // fp32 [T][h]
  float* xb = nullptr;   // fp32 [T][h]
  float* attn = nullptr; // fp32 [T][h]
  void* q = nullptr;     // act [T][h]
  void* xn = nullptr;    // act [T][h]
  void* ctx = nullptr;   // act [T][h]
  void* g = nullptr;     // act [T][4h]
  float* part_acc = nullptr;
  float* part_ml = nullptr;
  int max_chunks = 0, chunk = 64;
  float* slopes = nullptr;
  unsigned long long* keys = nullptr;  // [max_batch][V/16]
  int* tok = nullptr;                  // [max_batch]
  int* ids = nullptr;                  // [T] staging for host ids
  int* past_dev = nullptr;
  unsigned* att_tickets = nullptr;     // [max_batch][n_head]
  std::vector<int> past_next;          // what past_dev[0..B) holds after the enqueued forwards (last stage)
  bool past_next_valid = false;
  hipStream_t past_stream = nullptr;   // the stream those forwards were enqueued on
  float* sk_ws = nullptr;              // batched-GEMV split-K partials (kSkCap floats)
  unsigned* sk_tickets = nullptr;      // [kSkTickets]
  ProfClass prof;
  std::vector<WeightEntry> weights;  // weight_table(&d), each entry bound to its place in the arena
  std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;  // captured decode steps
  // Every device allocation of the stage, made at init or by the first call that needs it; the fields above and below
  // point into them.  free_stage and bs_stage_info walk this list.
  std::vector<OwnedAlloc> owned;
  float* logit_buf = nullptr;       // host-I/O logits staging
  size_t logit_cap = 0;
  // tail token pick (bs_set_sampling): top_k <= 1 greedy, else seeded top-k sampling
  int top_k = 1;
  float temperature = 1.f;
  uint64_t sample_seed = 0;
  float* sample_logits = nullptr;   // [max_batch][V] logits the sampler reads (device I/O without logits)
  // bs_set_graphs: decode steps on device buffers replay captured graphs.  Initial value: 1, or 0 when BS_GRAPHS=0 is
  // set (rocprofv3 --pmc runs: rocprofiler-sdk's counter-collection dispatch interception faulted on graph-launched
  // kernels)
  int graphs_on = graphs_default();
  // greedy lm_head screening (kernels.hip "Greedy lm_head screening"): the int8 shadow copy of the tied embedding,
  // its bound constants and the per-step buffers, one allocation made at init (hs.Q null: none, screening stays off)
  HeadScreen hs{};
  int hs_on = 0;         // bs_set_head_screen; starts on where the shadow copy exists (and BS_HEAD_SCREEN is not 0)
  int hs_last_rows = 0;  // rows of the last forward if its tail ran screened, else 0 (bs_read_head_screen)
  int cus = 0;           // CUs of the device (grids of the screened tail and of the scoring head)
  // bs_forward_score (head_score.hip): the per-split partials of the scoring head and the host-I/O staging of
  // targets / top_ids / scores, one allocation made by the first scoring call (sc_parts null: the stage never scored)
  void* sc_parts = nullptr;
  int* sc_targets = nullptr;  // [max_tokens]
  int* sc_top = nullptr;      // [max_tokens]
  float* sc_scores = nullptr; // [max_tokens][3]
  // BS_STEP_VERIFY (attn_verify.hip): the short-query attention's split partials for kVerifyMaxTokens positions, the
  // tail's argmax keys and ids of every position, one allocation made by the first verify call (vf_acc null: never)
  float* vf_acc = nullptr;             // [kVerifyMaxTokens][n_head][vf_stride][hd]
  float* vf_ml = nullptr;              // [kVerifyMaxTokens][n_head][vf_stride][2]
  int vf_stride = 0;                   // attention_verify_split_stride
  unsigned long long* vf_keys = nullptr;  // [kVerifyMaxTokens][V/16] (last stage)
  int* vf_tok = nullptr;               // [kVerifyMaxTokens] host-I/O staging of the ids
  // per-row sampling (row_sample.hip): the device table, histograms and read-outs, one allocation made by the first
  // bs_set_row_sampler / bs_sample_logits (rs.table null: never used); rs_host mirrors the table for routing
  RowSampleBufs rs{};
  std::vector<RowSamplerDev> rs_host;  // [max_batch]
  int rs_active = 0;                   // rows that hold state
  // per-row logit processors (logit_proc.hip): the device table and the rows' token state, one allocation made by the
  // first bs_set_row_processor / bs_process_logits (lp.table null: never used); lp_host mirrors what routing and the
  // argument checks need: does the row hold state, and how long its history is (an upper bound of the device's)
  LogitProcBufs lp{};
  struct RowProcHost { int active = 0, len = 0; };
  std::vector<RowProcHost> lp_host;  // [max_batch]
  int lp_active = 0;                 // rows that hold state
  // guided decoding (guide.hip): the device table of kGuideMax guide descriptors and the rows' guide state, one
  // allocation made by the first bs_load_guide (gd.guides null: never used); each loaded guide's arrays are one more
  // allocation, counted as workspace until it is unloaded.  gd_host mirrors the rows' guide ids for routing and for
  // the reference counts that keep a guide in use from being unloaded
  GuideBufs gd{};
  struct GuideHost { void* base = nullptr; int n_states = 0, start = 0, refs = 0; };
  GuideHost gd_guides[kGuideMax];
  std::vector<int> gd_host;  // [max_batch] guide id, -1: none
  int gd_active = 0;         // rows that hold state
  // BS_STEP_VERIFY_DRAW: the sampler scratch of kVerifyMaxTokens positions (vd, made by the first verify-draw pass
  // that runs the sampler) and the [max(max_batch, kVerifyMaxTokens)][V] logits its tail reads when the caller
  // gives no device logits (vd_logits, made by the first such pass); vd_last_*: the shape of the last such pass
  RowSampleBufs vd{};
  float* vd_logits = nullptr;
  int vd_last_slot = 0, vd_last_B = 0, vd_last_S = 0;  // B == 0: no verify-draw pass ran
  // bs_forward_topk (beam_topk.hip): the per-(row, slice) partials and the host-I/O staging of ids / logprobs / lse,
  // one allocation made by the first call (tk_pmax null: never)
  float* tk_pmax = nullptr;             // [max_batch][topk_slices(V)]
  float* tk_psum = nullptr;             // [max_batch][topk_slices(V)]
  unsigned long long* tk_pkeys = nullptr;  // [max_batch][topk_slices(V)][kTopkMaxK]
  int* tk_ids = nullptr;                // [max_batch][kTopkMaxK]
  float* tk_lp = nullptr;               // [max_batch][kTopkMaxK]
  float* tk_lse = nullptr;              // [max_batch]
};

// What a scoring pass (bs_forward_score) reads and writes instead of bs_forward's out / logits.
struct ScoreIO {
  const int32_t* targets;
  int32_t* top_ids;
  float* scores;
};

// What a top-k pass (bs_forward_topk) writes instead of bs_forward's out; logits null: none are returned.
struct TopkIO {
  int k;
  int32_t* ids;
  float* logprobs;
  float* lse;
  float* logits;
};

// Allocate `bytes` into the list the stage owns (freed with the stage), counted as workspace or not.
static bool owned_alloc(bs_stage* s, size_t bytes, bool counted, void** out) {
  if (hipMalloc(out, bytes) != hipSuccess) {
    *out = nullptr;
    return false;
  }
  s->owned.push_back({*out, counted ? bytes : 0});
  return true;
}

// ALiBi slopes, build_alibi_tensor (modeling_bloom.py:60-78).
static void alibi_slopes(int n_head, float* out) {
  int cp2 = 1;
  while (cp2 * 2 <= n_head) cp2 *= 2;
  const float basef = (float)std::pow(2.0, -std::pow(2.0, -(std::log2((double)cp2) - 3.0)));
  for (int i = 0; i < cp2; i++) out[i] = (float)std::pow((double)basef, (double)(i + 1));
  if (cp2 != n_head) {
    const float ebf = (float)std::pow(2.0, -std::pow(2.0, -(std::log2((double)(2 * cp2)) - 3.0)));
    const int rem = std::min(n_head - cp2, cp2);
    for (int i = 0; i < rem; i++) out[cp2 + i] = (float)std::pow((double)ebf, (double)(2 * i + 1));
  }
}

static int validate(const bs_stage_desc* d, bool from_file = false) {
  if (!d) return fail(BS_ERR_INVALID, "desc is NULL");
  if (d->hidden <= 0 || d->n_head <= 0 || d->hidden % d->n_head)
    return fail(BS_ERR_INVALID, "hidden must be a positive multiple of n_head");
  if (d->flags & BS_FLAG_MXFP4_WEIGHTS) {  // before the general width check: its own status codes
    if (d->flags & BS_FLAG_INT8_WEIGHTS)
      return fail(BS_ERR_INVALID, "BS_FLAG_MXFP4_WEIGHTS and BS_FLAG_INT8_WEIGHTS exclude each other");
    if (d->dtype != BS_DT_BFLOAT16) return fail(BS_ERR_UNSUPPORTED, "BS_FLAG_MXFP4_WEIGHTS needs dtype BFLOAT16");
    if (d->hidden % 32)
      return fail(BS_ERR_UNSUPPORTED, "BS_FLAG_MXFP4_WEIGHTS needs hidden to be a multiple of 32 (the MX block)");
  }
  if (d->hidden % 32) return fail(BS_ERR_INVALID, "hidden must be a multiple of 32");
  const int hd = d->hidden / d->n_head;
  if (hd % 8 || hd > 128) return fail(BS_ERR_INVALID, "head_dim must be a multiple of 8 and <= 128");
  if (d->n_layer <= 0 || d->layer_begin < 0 || d->layer_end > d->n_layer || d->layer_begin > d->layer_end)
    return fail(BS_ERR_INVALID, "bad layer range");
  if (d->vocab <= 0 || d->vocab % 16) return fail(BS_ERR_INVALID, "vocab must be a positive multiple of 16");
  if (d->dtype != BS_DT_BFLOAT16 && d->dtype != BS_DT_FLOAT) return fail(BS_ERR_INVALID, "dtype must be BFLOAT16 or FLOAT");
  if (d->max_batch <= 0 || d->max_ctx <= 0) return fail(BS_ERR_INVALID, "max_batch/max_ctx must be positive");
  if (!(d->ln_eps > 0.f)) return fail(BS_ERR_INVALID, "ln_eps must be positive");
  if (d->head_vocab_begin < 0 || d->head_vocab_end < d->head_vocab_begin || d->head_vocab_end > d->vocab ||
      d->head_vocab_begin % 16 || d->head_vocab_end % 16)
    return fail(BS_ERR_INVALID, "head vocab slice must be a 16-aligned sub-range of [0, vocab)");
  if (!from_file && d->weight_source != BS_WEIGHTS_SYNTHETIC && d->weight_source != BS_WEIGHTS_HOST)
    return fail(BS_ERR_INVALID, "unknown weight_source");
  if (d->flags & ~(BS_FLAG_INT8_WEIGHTS | BS_FLAG_CLASSIFIER | BS_FLAG_INT8_KV | BS_FLAG_MXFP4_WEIGHTS))
    return fail(BS_ERR_INVALID, "unknown desc flags");
  if ((d->flags & BS_FLAG_INT8_KV) && d->dtype != BS_DT_BFLOAT16)
    return fail(BS_ERR_INVALID, "BS_FLAG_INT8_KV needs dtype BFLOAT16");
  if ((d->flags & BS_FLAG_INT8_KV) && hd % 16)
    return fail(BS_ERR_UNSUPPORTED, "BS_FLAG_INT8_KV needs head_dim to be a multiple of 16");
  if (d->flags & BS_FLAG_CLASSIFIER) {
    if (!d->is_last) return fail(BS_ERR_INVALID, "BS_FLAG_CLASSIFIER needs the last stage");
    if (d->n_labels < 1 || d->n_labels > 64) return fail(BS_ERR_INVALID, "n_labels must be in [1, 64]");
    if (has_head_slice(d)) return fail(BS_ERR_INVALID, "a classifier stage takes no head slice");
  }
  if ((d->flags & BS_FLAG_INT8_WEIGHTS) && d->dtype != BS_DT_BFLOAT16)
    return fail(BS_ERR_UNSUPPORTED, "BS_FLAG_INT8_WEIGHTS needs dtype BFLOAT16");
  return BS_OK;
}

extern "C" uint64_t bs_stage_weight_count(const bs_stage_desc* d) {
  if (validate(d) != BS_OK) return 0;
  uint64_t n = 0;
  for (const WeightEntry& w : weight_table(d)) n += w.count;
  return n;
}

extern "C" int bs_abi_version(void) { return BS_ABI_VERSION; }

#ifndef BS_BUILD_ID
#define BS_BUILD_ID "unstamped"
#endif
extern "C" const char* bs_build_id(void) { return BS_BUILD_ID; }

static uint32_t host_lb32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

extern "C" int bs_prompt_ids(uint64_t seed, int32_t n, int32_t vocab, int32_t* out) {
  if (n < 0 || vocab <= 0 || (n && !out)) return fail(BS_ERR_INVALID, "bad prompt_ids arguments");
  const uint64_t key = tensor_key(seed, -1, 255);
  for (int32_t i = 0; i < n; i++)
    out[i] = (int32_t)(host_lb32((uint32_t)key ^ host_lb32((uint32_t)i + (uint32_t)(key >> 32))) % (uint32_t)vocab);
  return BS_OK;
}
extern "C" const char* bs_last_error(void) { return g_err.c_str(); }

static void free_stage(bs_stage* s) {
  if (!s) return;
  hipSetDevice(s->d.device);
  if (s->own) hipStreamSynchronize(s->own);
  for (auto e : s->prof.ev) hipEventDestroy(e);
  for (auto& g : s->graphs) hipGraphExecDestroy(g.second);
  for (const OwnedAlloc& a : s->owned) hipFree(a.p);
  if (s->own) hipStreamDestroy(s->own);
  delete s;
}

// The checkpoint tensor of a weight-table entry, present, shaped right and of a loadable type (else null and why).
static const st::Tensor* find_entry(const st::Checkpoint& ck, const WeightEntry& fe, std::string* why) {
  const st::Tensor* t = ck.find(fe.name);
  if (!t && fe.name == "word_embeddings.weight") t = ck.find("lm_head.weight");  // tied head saved alone
  if (!t) { *why = "checkpoint has no tensor '" + fe.name + "'"; return nullptr; }
  if (t->shape != fe.shape) {
    std::string a, b;
    for (auto v : t->shape) a += std::to_string(v) + ",";
    for (auto v : fe.shape) b += std::to_string(v) + ",";
    *why = "tensor '" + fe.name + "' has shape [" + a + "] but the stage needs [" + b + "]";
    return nullptr;
  }
  if (t->dtype == st::OTHER) { *why = "tensor '" + fe.name + "' has dtype " + t->dtype_name + " (need F32/F16/BF16)"; return nullptr; }
  return t;
}

static float host_f16(uint16_t v) {
  const uint32_t sgn = (uint32_t)(v >> 15) << 31, ex = (v >> 10) & 31, man = v & 1023;
  uint32_t bits;
  if (ex == 31) bits = sgn | 0x7F800000u | (man << 13);
  else if (ex) bits = sgn | ((ex + 112) << 23) | (man << 13);
  else if (!man) bits = sgn;
  else {  // subnormal: exact in fp32
    float f = (float)man * 5.9604644775390625e-8f;  // 2^-24
    std::memcpy(&bits, &f, 4);
    bits |= sgn;
  }
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

static int init_stage(const bs_stage_desc* desc, bs_stage** out, const st::Checkpoint* ck);

extern "C" int bs_init_stage(const bs_stage_desc* desc, bs_stage** out) { return init_stage(desc, out, nullptr); }

extern "C" int bs_init_stage_file(const bs_stage_desc* desc, const char* path, bs_stage** out) {
  if (!out) return fail(BS_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!path) return fail(BS_ERR_INVALID, "path is NULL");
  int rc = validate(desc, true);
  if (rc) return rc;
  st::Checkpoint ck;
  std::string err;
  if (!ck.open(path, &err)) return fail(BS_ERR_INVALID, err);
  for (const WeightEntry& fe : weight_table(desc))  // every tensor present and shaped right before any allocation
    if (!find_entry(ck, fe, &err)) return fail(BS_ERR_INVALID, err);
  return init_stage(desc, out, &ck);
}

extern "C" int bs_weights_file_probe(const char* path, int32_t* hidden, int32_t* n_layer, int32_t* vocab) {
  if (!path) return fail(BS_ERR_INVALID, "path is NULL");
  st::Checkpoint ck;
  std::string err;
  if (!ck.open(path, &err)) return fail(BS_ERR_INVALID, err);
  const st::Tensor* e = ck.find("word_embeddings.weight");
  if (!e) e = ck.find("lm_head.weight");
  int32_t hid = -1, nl = 0, V = -1;
  if (e && e->shape.size() == 2) { V = (int32_t)e->shape[0]; hid = (int32_t)e->shape[1]; }
  for (const auto& kv : ck.tensors()) {  // layers: 1 + the highest h.<i>. present
    const std::string& n = kv.first;
    auto ends = [&](const std::string& x) { return n.size() >= x.size() && !n.compare(n.size() - x.size(), x.size(), x); };
    if (hid < 0 && (ends("layernorm.weight") || ends("ln_f.weight")) && kv.second.shape.size() == 1)
      hid = (int32_t)kv.second.shape[0];  // any LayerNorm gives the width
    size_t p = n.rfind("h.", 0) == 0 ? 2 : (n.rfind("transformer.h.", 0) == 0 ? 14 : std::string::npos);
    if (p == std::string::npos) continue;
    long i = 0;
    size_t q = p;
    while (q < n.size() && n[q] >= '0' && n[q] <= '9' && i < 1000000) i = i * 10 + (n[q++] - '0');
    if (q > p && q < n.size() && n[q] == '.') nl = std::max(nl, (int32_t)i + 1);
  }
  if (hidden) *hidden = hid;
  if (n_layer) *n_layer = nl;
  if (vocab) *vocab = V;
  return BS_OK;
}

static int init_stage(const bs_stage_desc* desc, bs_stage** out, const st::Checkpoint* ck) {
  if (!out) return fail(BS_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int rc = validate(desc, ck != nullptr);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (desc->device < 0 || desc->device >= ndev) return fail(BS_ERR_INVALID, "device ordinal out of range");
  HIP_TRY(hipSetDevice(desc->device));

  bs_stage* s = new bs_stage();
  s->d = *desc;
  if (s->d.max_tokens <= 0) s->d.max_tokens = s->d.max_batch * 128;
  s->bf16 = desc->dtype == BS_DT_BFLOAT16;
  s->q8 = (desc->flags & BS_FLAG_INT8_WEIGHTS) != 0;
  s->mx4 = (desc->flags & BS_FLAG_MXFP4_WEIGHTS) != 0;
  s->kv8 = (desc->flags & BS_FLAG_INT8_KV) != 0;
  s->esz = s->bf16 ? 2 : 4;
  s->n_labels = (desc->flags & BS_FLAG_CLASSIFIER) ? desc->n_labels : 0;
  s->hd = desc->hidden / desc->n_head;
  s->L = desc->layer_end - desc->layer_begin;
  const size_t h = desc->hidden, V = desc->vocab, T = s->d.max_tokens;

  auto cleanup = [&](int code) { free_stage(s); return code; };
#define INIT_TRY(expr)  /* HIP_TRY that frees the half-built stage */                                        \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return cleanup(fail(BS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_))); \
  } while (0)
  if (hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(BS_ERR_DEVICE, "hipStreamCreate failed"));

  // ---- weight arena: every tensor 256-B aligned, in table order; a quantised matrix is its codes, then its scales
  s->weights = weight_table(desc);
  Carver wa;
  for (WeightEntry& w : s->weights) {
    if (w.N && s->q8) {
      wa.piece(&w.data, w.count);               // int8 [N][K]
      wa.piece(&w.row_scale, (size_t)w.N * 4);  // fp32 scale [N]
    } else if (w.N && s->mx4) {
      wa.piece(&w.data, w.count / 2);           // E2M1 codes, 16-B block records
      wa.piece(&w.blk_scale, w.count / 32);     // E8M0 scale [N][K / 32]
    } else {
      wa.piece(&w.data, w.count * s->esz);
    }
  }
  s->wbytes = wa.total;
  if (wa.alloc() != Carver::OK)
    return cleanup(fail(BS_ERR_OOM, "weight allocation failed (" + std::to_string(s->wbytes) + " B)"));
  s->owned.push_back({wa.base, 0});
  s->layers.assign(s->L, Layer{});
  void** const model_slot[] = {&s->wemb, &s->emb_g, &s->emb_b, &s->lnf_g, &s->lnf_b, &s->score, &s->hw};  // by M_*
  for (const WeightEntry& w : s->weights) {
    if (w.layer < 0) {
      *model_slot[w.tid] = w.data;
    } else {
      Layer& ly = s->layers[w.layer];
      ly.t[w.tid] = w.data; ly.sc[w.tid] = w.row_scale; ly.mxs[w.tid] = w.blk_scale;
    }
  }
  s->hv0 = desc->head_vocab_begin;
  s->hv1 = desc->head_vocab_end;
  if (has_head_slice(desc)) {
    if (s->wemb) s->hw = (char*)s->wemb + (size_t)s->hv0 * h * s->esz;  // else its own tensor (M_HEAD)
  } else if (desc->is_last && !s->n_labels) {
    s->hw = s->wemb; s->hv0 = 0; s->hv1 = desc->vocab;  // the last stage's full head
  }
  if ((s->q8 || s->mx4) && !owned_alloc(s, 4 * h * h * 2, false, &s->wtmp))
    return cleanup(fail(BS_ERR_OOM, std::string(s->q8 ? "int8" : "MXFP4") + " staging allocation failed"));
  // int8 / MXFP4 matrices are produced in bf16 in the staging buffer, then quantized into the arena
  auto target = [&](const WeightEntry& w) { return (char*)(w.quantised() ? s->wtmp : w.data); };
  auto quantize = [&](const WeightEntry& w) {
    if (w.blk_scale) launch_quantize_mx4(s->wtmp, (uint8_t*)w.data, w.blk_scale, w.N, w.K, s->own);
    else if (w.row_scale) launch_quantize_rows(s->wtmp, (int8_t*)w.data, w.row_scale, w.N, w.K, s->own);
  };

  // ---- weights: the three sources walk the table
  const size_t chunk = 16u << 20;
  // fp32 chunks on their way to the stage's type (file and host sources), freed on every path
  struct Bounce { float* p = nullptr; ~Bounce() { hipFree(p); } } bounce;
  auto upload_f32 = [&](char* dst, const float* src, size_t n) {
    if (hipMemcpyAsync(bounce.p, src, n * sizeof(float), hipMemcpyHostToDevice, s->own) != hipSuccess) return false;
    launch_convert_f32(dst, s->bf16, bounce.p, n, s->own);
    return true;
  };
  if (ck) {
    // Straight from the file mapping: matching dtypes are copied as they are, others widen to fp32 on
    // the host (exact) and take the BS_WEIGHTS_HOST conversion, so a file of fp32 weights loads
    // bit-identical to the same weights passed as a host buffer.
    std::vector<float> wide(chunk);
    if (hipMalloc(&bounce.p, chunk * sizeof(float)) != hipSuccess) return cleanup(fail(BS_ERR_OOM, "bounce alloc"));
    std::string why;
    for (const WeightEntry& w : s->weights) {
      const st::Tensor* t = find_entry(*ck, w, &why);
      if (!t || w.first + w.count > t->numel())
        return cleanup(fail(BS_ERR_INVALID, t ? "head slice outside the checkpoint's embedding" : why));
      const bool same = (s->bf16 && t->dtype == st::BF16) || (!s->bf16 && t->dtype == st::F32);
      const size_t tes = t->dtype == st::F32 ? 4 : 2;
      const uint8_t* src = t->data + w.first * tes;
      bool ok = true;
      if (same) {
        ok = hipMemcpyAsync(target(w), src, w.count * s->esz, hipMemcpyHostToDevice, s->own) == hipSuccess;
      } else {
        for (size_t i = 0; ok && i < w.count; i += chunk) {
          const size_t n = std::min<size_t>(chunk, w.count - i);
          const uint8_t* p = src + i * tes;
          if (t->dtype == st::F32) {
            std::memcpy(wide.data(), p, n * 4);
          } else {
            for (size_t j = 0; j < n; j++) {
              uint16_t v;
              std::memcpy(&v, p + 2 * j, 2);
              if (t->dtype == st::BF16) {
                const uint32_t b = (uint32_t)v << 16;
                std::memcpy(&wide[j], &b, 4);
              } else {
                wide[j] = host_f16(v);
              }
            }
          }
          ok = upload_f32(target(w) + i * s->esz, wide.data(), n) &&
               hipStreamSynchronize(s->own) == hipSuccess;  // `wide` is refilled next round
        }
      }
      if (!ok) return cleanup(fail(BS_ERR_DEVICE, "weight upload failed"));
      quantize(w);
    }
    if (hipStreamSynchronize(s->own) != hipSuccess)  // the mapping goes away after init
      return cleanup(fail(BS_ERR_DEVICE, "weight upload failed"));
  } else if (desc->weight_source == BS_WEIGHTS_SYNTHETIC) {
    for (const WeightEntry& w : s->weights) {
      launch_gen_fill(target(w), s->bf16, w.count, w.key, w.kind, s->own, w.first);
      quantize(w);
    }
  } else {
    const uint64_t need = bs_stage_weight_count(desc);
    if (!desc->host_weights || desc->host_weight_count != need)
      return cleanup(fail(BS_ERR_INVALID, "host_weights count mismatch: need " + std::to_string(need)));
    // canonical order == arena order; upload through an fp32 bounce buffer
    if (hipMalloc(&bounce.p, chunk * sizeof(float)) != hipSuccess) return cleanup(fail(BS_ERR_OOM, "bounce alloc"));
    const float* src = desc->host_weights;
    for (const WeightEntry& w : s->weights) {
      for (size_t i = 0; i < w.count; i += chunk)
        if (!upload_f32(target(w) + i * s->esz, src + i, std::min<size_t>(chunk, w.count - i)))
          return cleanup(fail(BS_ERR_DEVICE, "weight upload failed"));
      quantize(w);
      src += w.count;
    }
    hipStreamSynchronize(s->own);
  }

  // ---- greedy lm_head screening: int8 shadow copy of the resident bf16 embedding (the BS_FLAG_INT8_WEIGHTS rule),
  // one bound constant per row, and the per-step buffers for up to 2 rows.  A failed allocation leaves it off.
  if (s->bf16 && desc->is_last && !s->n_labels && s->wemb && head_screen_supported(1, (int)h) &&
      hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, desc->device) == hipSuccess && s->cus > 0) {
    const size_t nt = V / 16, mb = std::min<size_t>(desc->max_batch, 2);
    int8_t* Qh = nullptr;
    float *sch = nullptr, *cbh = nullptr;
    Carver c;
    c.piece(&Qh, V * h);
    c.piece(&sch, V * 4);
    c.piece(&cbh, V * 4);
    c.piece(&s->hs.hilo, mb * nt * 8);
    c.piece(&s->hs.rnorm, mb * 4);
    c.piece(&s->hs.lstar, mb * 4);
    c.piece(&s->hs.list, mb * nt * 4);
    c.piece(&s->hs.count, mb * 4);
    if (c.alloc() == Carver::OK) {
      s->owned.push_back({c.base, c.total});
      s->hs.Q = Qh; s->hs.scale = sch; s->hs.cb = cbh;
      if (hipMemsetAsync(s->hs.hilo, 0, c.base + c.total - (char*)s->hs.hilo, s->own) != hipSuccess)  // the per-step buffers
        return cleanup(fail(BS_ERR_DEVICE, "head screen memset"));
      launch_quantize_rows(s->wemb, Qh, sch, (int)V, (int)h, s->own);
      launch_head_bound(s->wemb, Qh, sch, cbh, (int)V, (int)h, s->own);
      s->hs_on = head_screen_default();
    } else {
      (void)hipGetLastError();  // not an init failure
    }
  }

  // ---- KV cache
  s->kv_half = (size_t)desc->max_batch * desc->n_head * desc->max_ctx * s->hd * (s->kv8 ? 1 : s->esz);
  s->kv_layer_stride = 2 * s->kv_half;
  s->kvbytes = s->kv_layer_stride * (s->L > 0 ? s->L : 0);
  if (s->kv8) {  // the scales follow the codes (16-B aligned: head_dim % 16 == 0)
    s->kv_sc_half = (size_t)desc->max_batch * desc->n_head * desc->max_ctx;
    s->kvbytes += 2 * s->kv_sc_half * 4 * (s->L > 0 ? s->L : 0);
  }
  if (s->kvbytes) {
    if (!owned_alloc(s, s->kvbytes, false, (void**)&s->kv))
      return cleanup(fail(BS_ERR_OOM, "KV cache allocation failed (" + std::to_string(s->kvbytes) + " B)"));
    if (hipMemsetAsync(s->kv, 0, s->kvbytes, s->own) != hipSuccess) return cleanup(fail(BS_ERR_DEVICE, "kv memset"));
    if (s->kv8) s->kv_scales = (float*)(s->kv + s->kv_layer_stride * s->L);
  }
  if (s->kv8 && s->L > 0) {  // bf16 staging of a call's new K / V rows (and, for S > 1, the dequantised past)
    s->kv_stage_cap = std::max<size_t>(T, desc->max_ctx);
    const size_t sb = 2 * s->kv_stage_cap * h * 2;
    if (!owned_alloc(s, sb, true, (void**)&s->kv_stage))
      return cleanup(fail(BS_ERR_OOM, "KV staging allocation failed (" + std::to_string(sb) + " B)"));
    if (hipMemsetAsync(s->kv_stage, 0, sb, s->own) != hipSuccess) return cleanup(fail(BS_ERR_DEVICE, "kv staging memset"));
  }

  // ---- workspace
  const size_t attn_f = attention_workspace_floats(desc->max_batch, desc->n_head, s->hd, desc->max_ctx, &s->max_chunks,
                                                   &s->chunk);
  Carver wc;
  wc.piece(&s->xa, T * h * 4);
  wc.piece(&s->xb, T * h * 4);
  wc.piece(&s->attn, T * h * 4);
  wc.piece(&s->q, T * h * 4);
  wc.piece(&s->xn, T * h * s->esz);
  wc.piece(&s->ctx, T * h * s->esz);
  wc.piece(&s->g, T * 4 * h * s->esz);
  wc.piece(&s->part_acc, attn_f * 4);  // part_ml follows
  wc.piece(&s->slopes, desc->n_head * 4);
  wc.piece(&s->keys, (size_t)desc->max_batch * (V / 16) * 8);
  wc.piece(&s->tok, (size_t)desc->max_batch * 4);
  wc.piece(&s->ids, T * 4);
  wc.piece(&s->past_dev, (size_t)desc->max_batch * 4);                     // per-row past_len (device copy)
  wc.piece(&s->att_tickets, (size_t)desc->max_batch * desc->n_head * 4);   // attention split-merge tickets
  wc.piece(&s->sk_ws, kSkCap * 4);                                         // batched-GEMV split-K partials
  wc.piece(&s->sk_tickets, kSkTickets * 4);                                // and their tickets
  s->wsbytes = wc.total;
  if (wc.alloc() != Carver::OK) return cleanup(fail(BS_ERR_OOM, "workspace allocation failed"));
  s->owned.push_back({wc.base, 0});
  s->ws = wc.base;
  s->part_ml = s->part_acc + (size_t)desc->max_batch * desc->n_head * s->max_chunks * s->hd;
  std::vector<float> sl(desc->n_head);
  alibi_slopes(desc->n_head, sl.data());
  INIT_TRY(hipMemsetAsync(s->ws, 0, s->wsbytes, s->own));
  INIT_TRY(hipMemcpyAsync(s->slopes, sl.data(), sl.size() * 4, hipMemcpyHostToDevice, s->own));
  hipError_t e = hipStreamSynchronize(s->own);
  if (e != hipSuccess) return cleanup(fail(BS_ERR_DEVICE, std::string("init sync: ") + hipGetErrorString(e)));
  e = hipGetLastError();
  if (e != hipSuccess) return cleanup(fail(BS_ERR_DEVICE, std::string("init kernels: ") + hipGetErrorString(e)));
  *out = s;
  return BS_OK;
#undef INIT_TRY
}

extern "C" void bs_release(bs_stage* s) { free_stage(s); }

extern "C" int bs_stage_info(const bs_stage* s, bs_stage_desc* d, uint64_t* wb, uint64_t* kvb, uint64_t* wsb) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (d) *d = s->d;
  if (wb) *wb = s->wbytes;
  if (kvb) *kvb = s->kvbytes;
  // the head-screening shadow copy, the int8 KV staging, the scoring, verify and sampler buffers count as workspace
  if (wsb) {
    *wsb = s->wsbytes;
    for (const OwnedAlloc& a : s->owned) *wsb += a.counted;
  }
  return BS_OK;
}

extern "C" int bs_read_weights(const bs_stage* s, uint64_t offset, uint64_t count, float* out) {
  if (!s || (count && !out)) return fail(BS_ERR_INVALID, "stage/out is NULL");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipStreamSynchronize(s->own));
  uint64_t base = 0, done = 0;
  std::vector<uint16_t> tmp;
  std::vector<int8_t> qtmp;
  std::vector<float> stmp;
  std::vector<uint8_t> ctmp, etmp;
  for (const WeightEntry& w : s->weights) {
    const uint64_t b = base, e = base + w.count;
    base = e;
    if (e <= offset || b >= offset + count) continue;
    const uint64_t lo = std::max<uint64_t>(b, offset), hi = std::min<uint64_t>(e, offset + count);
    const uint64_t n = hi - lo;
    const char* src = (const char*)w.data + (lo - b) * s->esz;
    float* dst = out + (lo - offset);
    const int K = w.K;
    if (w.blk_scale) {  // MXFP4 matrix: +-grid[code] * 2^(E - 127), codes in rotated block records
      const int nb = K / 32;
      const uint64_t b0 = (lo - b) / 32, b1 = (hi - b - 1) / 32;  // blocks of the matrix, row-major
      ctmp.resize((b1 - b0 + 1) * 16);
      etmp.resize(b1 - b0 + 1);
      HIP_TRY(hipMemcpy(ctmp.data(), (const uint8_t*)w.data + b0 * 16, ctmp.size(), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(etmp.data(), w.blk_scale + b0, etmp.size(), hipMemcpyDeviceToHost));
      static const float grid[16] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f, -0.f, -0.5f, -1.f, -1.5f, -2.f, -3.f, -4.f, -6.f};
      for (uint64_t blk = b0; blk <= b1; blk++) {
        const float X = std::ldexp(1.0f, (int)etmp[blk - b0] - 127);
        const uint8_t* rec = &ctmp[(blk - b0) * 16];
        const int rot = (int)((blk % nb) >> 2);
        float v[32];
        for (int g = 0; g < 4; g++) {
          const uint8_t* dw = rec + 4 * ((g - rot) & 3);
          for (int j = 0; j < 4; j++) {
            v[8 * g + 2 * j] = grid[dw[j] & 15] * X;
            v[8 * g + 2 * j + 1] = grid[dw[j] >> 4] * X;
          }
        }
        const uint64_t k0 = std::max<uint64_t>(blk * 32, lo - b), k1 = std::min<uint64_t>(blk * 32 + 32, hi - b);
        for (uint64_t k = k0; k < k1; k++) dst[k - (lo - b)] = v[k - blk * 32];
      }
    } else if (w.row_scale) {  // int8 matrix: dequantized values Q * scale
      const uint64_t r0 = (lo - b) / K, r1 = (hi - b - 1) / K;
      qtmp.resize(n);
      stmp.resize(r1 - r0 + 1);
      HIP_TRY(hipMemcpy(qtmp.data(), (const int8_t*)w.data + (lo - b), n, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(stmp.data(), w.row_scale + r0, stmp.size() * 4, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; i++) dst[i] = (float)qtmp[i] * stmp[(lo - b + i) / K - r0];
    } else if (s->bf16) {
      tmp.resize(n);
      HIP_TRY(hipMemcpy(tmp.data(), src, n * 2, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; i++) {
        uint32_t u = (uint32_t)tmp[i] << 16;
        std::memcpy(&dst[i], &u, 4);
      }
    } else {
      HIP_TRY(hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToHost));
    }
    done += n;
  }
  if (done != count) return fail(BS_ERR_INVALID, "read range outside the stage weights");
  return BS_OK;
}

extern "C" int bs_read_kv(const bs_stage* s, int32_t layer, int32_t slot, int32_t pos0, int32_t npos, float* out) {
  if (!s || !out) return fail(BS_ERR_INVALID, "stage/out is NULL");
  if (layer < 0 || layer >= s->L) return fail(BS_ERR_INVALID, "layer outside the stage");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (pos0 < 0 || npos < 0 || pos0 + npos > s->d.max_ctx) return fail(BS_ERR_INVALID, "positions outside max_ctx");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipStreamSynchronize(s->own));
  const int nh = s->d.n_head, hd = s->hd;
  const size_t run = (size_t)npos * hd;  // contiguous elements of one (K|V, head)
  std::vector<uint16_t> tmp(s->bf16 && !s->kv8 ? run : 0);
  std::vector<int8_t> qtmp(s->kv8 ? run : 0);
  std::vector<float> stmp(s->kv8 ? npos : 0);
  for (int w = 0; w < 2; w++)
    for (int hh = 0; hh < nh; hh++) {
      const size_t e0 = (((size_t)slot * nh + hh) * s->d.max_ctx + pos0) * hd;
      if (s->kv8) {  // dequantised values: (float)q * scale
        float* dq = out + ((size_t)w * nh + hh) * run;
        if (!run) continue;
        HIP_TRY(hipMemcpy(qtmp.data(), s->kv + layer * s->kv_layer_stride + w * s->kv_half + e0, run,
                          hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(stmp.data(), s->kv_scales + ((size_t)layer * 2 + w) * s->kv_sc_half + e0 / hd,
                          (size_t)npos * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < run; i++) dq[i] = (float)qtmp[i] * stmp[i / hd];
        continue;
      }
      const char* src = s->kv + layer * s->kv_layer_stride + w * s->kv_half + e0 * s->esz;
      float* dst = out + ((size_t)w * nh + hh) * run;
      if (s->bf16) {
        HIP_TRY(hipMemcpy(tmp.data(), src, run * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < run; i++) {
          const uint32_t u = (uint32_t)tmp[i] << 16;
          std::memcpy(&dst[i], &u, 4);
        }
      } else {
        HIP_TRY(hipMemcpy(dst, src, run * 4, hipMemcpyDeviceToHost));
      }
    }
  return BS_OK;
}

extern "C" int bs_reset_kv(bs_stage* s, int32_t slot) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  HIP_TRY(hipSetDevice(s->d.device));
  // Cached positions are addressed by past_len, so forgetting is bookkeeping only; zero the
  // rows anyway so stale data can never be read by a caller that reuses past_len wrongly.
  const size_t row = (size_t)s->d.n_head * s->d.max_ctx * s->hd * (s->kv8 ? 1 : s->esz);
  const size_t srow = (size_t)s->d.n_head * s->d.max_ctx;  // int8 KV: scales of one row
  for (int l = 0; l < s->L; l++)
    for (int w = 0; w < 2; w++) {
      char* base = s->kv + l * s->kv_layer_stride + w * s->kv_half;
      if (slot < 0) HIP_TRY(hipMemsetAsync(base, 0, s->kv_half, s->own));
      else HIP_TRY(hipMemsetAsync(base + (size_t)slot * row, 0, row, s->own));
      if (!s->kv8) continue;
      float* sc = s->kv_scales + ((size_t)l * 2 + w) * s->kv_sc_half;
      if (slot < 0) HIP_TRY(hipMemsetAsync(sc, 0, s->kv_sc_half * 4, s->own));
      else HIP_TRY(hipMemsetAsync(sc + (size_t)slot * srow, 0, srow * 4, s->own));
    }
  HIP_TRY(hipStreamSynchronize(s->own));
  return BS_OK;
}

// KV row fork (kv_fork.hip): one launch for the codes or values of every layer, one more for an int8 cache's scales.
// Enqueues only: no allocation, no synchronisation, no host copy, and the captured graphs stay (a graph's key holds
// no cache content).  past_dev / past_next are indexed by a call's rows and re-written by the next forward whose
// past_lens differ, so they need no update here.
extern "C" int bs_fork_kv(bs_stage* s, int32_t src_slot, int32_t dst_slot, int32_t count, int32_t npos, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  const int mb = s->d.max_batch;
  if (src_slot < 0 || dst_slot < 0 || count < 0 || npos < 0) return fail(BS_ERR_INVALID, "negative slot, count or npos");
  if (src_slot >= mb || dst_slot > mb - count) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (npos > s->d.max_ctx) return fail(BS_ERR_INVALID, "npos beyond max_ctx");
  if (src_slot >= dst_slot && src_slot - dst_slot < count) return fail(BS_ERR_INVALID, "the source row is one of the destination rows");
  if (!count || !npos || s->L <= 0) return BS_OK;
  const size_t pos_bytes = (size_t)s->hd * (s->kv8 ? 1 : s->esz);  // a multiple of 16 (head_dim % 8, % 16 for int8)
  if (!kv_fork_supported(npos, pos_bytes)) return fail(BS_ERR_UNSUPPORTED, "npos * head_dim too large for the fork kernel");
  HIP_TRY(hipSetDevice(s->d.device));
  if (s->cus <= 0 && hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, s->d.device) != hipSuccess) {
    (void)hipGetLastError();
    s->cus = 0;  // the launch falls back to 256
  }
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  launch_kv_fork(s->kv, 16, 2 * s->L, s->d.n_head, mb, s->d.max_ctx, pos_bytes, src_slot, dst_slot, count, npos, s->cus, st);
  if (s->kv8)  // scale segments start on 4-byte boundaries only
    launch_kv_fork(s->kv_scales, 4, 2 * s->L, s->d.n_head, mb, s->d.max_ctx, 4, src_slot, dst_slot, count, npos, s->cus, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("kv fork: ") + hipGetErrorString(err));
  return BS_OK;
}

// KV row pair copy: bs_fork_kv's contract for a list of (source row -> destination row) pairs, as fork launches
// (kv_fork.hip) -- one per run of pairs that share a source and have consecutive destinations (one more each for an
// int8 cache's scales).  A one-launch pair-list variant of the kernel measured slower than the fork launches of the
// same pairs at 5 of 12 points and was dropped.  The no-alias checks leave the launches
// without an ordering hazard among themselves.
extern "C" int bs_copy_kv(bs_stage* s, const int32_t* src_slots, const int32_t* dst_slots, int32_t count, int32_t npos,
                          void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  const int mb = s->d.max_batch;
  if (count < 0 || count > 32) return fail(BS_ERR_INVALID, "count must be in [0, 32]");
  if (count > 0 && (!src_slots || !dst_slots)) return fail(BS_ERR_INVALID, "slot lists are NULL");
  if (npos < 0 || npos > s->d.max_ctx) return fail(BS_ERR_INVALID, "npos outside [0, max_ctx]");
  for (int i = 0; i < count; i++) {
    if (src_slots[i] < 0 || src_slots[i] >= mb || dst_slots[i] < 0 || dst_slots[i] >= mb)
      return fail(BS_ERR_INVALID, "slot outside max_batch");
    for (int j = 0; j < count; j++) {
      if (dst_slots[i] == src_slots[j]) return fail(BS_ERR_INVALID, "a destination row is also a source row");
      if (j < i && dst_slots[i] == dst_slots[j]) return fail(BS_ERR_INVALID, "a destination row appears twice");
    }
  }
  if (!count || !npos || s->L <= 0) return BS_OK;
  const size_t pos_bytes = (size_t)s->hd * (s->kv8 ? 1 : s->esz);  // a multiple of 16 (head_dim % 8, % 16 for int8)
  if (!kv_fork_supported(npos, pos_bytes)) return fail(BS_ERR_UNSUPPORTED, "npos * head_dim too large for the copy kernel");
  HIP_TRY(hipSetDevice(s->d.device));
  if (s->cus <= 0 && hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, s->d.device) != hipSuccess) {
    (void)hipGetLastError();
    s->cus = 0;  // the launch falls back to 256
  }
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  for (int i = 0; i < count;) {
    int n = 1;  // pairs i .. i + n - 1: one source, destinations dst, dst + 1, ...
    while (i + n < count && src_slots[i + n] == src_slots[i] && dst_slots[i + n] == dst_slots[i] + n) n++;
    launch_kv_fork(s->kv, 16, 2 * s->L, s->d.n_head, mb, s->d.max_ctx, pos_bytes, src_slots[i], dst_slots[i], n, npos, s->cus, st);
    if (s->kv8)  // scale segments start on 4-byte boundaries only
      launch_kv_fork(s->kv_scales, 4, 2 * s->L, s->d.n_head, mb, s->d.max_ctx, 4, src_slots[i], dst_slots[i], n, npos, s->cus, st);
    i += n;
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("kv copy: ") + hipGetErrorString(err));
  return BS_OK;
}

// ---- profiling
extern "C" int bs_profile_enable(bs_stage* s, int32_t cls) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  s->prof.cls = cls;
  s->prof.used = 0;
  s->prof.algo = 0.0;
  return BS_OK;
}

static hipEvent_t prof_event(bs_stage* s) {
  if (s->prof.used >= s->prof.ev.size()) {
    // no system-scope fence on the timing markers: a fenced record writes back L2 between the
    // timed kernels and stretches each ~5 us launch by ~2 us against the kernel trace
    hipEvent_t e;
    hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    s->prof.ev.push_back(e);
  }
  return s->prof.ev[s->prof.used++];
}

extern "C" int bs_profile_read(bs_stage* s, double* total_ms, uint64_t* launches, double* algo) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  double tot = 0.0;
  for (size_t i = 0; i + 1 < s->prof.used; i += 2) {
    HIP_TRY(hipEventSynchronize(s->prof.ev[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->prof.ev[i], s->prof.ev[i + 1]));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = s->prof.used / 2;
  if (algo) *algo = s->prof.algo;
  return BS_OK;
}

// s_memrealtime ticks at 100 MHz; the spin is bounded by its argument
__global__ void stream_delay_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

extern "C" int bs_stream_delay(void* stream, int32_t microseconds) {
  if (microseconds < 0 || microseconds > 100000) return fail(BS_ERR_INVALID, "delay must be in [0, 100000] us");
  stream_delay_kernel<<<1, 1, 0, (hipStream_t)stream>>>((long long)microseconds * 100);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BS_ERR_DEVICE, std::string("stream delay: ") + hipGetErrorString(e));
  return BS_OK;
}

// ---- HBM probe (bench.py "hbm_measured"): STREAM-like read and copy rates of this device.
typedef unsigned int probe_u4 __attribute__((ext_vector_type(4)));
// Every thread keeps 8 16-B loads in flight (a 32 KB tile per 256-thread block and step), grid-stride
// over tiles: enough bytes in flight per CU to hide HBM latency at the full rate.
constexpr int kProbeU = 8;
__global__ __launch_bounds__(256) void probe_read_kernel(const probe_u4* __restrict__ p, size_t n, probe_u4* sink) {
  probe_u4 acc = {0u, 0u, 0u, 0u};
  const size_t tile = (size_t)blockDim.x * kProbeU;
  for (size_t t = (size_t)blockIdx.x * tile; t + tile <= n; t += (size_t)gridDim.x * tile) {
    probe_u4 v[kProbeU];
#pragma unroll
    for (int u = 0; u < kProbeU; u++) v[u] = __builtin_nontemporal_load(p + t + u * blockDim.x + threadIdx.x);
#pragma unroll
    for (int u = 0; u < kProbeU; u++) acc ^= v[u];
  }
  if ((acc.x & acc.y & acc.z & acc.w) == 0xFFFFFFFFu) sink[0] = acc;  // never in practice; keeps the loads
}
__global__ __launch_bounds__(256) void probe_copy_kernel(const probe_u4* __restrict__ p, probe_u4* __restrict__ q, size_t n) {
  const size_t tile = (size_t)blockDim.x * kProbeU;
  for (size_t t = (size_t)blockIdx.x * tile; t + tile <= n; t += (size_t)gridDim.x * tile) {
    probe_u4 v[kProbeU];
#pragma unroll
    for (int u = 0; u < kProbeU; u++) v[u] = __builtin_nontemporal_load(p + t + u * blockDim.x + threadIdx.x);
#pragma unroll
    for (int u = 0; u < kProbeU; u++) __builtin_nontemporal_store(v[u], q + t + u * blockDim.x + threadIdx.x);
  }
}

// Probe resources released on every exit path; every HIP call's status is checked.
namespace {
struct ProbeRes {
  void* buf[2] = {nullptr, nullptr};
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~ProbeRes() {
    if (st) hipStreamSynchronize(st);
    for (auto e : ev) if (e) hipEventDestroy(e);
    if (st) hipStreamDestroy(st);
    for (auto b : buf) if (b) hipFree(b);
  }
  int init(size_t bytes, int nbuf) {
    for (int i = 0; i < nbuf; i++)
      if (hipMalloc(&buf[i], bytes) != hipSuccess) return fail(BS_ERR_OOM, "probe allocation failed");
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    return BS_OK;
  }
  // Time one launch (enqueued by `launch`) with the event pair; ms < 0 never escapes (status instead).
  template <typename F>
  int timed(F&& launch, float* ms) {
    HIP_TRY(hipEventRecord(ev[0], st));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipEventSynchronize(ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, ev[0], ev[1]));
    if (!(*ms > 0.f)) return fail(BS_ERR_DEVICE, "probe: non-positive event time");
    return BS_OK;
  }
};
}  // namespace

extern "C" int bs_hbm_probe(int32_t device, uint64_t bytes, double* read_gbps, double* copy_gbps) {
  if (bytes < (1u << 20) || bytes % (1u << 20)) return fail(BS_ERR_INVALID, "probe bytes must be a positive multiple of 1 MiB");
  HIP_TRY(hipSetDevice(device));
  ProbeRes p;
  int rc = p.init(bytes, 2);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(p.buf[0], 1, bytes, p.st));
  const size_t n = bytes / 16;
  const unsigned grid = 256 * 8;  // 8 blocks per CU
  const probe_u4* a = (const probe_u4*)p.buf[0];
  probe_u4* b = (probe_u4*)p.buf[1];
  float best_r = 1e30f, best_c = 1e30f;
  for (int it = 0; it < 12; it++) {
    float ms = 0.f;
    if ((rc = p.timed([&] { probe_read_kernel<<<grid, 256, 0, p.st>>>(a, n, b); }, &ms))) return rc;
    if (it >= 2) best_r = std::min(best_r, ms);
    if ((rc = p.timed([&] { probe_copy_kernel<<<grid, 256, 0, p.st>>>(a, b, n); }, &ms))) return rc;
    if (it >= 2) best_c = std::min(best_c, ms);
  }
  if (read_gbps) *read_gbps = (double)bytes / (best_r * 1e-3) / 1e9;
  if (copy_gbps) *copy_gbps = 2.0 * (double)bytes / (best_c * 1e-3) / 1e9;
  return BS_OK;
}

// ---- MFMA probe (bench.py "mfma_measured"): dense bf16 matrix-core rate of this device.
// Every wave keeps 8 independent accumulator chains of v_mfma_f32_32x32x16_bf16 (16x16x32 for
// shape = 1) on register operands, 2 waves per SIMD (8 per CU) on a 4-block-per-CU grid: issue-bound
// on the matrix pipes, no memory traffic.  The result is stored only if it equals a value it never
// takes, which keeps the chains live.
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int SHAPE>
__global__ __launch_bounds__(128) void probe_mfma_kernel(int iters, float* sink) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    a[j] = (bf16)(1.0f + 0.001f * (float)((lane + j) & 7));
    b[j] = (bf16)(0.5f - 0.001f * (float)((lane * 3 + j) & 7));
  }
  float tot = 0.f;
  if constexpr (SHAPE == 0) {
    f32x16 acc[8];
#pragma unroll
    for (int c = 0; c < 8; c++) acc[c] = (f32x16){};
    for (int i = 0; i < iters; i++)
#pragma unroll
      for (int c = 0; c < 8; c++) acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
      for (int j = 0; j < 16; j++) tot += acc[c][j];
  } else {
    f32x4 acc[8];
#pragma unroll
    for (int c = 0; c < 8; c++) acc[c] = (f32x4){};
    for (int i = 0; i < iters; i++)
#pragma unroll
      for (int c = 0; c < 8; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
      for (int j = 0; j < 4; j++) tot += acc[c][j];
  }
  if (tot == -1.2345f) sink[blockIdx.x] = tot;
}

extern "C" int bs_mfma_probe(int32_t device, double* tflops_32x32x16, double* tflops_16x16x32) {
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  ProbeRes p;
  int rc = p.init(1u << 20, 1);
  if (rc) return rc;
  const int iters = 4096, blocks = prop.multiProcessorCount * 4;
  const double flops_per_iter[2] = {2.0 * 32 * 32 * 16, 2.0 * 16 * 16 * 32};  // per MFMA instruction
  double best[2] = {0.0, 0.0};
  for (int shape = 0; shape < 2; shape++) {
    for (int it = 0; it < 6; it++) {
      float ms = 0.f;
      rc = p.timed([&] {
        if (shape == 0) probe_mfma_kernel<0><<<blocks, 128, 0, p.st>>>(iters, (float*)p.buf[0]);
        else probe_mfma_kernel<1><<<blocks, 128, 0, p.st>>>(iters, (float*)p.buf[0]);
      }, &ms);
      if (rc) return rc;
      const double fl = (double)blocks * 2 /* waves */ * iters * 8 /* chains */ * flops_per_iter[shape];
      if (it >= 1) best[shape] = std::max(best[shape], fl / (ms * 1e-3) / 1e12);
    }
  }
  if (tflops_32x32x16) *tflops_32x32x16 = best[0];
  if (tflops_16x16x32) *tflops_16x16x32 = best[1];
  return BS_OK;
}

namespace {
struct ProfScope {
  bs_stage* s;
  hipStream_t st;
  bool on;
  ProfScope(bs_stage* s_, hipStream_t st_, int cls, double units) : s(s_), st(st_), on(s_->prof.cls == cls && cls) {
    if (on) {
      hipEventRecord(prof_event(s), st);
      s->prof.algo += units;
    }
  }
  ~ProfScope() {
    if (on) hipEventRecord(prof_event(s), st);
  }
};
}  // namespace

// Matrix t of a block as the kernels take it: the one place of the forward that knows the weight formats
// (int8 with row scales, MXFP4 with block scales, else the stage's own type).
static WMat wmat(const Layer& w, int t) { return WMat{w.t[t], w.sc[t], w.mxs[t]}; }

// Algorithmic bytes of one weight GEMV launch (decode): weights (+ scales) + bias + activations in/out.
static double gemv_bytes(const bs_stage* s, const WMat& w, int M, int N, int K, int out_bytes) {
  return wmat_stream_bytes(w, N, K, s->esz) + (double)N * s->esz + (double)M * K * s->esz + (double)M * N * out_bytes;
}

// The forward's GEMVs may split K through the stage's workspace (see kSkCap).
static Epi with_splitk(const bs_stage* s, const Epi& ep) {
  Epi e = ep;
  e.sk_ws = s->sk_ws; e.sk_tickets = s->sk_tickets; e.sk_cap = kSkCap; e.sk_ntickets = kSkTickets;
  return e;
}

// One profile record per launch: a weight-stream-bound GEMV by its bytes (class 1), a GEMM by its flops (class 2).
static void linear(bs_stage* s, hipStream_t st, const void* X, const WMat& w, int M, int N, int K, const Epi& ep,
                   int out_bytes) {
  const bool gemv = wmat_streams(s->bf16, w, M, N, K);
  ProfScope p(s, st, gemv ? 1 : 2, gemv ? gemv_bytes(s, w, M, N, K, out_bytes) : 2.0 * M * N * K);
  launch_wmat(s->bf16, X, w, s->wtmp, M, N, K, ep, st);
}

static void linear_ln(bs_stage* s, hipStream_t st, const float* x, int row_stride, int row_offset, const void* g,
                      const void* b, const WMat& w, int M, int N, int K, const Epi& ep, int out_bytes) {
  if (!wmat_takes_ln(w, M, K)) {  // a quantised matrix beyond its LN-fused shapes: LayerNorm on its own, unrecorded
    launch_ln_rows(x, row_stride, row_offset, g, b, s->d.ln_eps, s->xn, M, K, st);
    linear(s, st, s->xn, w, M, N, K, ep, out_bytes);
    return;
  }
  const bool gemv = wmat_streams(s->bf16, w, M, N, K);
  ProfScope p(s, st, gemv ? 1 : 2, gemv ? gemv_bytes(s, w, M, N, K, out_bytes) : 2.0 * M * N * K);
  launch_wmat_ln(s->bf16, x, row_stride, row_offset, g, b, s->d.ln_eps, s->xn, w, M, N, K, ep, st);
}

// Does a row of [slot, slot + B) hold sampler state (bs_set_row_sampler)?  Then the tail is the per-row sampler.
static bool rows_sampled(const bs_stage* s, int slot, int B) {
  if (!s->rs_active) return false;
  for (int b = 0; b < B; b++)
    if (s->rs_host[slot + b].active) return true;
  return false;
}

// Does a row of [slot, slot + B) hold processor state (bs_set_row_processor)?  Then the tail applies it before the pick.
static bool rows_processed(const bs_stage* s, int slot, int B) {
  if (!s->lp_active) return false;
  for (int b = 0; b < B; b++)
    if (s->lp_host[slot + b].active) return true;
  return false;
}

// Does a row of [slot, slot + B) hold guide state (bs_set_row_guide)?  Then the tail masks before and steps after the pick.
static bool rows_guided(const bs_stage* s, int slot, int B) {
  if (!s->gd_active) return false;
  for (int b = 0; b < B; b++)
    if (s->gd_host[slot + b] >= 0) return true;
  return false;
}

// Which tail this pass ends in (scoring: a bs_forward_score pass).  forward_impl has checked the step against the stage.
static Tail plan_tail(const bs_stage* s, const bs_step* step, bool scoring, bool topk = false) {
  const int B = step->batch, M = B * step->seq, V = s->d.vocab;
  if (!s->d.is_last) return Tail{};
  if (s->n_labels) return Tail{TAIL_CLASSIFY, B, s->n_labels};
  if (scoring) return Tail{TAIL_SCORE, M, V};
  if (topk) return Tail{TAIL_TOPK_LOGPROBS, B, V};  // bs_forward_topk has excluded sampler state of either kind
  const bool rows = rows_sampled(s, step->slot, B);  // excludes top_k > 1 (bs_set_row_sampler / bs_set_sampling)
  if (step->flags & BS_STEP_VERIFY)
    return Tail{rows && (step->flags & BS_STEP_VERIFY_DRAW) ? TAIL_VERIFY_DRAW : TAIL_VERIFY_ARGMAX, M, V};
  if (rows_guided(s, step->slot, B)) return Tail{TAIL_ROWS_GUIDE, B, V};    // forward_impl has excluded verify passes
  if (rows_processed(s, step->slot, B)) return Tail{TAIL_ROWS_PROC, B, V};
  if (rows) return Tail{TAIL_ROWS, B, V};
  if (s->top_k > 1) return Tail{TAIL_TOPK, B, V};
  if (s->hs_on && s->hs.Q && !(step->flags & BS_STEP_LOGITS) && head_screen_supported(B, s->d.hidden))
    return Tail{TAIL_SCREENED, B, V};
  return Tail{TAIL_GREEDY, B, V};
}

// Device staging for logits requested with host I/O: one buffer per stage, grown on demand (a
// stream-ordered hipMallocAsync/hipFreeAsync pair per call handed blocks across the streams of
// two stages and returned zeros on ROCm 7.2; this is also cheaper).
static int logits_staging(bs_stage* s, size_t bytes, hipStream_t st, float** out) {
  if (bytes > s->logit_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    if (s->logit_buf) {
      s->owned.erase(std::find_if(s->owned.begin(), s->owned.end(), [&](const OwnedAlloc& a) { return a.p == s->logit_buf; }));
      HIP_TRY(hipFree(s->logit_buf));
    }
    s->logit_buf = nullptr;
    s->logit_cap = 0;
    if (!owned_alloc(s, bytes, false, (void**)&s->logit_buf)) return fail(BS_ERR_OOM, "logits staging allocation failed");
    s->logit_cap = bytes;
  }
  *out = s->logit_buf;
  return BS_OK;
}

// Where a tail's head writes its logits: the caller's device buffer, with host I/O the staging (*staged, which
// tail_copy_out copies to the caller), else `priv`, the buffer the kind's own pick reads (null: none are written).
static int tail_logits(bs_stage* s, const Tail& t, const bs_step* step, float* caller, float* priv, hipStream_t st,
                       float** dev, float** staged) {
  *staged = nullptr;
  *dev = priv;
  if (!(step->flags & BS_STEP_LOGITS)) return BS_OK;
  if (!(step->flags & BS_STEP_HOST_IO)) {
    *dev = caller;
    return BS_OK;
  }
  int rc = logits_staging(s, (size_t)t.rows * t.width * 4, st, staged);
  if (rc == BS_OK) *dev = *staged;
  return rc;
}

// Host I/O: the tail's ids from their device staging `tok` to `out`, the staged logits to the caller's buffer.
static int tail_copy_out(const Tail& t, const bs_step* step, const int* tok, void* out, const float* staged,
                         float* logits, hipStream_t st) {
  if (!(step->flags & BS_STEP_HOST_IO)) return BS_OK;
  HIP_TRY(hipMemcpyAsync(out, tok, (size_t)t.rows * 4, hipMemcpyDeviceToHost, st));
  if (staged) HIP_TRY(hipMemcpyAsync(logits, staged, (size_t)t.rows * t.width * 4, hipMemcpyDeviceToHost, st));
  return BS_OK;
}

// Enqueue one forward on `st`.  The kernels read each row's past_len from past_dev (device [B],
// written ahead of the forward or of the graph replay); `pasts` is the host copy (profiling bytes).
// tail: what forward_impl planned; sc: what a TAIL_SCORE reads and writes (bs_forward_score); tk: what a
// TAIL_TOPK_LOGPROBS writes (bs_forward_topk).
static int enqueue_forward(bs_stage* s, const bs_step* step, const Tail& tail, const void* in, void* out, float* logits,
                           hipStream_t st, const int* past_dev, const std::vector<int>& pasts,
                           const ScoreIO* sc = nullptr, const TopkIO* tk = nullptr) {
  const bs_stage_desc& d = s->d;
  const int B = step->batch, S = step->seq, slot = step->slot, past = pasts[0];
  double ctx_sum = 0.0;
  for (int b = 0; b < B; b++) ctx_sum += (double)pasts[b] + S;
  const int M = B * S;
  const bool host_io = (step->flags & BS_STEP_HOST_IO) != 0;
  const bool verify = (step->flags & BS_STEP_VERIFY) != 0;  // forward_impl checked the shape and the stage
  const int h = d.hidden, V = d.vocab, hd = s->hd, nh = d.n_head;

  // ---- input
  const float* cur = nullptr;
  const int* ids = nullptr;
  // bf16 decode of <= 2 rows: the embedding gather and its LayerNorm run in layer 0's LN + QKV kernel
  const bool emb_fused = d.is_first && s->bf16 && !s->q8 && !s->mx4 && M <= 2 && s->L > 0;
  if (d.is_first) {
    ids = (const int*)in;
    if (host_io) {
      HIP_TRY(hipMemcpyAsync(s->ids, ids, (size_t)M * 4, hipMemcpyHostToDevice, st));
      ids = s->ids;
    }
    if (!emb_fused) launch_layernorm(s->bf16, s->wemb, ids, 0, 0, s->emb_g, s->emb_b, s->xa, 1, M, h, d.ln_eps, st);
    cur = s->xa;
  } else if (host_io) {
    HIP_TRY(hipMemcpyAsync(s->xa, in, (size_t)M * h * 4, hipMemcpyHostToDevice, st));
    cur = s->xa;
  } else {
    cur = (const float*)in;
  }

  // ---- decoder blocks
  const float inv_norm = 1.0f / std::sqrt((float)hd);
  for (int l = 0; l < s->L; l++) {
    const Layer& w = s->layers[l];
    char* kbase = s->kv + l * s->kv_layer_stride;
    // x1 = LN_in(x); fused QKV (+bias) -> q, K/V cache
    Epi e{};
    e.kind = EPI_QKV; e.bias = w.t[T_QKV_B]; e.q_out = s->q; e.k_cache = kbase; e.v_cache = kbase + s->kv_half;
    e.hidden = h; e.head_dim = hd; e.max_ctx = d.max_ctx; e.n_head = nh; e.seq = S; e.slot = slot; e.past = past;
    e.past_dev = past_dev; e.ldo = 3 * h;
    // int8 KV: the epilogue writes the call's bf16 K / V rows to staging [B][head][lmax][hd]; S == 1 keeps one
    // position per (row, head) at static arguments (graph-capturable), S > 1 lays each row out as the prefill
    // attention reads it: its dequantised past, then the new positions at past_b ..
    KvQ8 kq{};
    const int past_max = *std::max_element(pasts.begin(), pasts.end());
    const int lmax = S == 1 ? 1 : past_max + S;
    if (s->kv8) {
      kq.k_scale = s->kv_scales + (size_t)l * 2 * s->kv_sc_half; kq.v_scale = kq.k_scale + s->kv_sc_half;
      kq.k_stage = (bf16*)s->kv_stage; kq.v_stage = kq.k_stage + s->kv_stage_cap * h;
      e.k_cache = kq.k_stage; e.v_cache = kq.v_stage; e.slot = 0; e.max_ctx = lmax;
      if (S == 1) { e.past_dev = nullptr; e.past = 0; }
    }
    bool done = false;
    if (l == 0 && emb_fused) {
      ProfScope p(s, st, 1, gemv_bytes(s, wmat(w, T_QKV_W), M, 3 * h, h, 4) + (double)M * h * (s->esz + 4));
      done = launch_linear_emb(ids, s->wemb, s->emb_g, s->emb_b, s->xa, w.t[T_LN1_G], w.t[T_LN1_B], d.ln_eps,
                               w.t[T_QKV_W], M, 3 * h, h, with_splitk(s, e), st);
      if (!done) launch_layernorm(s->bf16, s->wemb, ids, 0, 0, s->emb_g, s->emb_b, s->xa, 1, M, h, d.ln_eps, st);
    }
    if (!done)
      linear_ln(s, st, cur, 1, 0, w.t[T_LN1_G], w.t[T_LN1_B], wmat(w, T_QKV_W), M, 3 * h, h, with_splitk(s, e), 4);
    // attention
    AttnArgs a{};
    a.q = s->q; a.k_cache = kbase; a.v_cache = kbase + s->kv_half; a.ctx_out = s->ctx; a.slopes = s->slopes;
    a.B = B; a.S = S; a.slot = slot; a.past = past; a.past_dev = past_dev; a.n_head = nh; a.head_dim = hd;
    a.max_ctx = d.max_ctx; a.hidden = h; a.inv_norm = inv_norm; a.part_acc = s->part_acc; a.part_ml = s->part_ml;
    a.max_chunks = s->max_chunks; a.chunk = s->chunk; a.tickets = s->att_tickets;
    // prefill: the long query tiles' keys split over blocks of 4 key tiles, partials in the GEMM split-K
    // workspace (free between the QKV GEMM and the dense GEMM on this stream)
    a.pf_tiles = 4; a.pf_ws = s->sk_ws; a.pf_cap = kSkCap; a.pf_tickets = s->sk_tickets; a.pf_ntickets = kSkTickets;
    a.pf_past_max = *std::max_element(pasts.begin(), pasts.end());
    // a split decode context merges in the dense GEMV's prologue when that kernel can take it
    const int nsplit = S == 1 ? attention_decode_splits(B, nh, s->max_chunks) : 1;
    const WMat dense = wmat(w, T_DENSE_W);
    a.defer_merge = s->bf16 && nsplit > 1 && wmat_parts_supported(dense, M, h, hd, nsplit);
    // a = x + dense(ctx)
    Epi e2{};
    e2.kind = EPI_RESID; e2.bias = w.t[T_DENSE_B]; e2.out_f32 = s->attn; e2.resid = cur; e2.ldo = h;
    if (verify) {
      // short-query split-context attention on a static grid (attn_verify.hip): every row's length from past_dev
      ProfScope p(s, st, 3, ctx_sum * nh * hd * 2 * s->esz);
      AttnArgs av = a;
      av.part_acc = s->vf_acc; av.part_ml = s->vf_ml; av.max_chunks = s->vf_stride;
      launch_attention_verify(s->bf16, av, st);
    } else if (!s->kv8) {
      ProfScope p(s, st, 3, ctx_sum * nh * hd * 2 * s->esz);
      launch_attention(s->bf16, a, st);
    } else if (S == 1) {
      ProfScope p(s, st, 3, ctx_sum * nh * 2 * (hd + 4));
      launch_attention_q8(a, kq, st);
    } else {
      ProfScope p(s, st, 3, ctx_sum * nh * 2 * (hd + 4));
      launch_kv_dequant(kbase, kbase + s->kv_half, kq, past_dev, B, slot, nh, hd, d.max_ctx, lmax, past_max, st);
      AttnArgs as = a;
      as.k_cache = kq.k_stage; as.v_cache = kq.v_stage; as.slot = 0; as.max_ctx = lmax;
      launch_attention(1, as, st);
      launch_kv_quant(kbase, kbase + s->kv_half, kq, past_dev, B, S, slot, nh, hd, d.max_ctx, lmax, st);
    }
    if (a.defer_merge) {
      const AttnParts parts{s->part_acc, s->part_ml, nsplit, nh, hd, s->max_chunks, slot};
      ProfScope p(s, st, 1, gemv_bytes(s, dense, M, h, h, 4));
      launch_wmat_parts(parts, dense, M, h, h, e2, st);
    } else {
      linear(s, st, s->ctx, dense, M, h, h, with_splitk(s, e2), 4);
    }
    // x2 = LN_post(a); g = gelu(x2 W1 + b1)
    Epi e3{};
    e3.kind = EPI_GELU; e3.bias = w.t[T_FC1_B]; e3.out_act = s->g; e3.ldo = 4 * h;
    linear_ln(s, st, s->attn, 1, 0, w.t[T_LN2_G], w.t[T_LN2_B], wmat(w, T_FC1_W), M, 4 * h, h, with_splitk(s, e3),
              (int)s->esz);
    // x = a + g W2 + b2
    float* nxt = (!d.is_last && !host_io && l == s->L - 1) ? (float*)out : (cur == s->xa ? s->xb : s->xa);
    Epi e4{};
    e4.kind = EPI_RESID; e4.bias = w.t[T_FC2_B]; e4.out_f32 = nxt; e4.resid = s->attn; e4.ldo = h;
    linear(s, st, s->g, wmat(w, T_FC2_W), M, h, 4 * h, with_splitk(s, e4), 4);
    cur = nxt;
  }

  // ---- output: the tail forward_impl planned.  Each tail's last kernel advances past_dev by S for the B rows.
  int rc = BS_OK;
  float* staged = nullptr;  // host-I/O logits on their way to the caller
  switch (tail.kind) {
    case TAIL_NONE:
      if (host_io) HIP_TRY(hipMemcpyAsync(out, cur, (size_t)M * h * 4, hipMemcpyDeviceToHost, st));
      else if (s->L == 0) HIP_TRY(hipMemcpyAsync(out, cur, (size_t)M * h * 4, hipMemcpyDeviceToDevice, st));
      break;
    case TAIL_CLASSIFY: {
      // sequence-classification tail (run_inference_with_binary_classification, inference.cpp:220-270): ln_f on each
      // row's last position, score, first maximal class
      float* dev_logits = nullptr;
      if ((rc = tail_logits(s, tail, step, logits, nullptr, st, &dev_logits, &staged)) != BS_OK) return rc;
      launch_layernorm(s->bf16, cur, nullptr, S, S - 1, s->lnf_g, s->lnf_b, s->xn, 0, B, h, d.ln_eps, st);
      launch_classify(s->bf16, s->xn, s->score, B, s->n_labels, h, dev_logits, host_io ? s->tok : (int*)out, s->past_dev,
                      S, st);
      return tail_copy_out(tail, step, s->tok, out, staged, logits, st);
    }
    case TAIL_SCORE: {
      // teacher-forced scoring: ln_f of all M positions -> xn, then the tied lm_head fused with a log-softmax
      // (head_score.hip)
      const int* tg = sc->targets;
      if (host_io && tg) {
        HIP_TRY(hipMemcpyAsync(s->sc_targets, tg, (size_t)M * 4, hipMemcpyHostToDevice, st));
        tg = s->sc_targets;
      }
      int* top = sc->top_ids ? (host_io ? s->sc_top : sc->top_ids) : nullptr;
      float* scr = sc->scores ? (host_io ? s->sc_scores : sc->scores) : nullptr;
      launch_layernorm(s->bf16, cur, nullptr, 1, 0, s->lnf_g, s->lnf_b, s->xn, 0, M, h, d.ln_eps, st);
      {
        ProfScope p(s, st, 2, 2.0 * M * V * h);
        launch_head_score(s->xn, s->wemb, tg, M, V, h, s->cus, s->sc_parts, top, scr, s->past_dev, B, S, st);
      }
      if (host_io) {
        if (top) HIP_TRY(hipMemcpyAsync(sc->top_ids, top, (size_t)M * 4, hipMemcpyDeviceToHost, st));
        if (scr) HIP_TRY(hipMemcpyAsync(sc->scores, scr, (size_t)M * 12, hipMemcpyDeviceToHost, st));
      }
      break;
    }
    case TAIL_VERIFY_ARGMAX:
    case TAIL_VERIFY_DRAW: {
      // ln_f of all M positions and the tied lm_head over M rows (never screened), then the first index of the largest
      // logit at every position, or the row sampler's draw at each of them from the head's logits (row_sample.hip)
      const bool draws = tail.kind == TAIL_VERIFY_DRAW;
      Epi e{};
      e.kind = EPI_ARGMAX; e.keys = s->vf_keys; e.ldo = V;
      if ((rc = tail_logits(s, tail, step, logits, draws ? s->vd_logits : nullptr, st, &e.logits, &staged)) != BS_OK) return rc;
      int* tok_out = host_io ? s->vf_tok : (int*)out;
      linear_ln(s, st, cur, 1, 0, s->lnf_g, s->lnf_b, WMat{s->wemb}, M, V, h, with_splitk(s, e), 0);
      if (draws)
        launch_row_sample_verify(s->vd, e.logits, V, V, slot, B, S, past_dev, tok_out, s->past_dev, st);
      else
        launch_argmax_finalize(s->vf_keys, M, V / 16, nullptr, nullptr, tok_out, st, s->past_dev, S, B);
      return tail_copy_out(tail, step, s->vf_tok, out, staged, logits, st);
    }
    case TAIL_SCREENED:
    case TAIL_GREEDY:
    case TAIL_TOPK:
    case TAIL_ROWS:
    case TAIL_ROWS_PROC:
    case TAIL_ROWS_GUIDE: {
      // ln_f on each row's last position, tied lm_head, token pick
      const bool guided = tail.kind == TAIL_ROWS_GUIDE;
      const bool processed = tail.kind == TAIL_ROWS_PROC || guided;  // bs_set_row_guide has made the processors' buffers
      const bool reads_logits = tail.kind == TAIL_TOPK || tail.kind == TAIL_ROWS || processed;
      Epi e{};
      e.kind = EPI_ARGMAX; e.keys = s->keys; e.ldo = V;
      e.key_hi_index = tail.kind == TAIL_TOPK ? 1 : 0;  // sampling ranks equal logits by the higher index (decoding.cpp:44-45)
      if ((rc = tail_logits(s, tail, step, logits, reads_logits ? s->sample_logits : nullptr, st, &e.logits, &staged)) != BS_OK)
        return rc;
      int* tok_out = host_io ? s->tok : (int*)out;
      if (tail.kind == TAIL_SCREENED) {
        // int8 screening pass, then the exact head on the few tiles that can win
        {  // class 1 counts the bytes the screen really streams: int8 rows, scales, bound constants, rows in, hi/lo out
          ProfScope p(s, st, 1, (double)V * h + 8.0 * V + (double)B * h * 4 + (double)B * (V / 16) * 8);
          launch_head_screen(s->hs, cur, S, S - 1, s->lnf_g, s->lnf_b, d.ln_eps, B, V, h, s->cus, st);
        }
        // select + re-score + finalize stay outside class 1 (the candidate count is known on the device only)
        launch_head_pick(s->hs, cur, S, S - 1, s->lnf_g, s->lnf_b, d.ln_eps, s->wemb, B, V, h, e, s->cus, tok_out,
                         s->past_dev, S, st);
      } else {
        linear_ln(s, st, cur, S, S - 1, s->lnf_g, s->lnf_b, WMat{s->wemb}, B, V, h, with_splitk(s, e), 0);
        if (processed)  // in place: BS_STEP_LOGITS returns what the pick saw
          launch_logit_proc_apply(s->lp, e.logits, V, slot, B, st);
        if (guided)  // after the processors, as prefix_allowed_tokens_fn follows min_new_tokens
          launch_guide_apply(s->gd, e.logits, V, slot, B, st);
        if (tail.kind == TAIL_ROWS || processed)  // rows of the call without state get the first index of their largest logit
          launch_row_sample(s->rs, e.logits, V, V, slot, B, nullptr, past_dev, S, tok_out, s->past_dev, st);
        if (processed)  // each row with processor state appends its pick to its history
          launch_logit_proc_note_picks(s->lp, slot, B, tok_out, st);
        if (guided)  // each row with guide state steps by its pick
          launch_guide_advance_picks(s->gd, slot, B, tok_out, st);
        if (tail.kind == TAIL_TOPK)
          launch_topk_sample(s->keys, V / 16, e.logits, V, B, s->top_k, 1.0f / s->temperature, s->sample_seed, slot,
                             past_dev, S, tok_out, st, s->past_dev);
        if (tail.kind == TAIL_GREEDY)
          launch_argmax_finalize(s->keys, B, V / 16, nullptr, nullptr, tok_out, st, s->past_dev, S);
      }
      return tail_copy_out(tail, step, s->tok, out, staged, logits, st);
    }
    case TAIL_TOPK_LOGPROBS: {
      // ln_f on each row's last position, the full head with its logits written (the caller's buffer, with host I/O
      // the staging, else the sampling-logits buffer), then the k best and the log-sum-exp from them (beam_topk.hip)
      const int k = tk->k;
      float* dev_logits = s->sample_logits;
      if (tk->logits) {
        dev_logits = tk->logits;
        if (host_io && (rc = logits_staging(s, (size_t)B * V * 4, st, &dev_logits)) != BS_OK) return rc;
      }
      Epi e{};
      e.kind = EPI_ARGMAX; e.keys = s->keys; e.ldo = V; e.logits = dev_logits;
      linear_ln(s, st, cur, S, S - 1, s->lnf_g, s->lnf_b, WMat{s->wemb}, B, V, h, with_splitk(s, e), 0);
      launch_topk_logprobs(dev_logits, V, V, B, k, s->tk_pmax, s->tk_psum, s->tk_pkeys, host_io ? s->tk_ids : tk->ids,
                           host_io ? s->tk_lp : tk->logprobs, tk->lse ? (host_io ? s->tk_lse : tk->lse) : nullptr,
                           s->past_dev, S, st);
      if (host_io) {
        HIP_TRY(hipMemcpyAsync(tk->ids, s->tk_ids, (size_t)B * k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(tk->logprobs, s->tk_lp, (size_t)B * k * 4, hipMemcpyDeviceToHost, st));
        if (tk->lse) HIP_TRY(hipMemcpyAsync(tk->lse, s->tk_lse, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        if (tk->logits) HIP_TRY(hipMemcpyAsync(tk->logits, dev_logits, (size_t)B * V * 4, hipMemcpyDeviceToHost, st));
      }
      break;
    }
  }
  return BS_OK;
}

extern "C" int bs_head_norm(bs_stage* s, const float* hidden, int32_t B, int32_t S, void* xn, void* stream) {
  if (!s || !hidden || !xn) return fail(BS_ERR_INVALID, "stage/hidden/xn is NULL");
  if (!s->lnf_g) return fail(BS_ERR_STATE, "stage has no ln_f (needs is_last or a head slice)");
  if (B <= 0 || S <= 0 || B > s->d.max_batch) return fail(BS_ERR_INVALID, "bad batch/seq");
  HIP_TRY(hipSetDevice(s->d.device));
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  launch_layernorm(s->bf16, hidden, nullptr, S, S - 1, s->lnf_g, s->lnf_b, xn, 0, B, s->d.hidden, s->d.ln_eps, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("head_norm: ") + hipGetErrorString(err));
  return BS_OK;
}

extern "C" int bs_head_slice(bs_stage* s, const void* xn, int32_t B, const uint64_t* keys_in, uint64_t* keys_out,
                             int32_t* tokens, void* stream) {
  if (!s || !xn) return fail(BS_ERR_INVALID, "stage/xn is NULL");
  if (!s->hw || s->hv1 <= s->hv0) return fail(BS_ERR_STATE, "stage has no head slice");
  if (B <= 0 || B > s->d.max_batch) return fail(BS_ERR_INVALID, "bad batch");
  HIP_TRY(hipSetDevice(s->d.device));
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  const int n = s->hv1 - s->hv0;
  Epi e{};
  e.kind = EPI_ARGMAX; e.keys = s->keys; e.ldo = n; e.col_offset = s->hv0;
  linear(s, st, xn, WMat{s->hw}, B, n, s->d.hidden, e, 0);
  launch_argmax_finalize(s->keys, B, n / 16, (const unsigned long long*)keys_in, (unsigned long long*)keys_out,
                         tokens, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("head_slice: ") + hipGetErrorString(err));
  return BS_OK;
}

// ---- the graph cache: captured decode steps and verify passes by GraphKey, at most 64
static hipGraphExec_t find_graph(const bs_stage* s, const GraphKey& key) {
  for (const auto& g : s->graphs)
    if (g.first == key) return g.second;
  return nullptr;
}

static int insert_graph(bs_stage* s, const GraphKey& key, hipGraphExec_t exec) {
  if (s->graphs.size() >= 64) {
    HIP_TRY(hipStreamSynchronize(key.st));  // the evicted (oldest) graph may still be replaying on this stream
    hipGraphExecDestroy(s->graphs.front().second);
    s->graphs.erase(s->graphs.begin());
  }
  s->graphs.push_back({key, exec});
  return BS_OK;
}

// A setter changed what the captured tails hold (the pick, the screening, graphs off): wait for the device, drop all.
static int drop_graphs(bs_stage* s) {
  HIP_TRY(hipDeviceSynchronize());
  for (auto& g : s->graphs) hipGraphExecDestroy(g.second);
  s->graphs.clear();
  return BS_OK;
}

extern "C" int bs_set_sampling(bs_stage* s, int32_t top_k, float temperature, uint64_t seed) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (top_k > 16) return fail(BS_ERR_UNSUPPORTED, "top_k must be <= 16");
  if (top_k > 1 && (!s->d.is_last || s->n_labels))
    return fail(BS_ERR_UNSUPPORTED, "sampling needs the last stage of a generation model (whole lm_head)");
  if (top_k > 1 && !(temperature > 0.f)) return fail(BS_ERR_INVALID, "temperature must be positive");
  if (top_k > 1 && s->rs_active) return fail(BS_ERR_STATE, "rows hold per-row sampler state (bs_set_row_sampler)");
  if (top_k > 1 && s->lp_active) return fail(BS_ERR_STATE, "rows hold logit processor state (bs_set_row_processor)");
  if (top_k > 1 && s->gd_active) return fail(BS_ERR_STATE, "rows hold guide state (bs_set_row_guide)");
  HIP_TRY(hipSetDevice(s->d.device));
  if (top_k > 1 && !s->sample_logits) {
    HIP_TRY(hipStreamSynchronize(s->own));
    if (!owned_alloc(s, (size_t)s->d.max_batch * s->d.vocab * 4, false, (void**)&s->sample_logits))
      return fail(BS_ERR_OOM, "sampling logits allocation failed");
  }
  s->top_k = top_k < 1 ? 1 : top_k;
  s->temperature = top_k > 1 ? temperature : 1.f;
  s->sample_seed = seed;
  return drop_graphs(s);  // they hold the old pick as kernel arguments
}

// ---- per-row sampling (row_sample.hip)
static_assert(sizeof(bs_row_draw) == sizeof(RowDrawDev) && sizeof(bs_row_draw) == 40, "bs_row_draw layout");

// Sampler scratch (row_sample.hip lays it out): one allocation, zeroed by Carver's rule; `what` names it in errors.
static int sampler_scratch(bs_stage* s, size_t bytes, const std::string& what, char** base) {
  Carver c;
  c.piece(base, bytes);
  const int rc = c.alloc(s->own);
  if (rc == Carver::NO_MEMORY) return fail(BS_ERR_OOM, what + " allocation failed (" + std::to_string(bytes) + " B)");
  if (rc == Carver::NOT_ZEROED) return fail(BS_ERR_DEVICE, what + " memset");
  return BS_OK;
}

// The table, histograms and read-outs, and the [max_batch][V] logits buffer if bs_set_sampling has not made it
// (then it counts as workspace, else not).
static int row_sampler_buffers(bs_stage* s) {
  if (s->rs.table) return BS_OK;
  size_t off[6];
  const size_t bytes = row_sample_bytes(s->d.max_batch, off);
  char* base = nullptr;
  int rc = sampler_scratch(s, bytes, "row sampler buffers", &base);
  if (rc != BS_OK) return rc;
  if (!s->sample_logits && !owned_alloc(s, (size_t)s->d.max_batch * s->d.vocab * 4, true, (void**)&s->sample_logits)) {
    hipFree(base);
    return fail(BS_ERR_OOM, "sampling logits allocation failed");
  }
  s->owned.push_back({base, bytes});
  s->rs = row_sample_bufs(base, off);
  s->rs_host.assign(s->d.max_batch, RowSamplerDev{});
  return BS_OK;
}

static int row_sampler_stage_check(const bs_stage* s) {
  if (s->n_labels || !s->d.is_last || !s->wemb || s->hv0 != 0 || s->hv1 != s->d.vocab)
    return fail(BS_ERR_UNSUPPORTED, "per-row sampling needs the last stage of a generation model (whole lm_head)");
  return BS_OK;
}

extern "C" int bs_set_row_sampler(bs_stage* s, int32_t slot, int32_t count, const bs_row_sampler* params, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  int rc = row_sampler_stage_check(s);
  if (rc) return rc;
  if (count <= 0 || slot < 0 || slot > s->d.max_batch - count) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (params && s->top_k > 1) return fail(BS_ERR_STATE, "bs_set_sampling holds top_k > 1");
  std::vector<RowSamplerDev> rows(count, RowSamplerDev{});
  for (int i = 0; params && i < count; i++) {
    const bs_row_sampler& p = params[i];
    if (p.top_k < 0) return fail(BS_ERR_INVALID, "top_k must be >= 0");
    if (!(p.top_p > 0.f && p.top_p <= 1.f)) return fail(BS_ERR_INVALID, "top_p must be in (0, 1]");
    if (!(p.temperature > 0.f) || std::isinf(p.temperature)) return fail(BS_ERR_INVALID, "temperature must be positive and finite");
    rows[i] = RowSamplerDev{p.top_k, p.top_p, p.temperature, 1, p.seed};
  }
  if (!params && !s->rs.table) return BS_OK;  // nothing was ever set
  HIP_TRY(hipSetDevice(s->d.device));
  if ((rc = row_sampler_buffers(s)) != BS_OK) return rc;
  launch_row_table(s->rs, slot, rows.data(), count, stream ? (hipStream_t)stream : s->own);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("row sampler table: ") + hipGetErrorString(err));
  for (int i = 0; i < count; i++) {
    s->rs_active += rows[i].active - s->rs_host[slot + i].active;
    s->rs_host[slot + i] = rows[i];
  }
  return BS_OK;
}

extern "C" int bs_sample_logits(bs_stage* s, int32_t slot, int32_t batch, const int32_t* positions, const float* logits,
                                int32_t ld, int32_t* tokens, int32_t flags, void* stream) {
  if (!s || !positions || !logits || !tokens) return fail(BS_ERR_INVALID, "stage/positions/logits/tokens is NULL");
  int rc = row_sampler_stage_check(s);
  if (rc) return rc;
  const int V = s->d.vocab;
  if (batch <= 0 || slot < 0 || slot > s->d.max_batch - batch) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (ld < V) return fail(BS_ERR_INVALID, "ld must be >= vocab");
  if (flags & ~BS_STEP_HOST_IO) return fail(BS_ERR_INVALID, "only BS_STEP_HOST_IO is valid here");
  for (int b = 0; b < batch; b++)
    if (positions[b] < 0) return fail(BS_ERR_INVALID, "positions must be >= 0");
  HIP_TRY(hipSetDevice(s->d.device));
  if ((rc = row_sampler_buffers(s)) != BS_OK) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  const bool host_io = (flags & BS_STEP_HOST_IO) != 0;
  const float* dl = logits;
  int* dt = tokens;
  if (host_io) {
    float* stage_l = nullptr;
    const size_t n = (size_t)(batch - 1) * ld + V;  // the last row may end at its V-th column
    if ((rc = logits_staging(s, ((size_t)batch * ld) * 4, st, &stage_l)) != BS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(stage_l, logits, n * 4, hipMemcpyHostToDevice, st));
    dl = stage_l;
    dt = s->tok;
  }
  launch_row_sample(s->rs, dl, ld, V, slot, batch, positions, nullptr, 0, dt, nullptr, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("row sampler: ") + hipGetErrorString(err));
  if (host_io) {
    HIP_TRY(hipMemcpyAsync(tokens, s->tok, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return BS_OK;
}

extern "C" int bs_read_row_draw(bs_stage* s, int32_t slot, bs_row_draw* out) {
  if (!s || !out) return fail(BS_ERR_INVALID, "stage/out is NULL");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (!s->rs.table) return fail(BS_ERR_STATE, "the stage never ran the per-row sampler");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, s->rs.draw + slot, sizeof(*out), hipMemcpyDeviceToHost));
  return BS_OK;
}

// ---- per-row logit processors (logit_proc.hip)
static_assert(sizeof(bs_row_processor) + 4 == sizeof(RowProcDev) && BS_ROW_BIAS_MAX == kRowBiasMax, "bs_row_processor layout");

// The table and the rows' token state (zeroed), and the row sampler's buffers: its launches are the pick of a processed
// step, and its [max_batch][V] logits buffer is what the head writes when the caller gives none.
static int logit_proc_buffers(bs_stage* s) {
  if (s->lp.table) return BS_OK;
  int rc = row_sampler_buffers(s);
  if (rc != BS_OK) return rc;
  const size_t mb = s->d.max_batch, cap = (size_t)s->d.max_ctx + 1, words = ((size_t)s->d.vocab + 31) / 32;
  LogitProcBufs lp{};
  Carver c;
  c.piece(&lp.table, mb * sizeof(RowProcDev));
  c.piece(&lp.hist, mb * cap * 4);
  c.piece(&lp.distinct, mb * cap * 4);
  c.piece(&lp.seen, mb * words * 4);
  c.piece(&lp.counts, mb * 4 * 4);
  const int ar = c.alloc(s->own);
  if (ar == Carver::NO_MEMORY) return fail(BS_ERR_OOM, "logit processor buffers allocation failed (" + std::to_string(c.total) + " B)");
  if (ar == Carver::NOT_ZEROED) return fail(BS_ERR_DEVICE, "logit processor buffers memset");
  lp.cap = (int)cap; lp.words = (int)words; lp.V = s->d.vocab;
  s->owned.push_back({c.base, c.total});
  s->lp = lp;
  s->lp_host.assign(mb, bs_stage::RowProcHost{});
  return BS_OK;
}

extern "C" int bs_set_row_processor(bs_stage* s, int32_t slot, int32_t count, const bs_row_processor* params, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  int rc = row_sampler_stage_check(s);
  if (rc) return fail(BS_ERR_UNSUPPORTED, "logit processors need the last stage of a generation model (whole lm_head)");
  if (count <= 0 || slot < 0 || slot > s->d.max_batch - count) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (params && s->top_k > 1) return fail(BS_ERR_STATE, "bs_set_sampling holds top_k > 1");
  const int V = s->d.vocab;
  std::vector<RowProcDev> rows(count, RowProcDev{});
  for (int i = 0; params && i < count; i++) {
    const bs_row_processor& p = params[i];
    if (!std::isfinite(p.repetition_penalty) || !(p.repetition_penalty > 0.f))
      return fail(BS_ERR_INVALID, "repetition_penalty must be positive and finite");
    if (p.no_repeat_ngram < 0 || p.no_repeat_ngram > 32) return fail(BS_ERR_INVALID, "no_repeat_ngram must be in [0, 32]");
    if (p.min_new_tokens < 0) return fail(BS_ERR_INVALID, "min_new_tokens must be >= 0");
    if (p.eos_id >= V) return fail(BS_ERR_INVALID, "eos_id must be below vocab (negative: none)");
    if (p.n_bias < 0 || p.n_bias > BS_ROW_BIAS_MAX) return fail(BS_ERR_INVALID, "n_bias must be in [0, 64]");
    RowProcDev& r = rows[i];
    r.penalty = p.repetition_penalty; r.ngram = p.no_repeat_ngram; r.min_new = p.min_new_tokens;
    r.eos = p.eos_id < 0 ? -1 : p.eos_id; r.n_bias = p.n_bias; r.active = 1;
    for (int j = 0; j < p.n_bias; j++) {
      if (p.bias_ids[j] < 0 || p.bias_ids[j] >= V) return fail(BS_ERR_INVALID, "bias id outside [0, vocab)");
      if (std::isnan(p.bias_values[j]) || p.bias_values[j] == INFINITY)
        return fail(BS_ERR_INVALID, "bias value must be finite or -inf (a ban)");
      r.bias_ids[j] = p.bias_ids[j];
      r.bias_values[j] = p.bias_values[j];
    }
  }
  if (!params && !s->lp.table) return BS_OK;  // nothing was ever set
  HIP_TRY(hipSetDevice(s->d.device));
  if ((rc = logit_proc_buffers(s)) != BS_OK) return rc;
  launch_logit_proc_set(s->lp, slot, rows.data(), count, stream ? (hipStream_t)stream : s->own);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("logit processor table: ") + hipGetErrorString(err));
  for (int i = 0; i < count; i++) {
    s->lp_active += rows[i].active - s->lp_host[slot + i].active;
    s->lp_host[slot + i].active = rows[i].active;
    s->lp_host[slot + i].len = 0;
  }
  return BS_OK;
}

extern "C" int bs_note_tokens(bs_stage* s, int32_t slot, const int32_t* ids, int32_t n, int32_t flags, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (flags & ~(BS_STEP_HOST_IO | BS_NOTE_GENERATED)) return fail(BS_ERR_INVALID, "only BS_STEP_HOST_IO and BS_NOTE_GENERATED are valid here");
  if (n < 0 || (n > 0 && !ids)) return fail(BS_ERR_INVALID, "bad ids / n");
  if (!s->lp.table || !s->lp_host[slot].active) return fail(BS_ERR_STATE, "the row holds no logit processor state");
  if (s->lp_host[slot].len + n > s->lp.cap) return fail(BS_ERR_INVALID, "the row's token history would exceed max_ctx + 1");
  const bool host = (flags & BS_STEP_HOST_IO) != 0;
  if (host)
    for (int i = 0; i < n; i++)
      if (ids[i] < 0 || ids[i] >= s->d.vocab) return fail(BS_ERR_INVALID, "token id out of range");
  if (n == 0) return BS_OK;
  HIP_TRY(hipSetDevice(s->d.device));
  launch_logit_proc_note(s->lp, slot, host ? ids : nullptr, host ? nullptr : ids, n, (flags & BS_NOTE_GENERATED) ? 1 : 0,
                         stream ? (hipStream_t)stream : s->own);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("note tokens: ") + hipGetErrorString(err));
  s->lp_host[slot].len += n;
  return BS_OK;
}

extern "C" int bs_process_logits(bs_stage* s, int32_t slot, int32_t batch, float* logits, int32_t ld, int32_t flags,
                                 void* stream) {
  if (!s || !logits) return fail(BS_ERR_INVALID, "stage/logits is NULL");
  if (row_sampler_stage_check(s)) return BS_ERR_UNSUPPORTED;
  const int V = s->d.vocab;
  if (batch <= 0 || slot < 0 || slot > s->d.max_batch - batch) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (ld < V) return fail(BS_ERR_INVALID, "ld must be >= vocab");
  if (flags & ~BS_STEP_HOST_IO) return fail(BS_ERR_INVALID, "only BS_STEP_HOST_IO is valid here");
  HIP_TRY(hipSetDevice(s->d.device));
  int rc = logit_proc_buffers(s);
  if (rc != BS_OK) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  const bool host_io = (flags & BS_STEP_HOST_IO) != 0;
  float* dl = logits;
  const size_t n = (size_t)(batch - 1) * ld + V;  // the last row may end at its V-th column
  if (host_io) {
    if ((rc = logits_staging(s, (size_t)batch * ld * 4, st, &dl)) != BS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dl, logits, n * 4, hipMemcpyHostToDevice, st));
  }
  launch_logit_proc_apply(s->lp, dl, ld, slot, batch, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("logit processors: ") + hipGetErrorString(err));
  if (host_io) {
    HIP_TRY(hipMemcpyAsync(logits, dl, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return BS_OK;
}

extern "C" int bs_read_row_tokens(bs_stage* s, int32_t slot, int32_t* tokens, int32_t* n_tokens, int32_t* n_generated,
                                  int32_t* n_distinct) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (!s->lp.table) return fail(BS_ERR_STATE, "the stage never used the logit processors");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());
  int cnt[4];
  HIP_TRY(hipMemcpy(cnt, s->lp.counts + (size_t)slot * 4, sizeof(cnt), hipMemcpyDeviceToHost));
  const int len = std::min(std::max(cnt[0], 0), s->lp.cap);
  if (tokens && len) HIP_TRY(hipMemcpy(tokens, s->lp.hist + (size_t)slot * s->lp.cap, (size_t)len * 4, hipMemcpyDeviceToHost));
  if (n_tokens) *n_tokens = len;
  if (n_generated) *n_generated = cnt[2];
  if (n_distinct) *n_distinct = cnt[1];
  return BS_OK;
}

// ---- guided decoding (guide.hip)
static_assert(BS_GUIDE_MAX == kGuideMax && BS_GUIDE_SLICE == kGuideSlice, "guide constants");

static int guide_stage_check(const bs_stage* s) {
  if (s->n_labels || !s->d.is_last || !s->wemb || s->hv0 != 0 || s->hv1 != s->d.vocab)
    return fail(BS_ERR_UNSUPPORTED, "guided decoding needs the last stage of a generation model (whole lm_head)");
  return BS_OK;
}

// The descriptor table (zeroed: nothing loaded) and the rows' guide state (every row cleared).
static int guide_buffers(bs_stage* s) {
  if (s->gd.guides) return BS_OK;
  const size_t mb = s->d.max_batch;
  GuideBufs gd{};
  Carver c;
  c.piece(&gd.guides, kGuideMax * sizeof(GuideDev));
  c.piece(&gd.rows, mb * sizeof(GuideRowDev));
  const int ar = c.alloc(s->own);
  if (ar == Carver::NO_MEMORY) return fail(BS_ERR_OOM, "guide table allocation failed");
  if (ar == Carver::NOT_ZEROED) return fail(BS_ERR_DEVICE, "guide table memset");
  gd.V = s->d.vocab;
  launch_guide_set(gd, 0, (int)mb, -1, nullptr, s->own);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s->own) != hipSuccess) {
    hipFree(c.base);
    return fail(BS_ERR_DEVICE, "guide table clear");
  }
  s->owned.push_back({c.base, c.total});
  s->gd = gd;
  s->gd_host.assign(mb, -1);
  return BS_OK;
}

extern "C" int bs_load_guide(bs_stage* s, const bs_guide_desc* g, int32_t* guide_id) {
  if (!s || !g || !guide_id) return fail(BS_ERR_INVALID, "stage/guide/guide_id is NULL");
  int rc = guide_stage_check(s);
  if (rc) return rc;
  std::string why;
  if (!guide_table_check(g, s->d.vocab, &why)) return fail(BS_ERR_INVALID, "guide: " + why);
  int id = 0;
  while (id < kGuideMax && s->gd_guides[id].base) id++;
  if (id == kGuideMax) return fail(BS_ERR_STATE, "the stage holds BS_GUIDE_MAX guides already");
  HIP_TRY(hipSetDevice(s->d.device));
  if ((rc = guide_buffers(s)) != BS_OK) return rc;
  const size_t n = g->n_states, ne = g->row_ptr[n];
  int *row_ptr = nullptr, *tok = nullptr, *next = nullptr, *dn = nullptr;
  Carver c;
  c.piece(&row_ptr, (n + 1) * 4);
  c.piece(&tok, ne * 4);
  c.piece(&next, ne * 4);
  c.piece(&dn, n * 4);
  if (c.alloc() != Carver::OK) return fail(BS_ERR_OOM, "guide allocation failed (" + std::to_string(c.total) + " B)");
  const GuideDev dev{row_ptr, tok, next, dn, g->n_states, g->start};
  hipError_t e = hipMemcpy(row_ptr, g->row_ptr, (n + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && ne) e = hipMemcpy(tok, g->edge_token, ne * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && ne) e = hipMemcpy(next, g->edge_next, ne * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dn, g->default_next, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->gd.guides + id, &dev, sizeof(dev), hipMemcpyHostToDevice);  // last: the arrays are in place
  if (e != hipSuccess) {
    hipFree(c.base);
    return fail(BS_ERR_DEVICE, std::string("guide copy: ") + hipGetErrorString(e));
  }
  s->owned.push_back({c.base, (2 * n + 1 + 2 * ne) * 4});
  s->gd_guides[id] = bs_stage::GuideHost{c.base, g->n_states, g->start, 0};
  *guide_id = id;
  return BS_OK;
}

extern "C" int bs_unload_guide(bs_stage* s, int32_t id) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (id < 0 || id >= kGuideMax || !s->gd_guides[id].base) return fail(BS_ERR_STATE, "no such guide is loaded");
  if (s->gd_guides[id].refs) return fail(BS_ERR_STATE, "a row still references the guide (bs_set_row_guide clears it)");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());  // launches that read the guide have finished
  const GuideDev none{};
  HIP_TRY(hipMemcpy(s->gd.guides + id, &none, sizeof(none), hipMemcpyHostToDevice));
  void* base = s->gd_guides[id].base;
  s->owned.erase(std::find_if(s->owned.begin(), s->owned.end(), [&](const OwnedAlloc& a) { return a.p == base; }));
  s->gd_guides[id] = bs_stage::GuideHost{};
  HIP_TRY(hipFree(base));
  return BS_OK;
}

extern "C" int bs_set_row_guide(bs_stage* s, int32_t slot, int32_t count, int32_t id, const int32_t* states, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  int rc = guide_stage_check(s);
  if (rc) return rc;
  if (count <= 0 || slot < 0 || slot > s->d.max_batch - count) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  const bool set = id >= 0;
  if (set && (id >= kGuideMax || !s->gd_guides[id].base)) return fail(BS_ERR_STATE, "no such guide is loaded");
  if (set && s->top_k > 1) return fail(BS_ERR_STATE, "bs_set_sampling holds top_k > 1");
  if (!set && !s->gd.guides) return BS_OK;  // nothing was ever loaded
  std::vector<int> st(count, set ? s->gd_guides[id].start : 0);
  for (int i = 0; set && states && i < count; i++) {
    if (states[i] < 0 || states[i] >= s->gd_guides[id].n_states) return fail(BS_ERR_INVALID, "state outside the guide");
    st[i] = states[i];
  }
  HIP_TRY(hipSetDevice(s->d.device));
  if (set && (rc = logit_proc_buffers(s)) != BS_OK) return rc;  // the route runs the processors' and the sampler's launches
  launch_guide_set(s->gd, slot, count, set ? id : -1, st.data(), stream ? (hipStream_t)stream : s->own);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("guide row table: ") + hipGetErrorString(err));
  for (int i = 0; i < count; i++) {
    int& cur = s->gd_host[slot + i];
    if (cur >= 0) { s->gd_guides[cur].refs--; s->gd_active--; }
    cur = set ? id : -1;
    if (set) { s->gd_guides[id].refs++; s->gd_active++; }
  }
  return BS_OK;
}

extern "C" int bs_advance_row_guide(bs_stage* s, int32_t slot, const int32_t* ids, int32_t n, int32_t flags, void* stream) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (flags & ~BS_STEP_HOST_IO) return fail(BS_ERR_INVALID, "only BS_STEP_HOST_IO is valid here");
  if (n < 0 || (n > 0 && !ids)) return fail(BS_ERR_INVALID, "bad ids / n");
  if (!s->gd.guides || s->gd_host[slot] < 0) return fail(BS_ERR_STATE, "the row holds no guide state");
  const bool host = (flags & BS_STEP_HOST_IO) != 0;
  if (host)
    for (int i = 0; i < n; i++)
      if (ids[i] < 0 || ids[i] >= s->d.vocab) return fail(BS_ERR_INVALID, "token id out of range");
  if (n == 0) return BS_OK;
  HIP_TRY(hipSetDevice(s->d.device));
  launch_guide_advance(s->gd, slot, host ? ids : nullptr, host ? nullptr : ids, n, stream ? (hipStream_t)stream : s->own);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("guide advance: ") + hipGetErrorString(err));
  return BS_OK;
}

extern "C" int bs_guide_logits(bs_stage* s, int32_t slot, int32_t batch, float* logits, int32_t ld, int32_t flags,
                               void* stream) {
  if (!s || !logits) return fail(BS_ERR_INVALID, "stage/logits is NULL");
  int rc = guide_stage_check(s);
  if (rc) return rc;
  const int V = s->d.vocab;
  if (batch <= 0 || slot < 0 || slot > s->d.max_batch - batch) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  if (ld < V) return fail(BS_ERR_INVALID, "ld must be >= vocab");
  if (flags & ~BS_STEP_HOST_IO) return fail(BS_ERR_INVALID, "only BS_STEP_HOST_IO is valid here");
  if (!s->gd.guides) return fail(BS_ERR_STATE, "the stage never loaded a guide");
  HIP_TRY(hipSetDevice(s->d.device));
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  const bool host_io = (flags & BS_STEP_HOST_IO) != 0;
  float* dl = logits;
  const size_t n = (size_t)(batch - 1) * ld + V;  // the last row may end at its V-th column
  if (host_io) {
    if ((rc = logits_staging(s, (size_t)batch * ld * 4, st, &dl)) != BS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dl, logits, n * 4, hipMemcpyHostToDevice, st));
  }
  launch_guide_apply(s->gd, dl, ld, slot, batch, st);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("guide apply: ") + hipGetErrorString(err));
  if (host_io) {
    HIP_TRY(hipMemcpyAsync(logits, dl, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return BS_OK;
}

extern "C" int bs_read_row_guide(bs_stage* s, int32_t slot, int32_t* guide_id, int32_t* state, int32_t* n_steps,
                                 int32_t* n_rejected) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (slot < 0 || slot >= s->d.max_batch) return fail(BS_ERR_INVALID, "slot out of range");
  if (!s->gd.guides) return fail(BS_ERR_STATE, "the stage never loaded a guide");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());
  GuideRowDev r;
  HIP_TRY(hipMemcpy(&r, s->gd.rows + slot, sizeof(r), hipMemcpyDeviceToHost));
  if (guide_id) *guide_id = r.guide < 0 ? -1 : r.guide;
  if (state) *state = r.state;
  if (n_steps) *n_steps = r.n_steps;
  if (n_rejected) *n_rejected = r.n_rejected;
  return BS_OK;
}

// The scratch of a verify-draw pass (first use) and, when the pass has no other device logits to write, its own
// logits buffer (first such use).
static int verify_draw_buffers(bs_stage* s, bool need_logits) {
  if (!s->vd.draw) {
    size_t off[7];
    const size_t bytes = row_sample_verify_bytes(off);
    char* base = nullptr;
    int rc = sampler_scratch(s, bytes, "verify-draw sampler scratch", &base);
    if (rc != BS_OK) return rc;
    s->owned.push_back({base, bytes});
    s->vd = row_sample_verify_bufs(s->rs, base, off);
  }
  if (need_logits && !s->vd_logits) {
    const size_t lb = (size_t)std::max(s->d.max_batch, kVerifyMaxTokens) * s->d.vocab * 4;
    if (!owned_alloc(s, lb, true, (void**)&s->vd_logits))
      return fail(BS_ERR_OOM, "verify-draw logits allocation failed (" + std::to_string(lb) + " B)");
  }
  return BS_OK;
}

extern "C" int bs_read_verify_draw(bs_stage* s, int32_t slot, int32_t t, bs_row_draw* out) {
  if (!s || !out) return fail(BS_ERR_INVALID, "stage/out is NULL");
  if (!s->vd_last_B) return fail(BS_ERR_STATE, "the stage never ran a verify-draw pass");
  if (slot < s->vd_last_slot || slot >= s->vd_last_slot + s->vd_last_B || t < 0 || t >= s->vd_last_S)
    return fail(BS_ERR_INVALID, "row or position outside the last verify-draw pass");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, s->vd.draw + (size_t)(slot - s->vd_last_slot) * s->vd_last_S + t, sizeof(*out),
                    hipMemcpyDeviceToHost));
  return BS_OK;
}

extern "C" int bs_set_graphs(bs_stage* s, int32_t on) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  HIP_TRY(hipSetDevice(s->d.device));
  int rc = drop_graphs(s);
  if (rc == BS_OK) s->graphs_on = on ? 1 : 0;
  return rc;
}

extern "C" int bs_set_head_screen(bs_stage* s, int32_t on) {
  if (!s) return fail(BS_ERR_INVALID, "stage is NULL");
  if (on && !s->hs.Q) return fail(BS_ERR_STATE, "stage holds no head shadow copy (bf16 last stage with the whole lm_head)");
  HIP_TRY(hipSetDevice(s->d.device));
  int rc = drop_graphs(s);  // they hold the old tail
  if (rc == BS_OK) s->hs_on = on ? 1 : 0;
  return rc;
}

extern "C" int bs_read_head_screen(bs_stage* s, int32_t row, float* hilo, float* lstar, int32_t* list, int32_t* count) {
  if (!s || !count) return fail(BS_ERR_INVALID, "stage/count is NULL");
  if (s->hs_last_rows <= 0) { *count = -1; return BS_OK; }  // the last forward took the full head
  if (row < 0 || row >= s->hs_last_rows) return fail(BS_ERR_INVALID, "row outside the last forward");
  HIP_TRY(hipSetDevice(s->d.device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t nt = (size_t)s->d.vocab / 16;
  if (hilo) HIP_TRY(hipMemcpy(hilo, s->hs.hilo + (size_t)row * nt * 2, nt * 8, hipMemcpyDeviceToHost));
  if (lstar) HIP_TRY(hipMemcpy(lstar, s->hs.lstar + row, 4, hipMemcpyDeviceToHost));
  if (list) HIP_TRY(hipMemcpy(list, s->hs.list + (size_t)row * nt, nt * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(count, s->hs.count + row, 4, hipMemcpyDeviceToHost));
  return BS_OK;
}

// The buffers of a top-k pass (first use): slice partials + host-I/O staging, and the [max_batch][vocab] logits buffer
// if no sampler has made it (then it counts as workspace, as in row_sampler_buffers).
static int topk_buffers(bs_stage* s) {
  if (s->tk_pmax) return BS_OK;
  const size_t mb = s->d.max_batch, ns = topk_slices(s->d.vocab);
  Carver c;
  c.piece(&s->tk_pmax, mb * ns * 4);
  c.piece(&s->tk_psum, mb * ns * 4);
  c.piece(&s->tk_pkeys, mb * ns * kTopkMaxK * 8);
  c.piece(&s->tk_ids, mb * kTopkMaxK * 4);
  c.piece(&s->tk_lp, mb * kTopkMaxK * 4);
  c.piece(&s->tk_lse, mb * 4);
  if (c.alloc() != Carver::OK) return fail(BS_ERR_OOM, "top-k buffers allocation failed (" + std::to_string(c.total) + " B)");
  if (!s->sample_logits && !owned_alloc(s, mb * s->d.vocab * 4, true, (void**)&s->sample_logits)) {
    hipFree(c.base);
    s->tk_pmax = nullptr;
    return fail(BS_ERR_OOM, "top-k logits allocation failed");
  }
  s->owned.push_back({c.base, c.total});
  return BS_OK;
}

// bs_forward and bs_forward_score (sc non-null): argument checks, the rows' positions on the device, the enqueue
// (captured or eager) and the bookkeeping of what the pass's last kernel left in past_dev.
static int forward_impl(bs_stage* s, const bs_step* step, const void* in, void* out, float* logits, const ScoreIO* sc,
                        void* stream, const TopkIO* tk = nullptr) {
  if (!s || !step) return fail(BS_ERR_INVALID, "stage/step is NULL");
  const bs_stage_desc& d = s->d;
  const int B = step->batch, S = step->seq, slot = step->slot;
  const int M = B * S;
  if (B <= 0 || S <= 0) return fail(BS_ERR_INVALID, "batch and seq must be positive");
  if (slot < 0 || slot + B > d.max_batch) return fail(BS_ERR_INVALID, "slot range outside max_batch");
  std::vector<int> pasts(B);
  for (int b = 0; b < B; b++) {
    pasts[b] = step->past_lens ? step->past_lens[b] : step->past_len;
    if (pasts[b] < 0 || pasts[b] + S > d.max_ctx) return fail(BS_ERR_INVALID, "past_len + seq exceeds max_ctx");
  }
  if (M > d.max_tokens) return fail(BS_ERR_INVALID, "batch*seq exceeds max_tokens");
  if (s->kv8 && S > 1 && s->L > 0) {  // every row's past and new positions side by side in the bf16 staging
    const size_t need = (size_t)B * (*std::max_element(pasts.begin(), pasts.end()) + S);
    if (need > s->kv_stage_cap)
      return fail(BS_ERR_UNSUPPORTED, "int8 KV: batch * (longest past_len + seq) = " + std::to_string(need) +
                                          " positions exceed the staging capacity of " +
                                          std::to_string(s->kv_stage_cap) + " (max(max_tokens, max_ctx))");
  }
  const bool verify = (step->flags & BS_STEP_VERIFY) != 0;
  const bool draw = (step->flags & BS_STEP_VERIFY_DRAW) != 0;
  if (draw && (sc || !verify))
    return fail(BS_ERR_INVALID, "BS_STEP_VERIFY_DRAW is valid only together with BS_STEP_VERIFY on bs_forward");
  if (verify) {
    if (sc) return fail(BS_ERR_INVALID, "BS_STEP_VERIFY is not valid for a scoring pass");
    if (S < 2 || S > 8 || M > kVerifyMaxTokens)
      return fail(BS_ERR_INVALID, "a verify pass needs 2 <= seq <= 8 and batch * seq <= 32");
    if (s->kv8) return fail(BS_ERR_UNSUPPORTED, "BS_STEP_VERIFY on an int8 KV cache is not supported");
    if (s->hd > 128) return fail(BS_ERR_UNSUPPORTED, "BS_STEP_VERIFY needs head_dim <= 128");
    if (s->n_labels) return fail(BS_ERR_STATE, "BS_STEP_VERIFY on a classifier stage");
    if (s->top_k > 1) return fail(BS_ERR_STATE, "BS_STEP_VERIFY needs the greedy pick (bs_set_sampling top_k <= 1)");
    if (d.is_last && (!s->wemb || s->hv0 != 0 || s->hv1 != d.vocab))
      return fail(BS_ERR_STATE, "BS_STEP_VERIFY on a last stage needs the whole lm_head");
    if (!draw && rows_sampled(s, slot, B))
      return fail(BS_ERR_STATE, "BS_STEP_VERIFY on a row that holds sampler state (BS_STEP_VERIFY_DRAW draws from it)");
  }
  if (!in || (!out && !sc && !tk)) return fail(BS_ERR_INVALID, "in/out is NULL");
  if (tk && rows_sampled(s, slot, B)) return fail(BS_ERR_STATE, "bs_forward_topk on a row that holds sampler state");
  if (!sc && (tk || verify) && rows_processed(s, slot, B))
    return fail(BS_ERR_STATE, "bs_forward_topk / BS_STEP_VERIFY on a row that holds logit processor state");
  if (!sc && (tk || verify) && rows_guided(s, slot, B))
    return fail(BS_ERR_STATE, "bs_forward_topk / BS_STEP_VERIFY on a row that holds guide state");
  const bool want_logits = (step->flags & BS_STEP_LOGITS) != 0;
  if (want_logits && (!d.is_last || !logits)) return fail(BS_ERR_INVALID, "logits requested on a non-last stage or NULL");
  const bool host_io = (step->flags & BS_STEP_HOST_IO) != 0;
  if (d.is_first && host_io) {
    const int* ids = (const int*)in;
    for (int i = 0; i < M; i++)
      if (ids[i] < 0 || ids[i] >= d.vocab) return fail(BS_ERR_INVALID, "token id out of range");
  }
  BS_TRACE("B=%d S=%d slot=%d flags=%u stream=%p hipSetDevice", B, S, slot, (unsigned)step->flags, stream);
  HIP_TRY(hipSetDevice(d.device));
  hipStream_t st = stream ? (hipStream_t)stream : s->own;
  // ---- what the pass ends in, and the buffers its attention and that tail need, made before any capture
  const Tail tail = plan_tail(s, step, sc != nullptr, tk != nullptr);
  if (verify && !s->vf_acc) {  // first verify call: split partials of the attention, keys and ids of every position
    const int stride = attention_verify_split_stride(d.n_head, s->max_chunks);
    Carver c;
    c.piece(&s->vf_acc, (size_t)kVerifyMaxTokens * d.n_head * stride * s->hd * 4);
    c.piece(&s->vf_ml, (size_t)kVerifyMaxTokens * d.n_head * stride * 2 * 4);
    c.piece(&s->vf_keys, d.is_last ? (size_t)kVerifyMaxTokens * (d.vocab / 16) * 8 : 0);
    c.piece(&s->vf_tok, (size_t)kVerifyMaxTokens * 4);
    if (c.alloc() != Carver::OK)
      return fail(BS_ERR_OOM, "verify buffers allocation failed (" + std::to_string(c.total) + " B)");
    s->owned.push_back({c.base, c.total});
    s->vf_stride = stride;
  }
  if (tail.kind == TAIL_TOPK_LOGPROBS) {
    int rc = topk_buffers(s);
    if (rc != BS_OK) return rc;
  }
  if (tail.kind == TAIL_VERIFY_DRAW) {
    int rc = verify_draw_buffers(s, !want_logits);  // host-I/O logits go through the logits staging
    if (rc != BS_OK) return rc;
  }

  // Decode steps and verify passes on device buffers replay a captured hipGraph: the kernels read past_len from
  // device memory, set by one small kernel ahead of the replay -- unless the last forward (a last
  // stage's, whose token pick advances past_dev by its seq) already left exactly these values there,
  // on this same stream: a forward on another stream is not ordered behind that advance, so it always
  // writes its own positions.
  const bool past_matches = s->past_next_valid && s->past_stream == st && (int)s->past_next.size() == B &&
                            std::equal(pasts.begin(), pasts.end(), s->past_next.begin());
  s->past_next_valid = false;  // until this forward is enqueued
  const bool graph = (S == 1 || verify) && !host_io && s->prof.cls == 0 && s->graphs_on && !sc;  // scoring is always eager
  hipGraphExec_t exec = nullptr;
  GraphKey key{B, S, slot, step->flags, tail.kind, in, out, logits, st};
  if (tk) { key.out = tk->ids; key.logits = tk->logits; key.k = tk->k; key.logprobs = tk->logprobs; key.lse = tk->lse; }
  if (graph && !(exec = find_graph(s, key))) {
    hipGraph_t gr = nullptr;
    BS_TRACE("hipStreamBeginCapture");
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    BS_TRACE("enqueue_forward (capturing)");
    int rc = enqueue_forward(s, step, tail, in, out, logits, st, s->past_dev, pasts, nullptr, tk);
    BS_TRACE("hipStreamEndCapture");
    hipError_t ce = hipStreamEndCapture(st, &gr);
    if (rc != BS_OK) { if (gr) hipGraphDestroy(gr); return rc; }
    if (ce != hipSuccess) return fail(BS_ERR_DEVICE, std::string("graph capture: ") + hipGetErrorString(ce));
    BS_TRACE("hipGraphInstantiate");
    hipError_t ie = hipGraphInstantiate(&exec, gr, nullptr, nullptr, 0);
    BS_TRACE("hipGraphDestroy");
    hipGraphDestroy(gr);
    if (ie != hipSuccess) return fail(BS_ERR_DEVICE, std::string("graph instantiate: ") + hipGetErrorString(ie));
    if ((rc = insert_graph(s, key, exec)) != BS_OK) return rc;
  }
  if (!past_matches) {
    BS_TRACE("set_past launch");
    launch_set_past(s->past_dev, pasts.data(), B, st);
  }
  if (exec) {
    BS_TRACE("hipGraphLaunch");
    HIP_TRY(hipGraphLaunch(exec, st));
  } else {
    BS_TRACE("enqueue_forward (eager)");
    int rc = enqueue_forward(s, step, tail, in, out, logits, st, s->past_dev, pasts, sc, tk);
    if (rc != BS_OK) return rc;
  }
  BS_TRACE("hipGetLastError");
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BS_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(err));
  s->hs_last_rows = tail.kind == TAIL_SCREENED ? B : 0;
  if (tail.kind == TAIL_VERIFY_DRAW) { s->vd_last_slot = slot; s->vd_last_B = B; s->vd_last_S = S; }
  if (tail.kind == TAIL_ROWS_PROC || tail.kind == TAIL_ROWS_GUIDE)  // the note launch appended one pick to every row with state
    for (int b = 0; b < B; b++)
      if (s->lp_host[slot + b].active) s->lp_host[slot + b].len = std::min(s->lp_host[slot + b].len + 1, s->lp.cap);
  if (d.is_last) {  // the last kernel advanced past_dev[0..B) by S (stream-ordered before the next forward)
    s->past_next.assign(pasts.begin(), pasts.end());
    for (int& p : s->past_next) p += S;
    s->past_next_valid = true;
    s->past_stream = st;
  }
  if (host_io) {
    BS_TRACE("hipStreamSynchronize");
    HIP_TRY(hipStreamSynchronize(st));
  }
  BS_TRACE("done");
  return BS_OK;
}

extern "C" int bs_forward(bs_stage* s, const bs_step* step, const void* in, void* out, float* logits, void* stream) {
  return forward_impl(s, step, in, out, logits, nullptr, stream);
}

extern "C" int bs_forward_score(bs_stage* s, const bs_step* step, const void* in, const int32_t* targets,
                                int32_t* top_ids, float* scores, void* stream) {
  if (!s || !step) return fail(BS_ERR_INVALID, "stage/step is NULL");
  const bs_stage_desc& d = s->d;
  if (!d.is_last || s->n_labels || !s->wemb)
    return fail(BS_ERR_STATE, "scoring needs the last stage of a generation model (ln_f + the whole lm_head)");
  if (!s->bf16) return fail(BS_ERR_UNSUPPORTED, "scoring needs a BFLOAT16 stage");
  if (step->flags & BS_STEP_LOGITS) return fail(BS_ERR_INVALID, "BS_STEP_LOGITS is not valid for a scoring pass");
  if (!top_ids && !scores) return fail(BS_ERR_INVALID, "top_ids and scores are both NULL");
  HIP_TRY(hipSetDevice(d.device));
  if (!s->sc_parts) {  // first scoring call: partials for the largest pass + host-I/O staging
    if (s->cus <= 0) HIP_TRY(hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, d.device));
    const size_t T = d.max_tokens;
    size_t pb = 0;
    for (size_t m = 128; m < T + 128; m += 128)  // the splits shrink as the row tiles grow
      pb = std::max(pb, head_score_partial_bytes((int)std::min(m, T), d.vocab, s->cus));
    Carver c;
    c.piece(&s->sc_parts, pb);
    c.piece(&s->sc_targets, T * 4);
    c.piece(&s->sc_top, T * 4);
    c.piece(&s->sc_scores, T * 12);
    if (c.alloc() != Carver::OK)
      return fail(BS_ERR_OOM, "scoring buffers allocation failed (" + std::to_string(c.total) + " B)");
    s->owned.push_back({c.base, c.total});
  }
  const ScoreIO sc{targets, top_ids, scores};
  return forward_impl(s, step, in, nullptr, nullptr, &sc, stream);
}

// The top-k log-prob tail (beam_topk.hip): argument and state checks, then a forward whose tail is
// TAIL_TOPK_LOGPROBS (forward_impl makes the buffers of the first call after its own checks, before any capture).
extern "C" int bs_forward_topk(bs_stage* s, const bs_step* step, const void* in, int32_t k, int32_t* ids, float* logprobs,
                               float* lse, float* logits, void* stream) {
  if (!s || !step) return fail(BS_ERR_INVALID, "stage/step is NULL");
  const bs_stage_desc& d = s->d;
  if (k < 1 || k > kTopkMaxK) return fail(BS_ERR_INVALID, "k must be in [1, 16]");
  if (!ids || !logprobs) return fail(BS_ERR_INVALID, "ids/logprobs is NULL");
  if (step->flags & (BS_STEP_VERIFY | BS_STEP_VERIFY_DRAW | BS_STEP_LOGITS))
    return fail(BS_ERR_INVALID, "BS_STEP_VERIFY, BS_STEP_VERIFY_DRAW and BS_STEP_LOGITS are not valid for a top-k pass "
                                "(the logits pointer says whether logits are wanted)");
  if (!(step->flags & BS_STEP_HOST_IO) && logits && ((uintptr_t)logits & 15))
    return fail(BS_ERR_INVALID, "device logits must be 16-byte aligned");
  if (s->n_labels) return fail(BS_ERR_STATE, "bs_forward_topk on a classifier stage");
  if (!d.is_last || !s->wemb || s->hv0 != 0 || s->hv1 != d.vocab)
    return fail(BS_ERR_STATE, "bs_forward_topk needs the last stage of a generation model (ln_f + the whole lm_head)");
  if (s->top_k > 1) return fail(BS_ERR_STATE, "bs_forward_topk needs the greedy pick (bs_set_sampling top_k <= 1)");
  if (topk_slices(d.vocab) > kTopkMaxSlices) return fail(BS_ERR_UNSUPPORTED, "vocab too large for the top-k tail");
  HIP_TRY(hipSetDevice(d.device));
  const TopkIO tk{k, ids, logprobs, lse, logits};
  return forward_impl(s, step, in, nullptr, nullptr, nullptr, stream, &tk);
}
