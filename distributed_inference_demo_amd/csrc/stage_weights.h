// stage_weights.h — the canonical weight order of a stage, from its bs_stage_desc alone (plain host C++).
//
// weight_table() is the one place that knows which tensors a stage holds and in which order: the BS_WEIGHTS_HOST
// layout, the arena order, the checkpoint names and shapes, and the synthetic-fill keys all come from walking it
// (stage.hip: bs_stage_weight_count, bs_init_stage_file's pre-device check, init_stage, bs_read_weights).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bloomstage.h"

enum { T_LN1_G, T_LN1_B, T_QKV_W, T_QKV_B, T_DENSE_W, T_DENSE_B, T_LN2_G, T_LN2_B, T_FC1_W, T_FC1_B,
       T_FC2_W, T_FC2_B, T_NLAYER };
// model tensors; M_HEAD is a head slice held on its own (rows of the embedding a stage does not own)
enum { M_WEMB = 0, M_EMB_G = 1, M_EMB_B = 2, M_LNF_G = 3, M_LNF_B = 4, M_SCORE = 5, M_HEAD = 6 };

static inline uint64_t host_sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static inline uint64_t tensor_key(uint64_t seed, int layer, uint32_t tid) {
  return host_sm64(seed ^ host_sm64(((uint64_t)(uint32_t)(layer + 1) << 8) | tid));
}

// Does the stage hold the whole word embedding (the first stage gathers from it, a generation model's last stage
// ties its lm_head to it)?
static inline bool owns_embedding(const bs_stage_desc* d) {
  return d->is_first || (d->is_last && !(d->flags & BS_FLAG_CLASSIFIER));
}
static inline bool has_head_slice(const bs_stage_desc* d) { return d->head_vocab_end > d->head_vocab_begin; }

struct WeightEntry {
  int layer;                   // -1: a model tensor (tid is an M_*), else the stage's layer index (tid is a T_*)
  int tid;
  uint64_t count;              // elements (what the tensor takes of the BS_WEIGHTS_HOST buffer)
  int N, K;                    // the four block matrices: [N][K] (the int8 / MXFP4 formats apply); else 0
  std::string name;            // checkpoint tensor (HF BloomModel names, modeling_bloom.py)
  std::vector<int64_t> shape;  // the checkpoint tensor's expected shape
  uint64_t first;              // first element inside the checkpoint tensor and the synthetic stream (head slice rows)
  uint64_t key;                // synthetic fill: the generator key and the kind of values
  int kind;                    // 0 matrix, 1 bias, 2 LayerNorm gain, 3 LayerNorm bias
  // where init_stage put it: the values (or the int8 / E2M1 codes), the int8 row scales, the MXFP4 block scales
  void* data = nullptr;
  float* row_scale = nullptr;
  uint8_t* blk_scale = nullptr;
  bool quantised() const { return row_scale || blk_scale; }
};

static inline std::vector<WeightEntry> weight_table(const bs_stage_desc* d) {
  const int64_t h = d->hidden, V = d->vocab;
  std::vector<WeightEntry> w;
  auto model = [&](int tid, const char* name, std::vector<int64_t> shape, uint64_t count, int key_tid, int kind,
                   uint64_t first = 0) {
    w.push_back({-1, tid, count, 0, 0, name, std::move(shape), first, tensor_key(d->seed, -1, key_tid), kind});
  };
  auto ln_f = [&] {
    model(M_LNF_G, "ln_f.weight", {h}, h, M_LNF_G, 2);
    model(M_LNF_B, "ln_f.bias", {h}, h, M_LNF_B, 3);
  };
  if (owns_embedding(d)) model(M_WEMB, "word_embeddings.weight", {V, h}, V * h, M_WEMB, 0);
  if (d->is_first) {
    model(M_EMB_G, "word_embeddings_layernorm.weight", {h}, h, M_EMB_G, 2);
    model(M_EMB_B, "word_embeddings_layernorm.bias", {h}, h, M_EMB_B, 3);
  }
  struct { const char* name; int64_t n, k; int kind; } const lt[T_NLAYER] = {  // k == 0: a vector of n
      {"input_layernorm.weight", h, 0, 2},           {"input_layernorm.bias", h, 0, 3},
      {"self_attention.query_key_value.weight", 3 * h, h, 0}, {"self_attention.query_key_value.bias", 3 * h, 0, 1},
      {"self_attention.dense.weight", h, h, 0},      {"self_attention.dense.bias", h, 0, 1},
      {"post_attention_layernorm.weight", h, 0, 2},  {"post_attention_layernorm.bias", h, 0, 3},
      {"mlp.dense_h_to_4h.weight", 4 * h, h, 0},     {"mlp.dense_h_to_4h.bias", 4 * h, 0, 1},
      {"mlp.dense_4h_to_h.weight", h, 4 * h, 0},     {"mlp.dense_4h_to_h.bias", h, 0, 1}};
  for (int l = d->layer_begin; l < d->layer_end; l++)
    for (int t = 0; t < T_NLAYER; t++) {
      const auto& e = lt[t];
      std::vector<int64_t> shape = e.k ? std::vector<int64_t>{e.n, e.k} : std::vector<int64_t>{e.n};
      w.push_back({l - d->layer_begin, t, (uint64_t)(e.k ? e.n * e.k : e.n), (int)(e.k ? e.n : 0), (int)e.k,
                   "h." + std::to_string(l) + "." + e.name, std::move(shape), 0, tensor_key(d->seed, l, t), e.kind});
    }
  if (d->is_last) ln_f();
  if (d->flags & BS_FLAG_CLASSIFIER)  // BloomForSequenceClassification.score
    model(M_SCORE, "score.weight", {(int64_t)d->n_labels, h}, (uint64_t)d->n_labels * h, M_SCORE, 0);
  if (has_head_slice(d)) {  // a stage that owns the embedding takes its slice from there
    if (!owns_embedding(d))
      model(M_HEAD, "word_embeddings.weight", {V, h}, (uint64_t)(d->head_vocab_end - d->head_vocab_begin) * h, M_WEMB,
            0, (uint64_t)d->head_vocab_begin * h);
    if (!d->is_last) ln_f();
  }
  return w;
}
