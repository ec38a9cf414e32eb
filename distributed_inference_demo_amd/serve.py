"""serve.py — the reference's server/client run on one node.

Reference: `server.py:893-1042` builds the run config {num_sample, max_length, core_pool_size,
num_device, graph, ...}, places contiguous layer ranges with `round_robin_module_arrangement`
(`server.py:893-905`) and drives every device through Ready -> Running -> Finish -> Close
(`Client.java:50-173`); on each device `Communication.running` (`Communication.java:389-470`) keeps
`core_pool_size` samples in flight until `num_sample` samples are done, and every sample produces
`max_length` tokens, one pipeline round each (`Communication.java:621-651`).

Here: one process per GPU (torchrun), rank r = device r of the graph, layers from the same
placement (`placement.stage_ranges`).  Lifecycle:
  init   — RunConfig -> this rank's stage + Pipeline (`pipeline.build_rank`); the `core_pool_size`
           samples in flight = min(pool, stages) micro-batches x the rest as rows, every row a KV slot
           holding one sample at its own position (bs_step.past_lens), so every stage computes while
           the hops overlap;
  run    — continuous admission (Communication.java:418-464: a new sample starts as soon as one in
           flight finishes): a row takes the next sample the round its previous sample produced its
           `max_length`-th token.  The admitted sample's whole prompt goes through the stages as one
           prefill pass of that row (S = len(prompt) at its KV slot, Pipeline.prefill_row) just before
           the decode round, which it joins with its first generated token; decode rounds are S = 1 for
           every row, each at its own position.  (prefill=False feeds the prompt one token a round, as
           the reference header does, Communication.java:322-326.)  Prompts may have different lengths.
           The admission schedule depends only on the prompt lengths, so every rank derives the same
           per-row positions and prefill passes;
  finish — rank 0 returns every sample's `max_length` greedy token ids and the run's tokens/s.
max_length == 0 is the classification task (Communication.java:591-603: one OneStep pass per sample, the
last device's classifier tail, binaryClassify at Communication.java:532-534): the last stage holds a
score head of `n_labels` labels (BS_FLAG_CLASSIFIER), samples of equal prompt length go through
together, `core_pool_size` rows a pass, and rank 0 returns each sample's class id (first maximal label).
--score is the scoring task (no counterpart in the reference): every sample's prompt is one teacher-forced pass
(pipeline.score, bs_forward_score on the last stage), `core_pool_size` samples a pass, and rank 0 returns each
sample's summed log-likelihood, token count and perplexity.
--speculate K is speculative decoding on one GPU (speculative.py; no counterpart in the reference): the samples are
decoded one after another in KV row 0, a drafter (--draft ngram: prompt lookup; --draft MODEL: a draft model with the
same vocabulary, e.g. the target's "-int8" variant) proposes up to K tokens a round and one BS_STEP_VERIFY pass of
the target emits the agreeing prefix plus one token.  The tokens are plain greedy decoding's; rank 0 also returns
the acceptance statistics.  One stage only: the ranks of a pipeline derive their schedule from the prompt lengths
alone, and how many tokens a pass accepts depends on the data.
--sample is per-row nucleus sampling (bs_set_row_sampler; the reference's tail draws an unseeded top-k sample,
decoding.cpp:24-66): the last rank gives the row a sample is admitted into the state (--top-k, --top-p, --temperature,
request_seed(--sample-seed, sample id)) just before the sample's prefill pass, so its first generated token is already
sampled.  A draw depends on (seed, position, logits) only, never on the row.  The whole lm_head stays on the last
stage (no head ring).
--sample --sample-speculate K is sampled speculative decoding on one GPU: --speculate's loop with the row's sampler
state set before each sample's prefill and verify passes that return the row's own draw at every position
(BS_STEP_VERIFY_DRAW).  The tokens are plain sampled decoding's for the same state and seed; a draft model holds the
same state, so it draws with the target's u at every position.
--shared-prefix P: the first P tokens of every prompt are the same (a system prompt, few-shot examples) and are
prefilled once, into a template KV row behind the pool's rows; an admitted sample forks the template into its row
(bs_fork_kv, a device copy of the P cached positions on every rank) and prefills only the rest of its prompt at
past = P.  The schedule is unchanged.  --prefix-fork 0 is the A/B baseline: every sample prefills the prefix in its own
row with a pass of the same shape, then the rest, so both settings return the same tokens.
--num-beams W is beam search on one GPU (beam.py; no counterpart in the reference): the samples are decoded one after
another in KV rows [0, W) of the whole model as one stage; every step is one top-k log-prob pass (bs_forward_topk, the
2W best tokens of each hypothesis), the selection of transformers' generate(num_beams=W) on the host (--length-penalty,
--eos-id) and one bs_copy_kv call that hands the rows of dead hypotheses to the children of living ones.  Rank 0
returns each sample's best hypothesis, its score and the number of KV row pairs copied.
--repetition-penalty R, --no-repeat-ngram-size N, --min-new-tokens M (with --eos-id), --bad-token ID and --token-bias
ID:VALUE (both repeatable) are the per-row logit processors (bs_set_row_processor; transformers'
repetition_penalty, no_repeat_ngram_size, min_new_tokens, length-1 bad_words_ids and sequence_bias): at admission the
last rank gives the sample's row the state and notes the sample's whole prompt (a shared prefix included) as the row's
token history, just before the prefill pass that yields the first generated token; from then on the device notes its
own picks.  The last rank holds the prompts (they are broadcast once at start when world > 1) and the whole lm_head.
They combine with --sample (the processed logits are what the sampler draws from), --shared-prefix, --kv int8 and
int8 / MXFP4 weights.
--guide-file PATH (a JSON token automaton, guide.Guide.to_json) or --choice "ID,ID,..." (repeatable, with --eos-id: the
sample generates exactly one of the sequences, then only the EOS) is guided decoding (bs_set_row_guide, DESIGN.md §5k;
transformers' prefix_allowed_tokens_fn): the last rank loads the guide once and, at admission, sets the sample's row to
the guide's start state just before the prefill pass, so the guide sees generated tokens only (never the prompt or a
shared prefix); from then on the device masks the logits ahead of the pick and steps the state behind it.  Each
sample's record gains the guide's final state, the count of rejected picks and the index of the first EOS.  Combines
with --sample, the logit processor options, --shared-prefix, --kv int8 and int8 / MXFP4 weights.
Differences from the reference, by design: full-context decode (the reference
header feeds only the last token), argmax (or, with --sample, seeded per-request top-k / top-p sampling) instead of
unseeded top-k, token ids in (no tokenizer).

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29512 \\
      -m distributed_inference_demo_amd.serve --model bloom-560m --num-sample 8 --max-length 40 \\
      --core-pool-size 2
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch
import torch.distributed as dist

from . import config
from .pipeline import build_rank, init_distributed

STATES = ("Ready", "Running", "Finish", "Close")  # Client.java status strings, in order
M64 = (1 << 64) - 1


@dataclasses.dataclass
class RunConfig:
    """The run config of server.py:998-1013 that shapes the computation."""
    model: str = "bloom-560m"
    num_sample: int = 8
    max_length: int = 40          # tokens generated per sample; 0 = the classification task
    core_pool_size: int = 1       # samples in flight
    n_labels: int = 2             # classification: score-head labels (the reference's binary classifier)
    prompt_len: int = 16          # synthetic prompts (token ids U[0, V), seed 1234 + sample id)
    dtype: str = "bf16"
    seed: int = 0                 # weight generator seed
    head_split: bool = True       # vocabulary-parallel lm_head ring when world > 1
    prefill: bool = True          # an admitted sample's prompt as one prefill pass of its row (else a token a round)
    kv: str = "bf16"              # KV cache storage: "bf16", or "int8" (BS_FLAG_INT8_KV: about half the cache bytes)
    score: bool = False           # the scoring task: each prompt's log-likelihood and perplexity, one pass a sample
    speculate: int = 0            # speculative decoding: tokens drafted per verify pass (0 = off; one GPU only)
    draft: str = "ngram"          # the drafter: "ngram" (prompt lookup) or a draft model's name (same vocabulary)
    sample: bool = False          # per-row nucleus sampling instead of greedy decoding (whole lm_head on the last stage)
    top_k: int = 0                # sampling: keep the top_k largest logits (ties at the k-th kept); 0 = no limit
    top_p: float = 1.0            # sampling: the nucleus' share of the candidates' mass, in (0, 1]
    temperature: float = 1.0      # sampling: > 0
    sample_seed: int = 0          # sampling: sample i draws with request_seed(sample_seed, i)
    sample_speculate: int = 0     # sampled speculative decoding: tokens drafted per verify-draw pass (0 = off; needs sample)
    shared_prefix: int = 0        # the first shared_prefix tokens of every prompt are identical and are prefilled once
    prefix_fork: bool = True      # shared_prefix: fork the template row (else every sample prefills the prefix itself)
    num_beams: int = 0            # beam search: hypotheses per sample (0 = off; one GPU only)
    length_penalty: float = 1.0   # beam search: a finished hypothesis scores sum(log p) / length ** length_penalty
    eos_id: int = -1              # beam search: the token that finishes a hypothesis; min_new_tokens: the banned one (-1 = none)
    repetition_penalty: float = 1.0   # logit processors: seen tokens' logits divided (> 0) / multiplied (< 0); 1 = off
    no_repeat_ngram_size: int = 0     # logit processors: no n-gram of this size twice (0 = off, else 1..32)
    min_new_tokens: int = 0           # logit processors: eos_id is banned for a sample's first min_new_tokens tokens
    bad_token: tuple = ()             # logit processors: banned token ids (at most 64 with token_bias)
    token_bias: tuple = ()            # logit processors: (id, value) pairs or "ID:VALUE" strings, value added to the logit
    guide_file: str = ""              # guided decoding: a JSON token automaton (guide.Guide.to_json) for every sample
    choice: tuple = ()                # guided decoding: token-id sequences ("ID,ID,..." or lists), one is generated, then eos_id

    @property
    def guided(self):
        return bool(self.guide_file or self.choice)

    def make_guide(self, vocab):
        """The run's Guide (None when guided decoding is off), validated against the vocabulary."""
        from . import guide
        if self.choice:
            return guide.from_choices(self.choice, self.eos_id).validate(vocab)
        return guide.Guide.from_file(self.guide_file).validate(vocab) if self.guide_file else None

    @property
    def processors(self):
        """Stage.row_processor's keywords when any logit processor is on, else None."""
        if (self.repetition_penalty == 1.0 and not self.no_repeat_ngram_size and not self.min_new_tokens
                and not self.bad_token and not self.token_bias):
            return None
        return {"repetition_penalty": self.repetition_penalty, "no_repeat_ngram": self.no_repeat_ngram_size,
                "min_new_tokens": self.min_new_tokens, "eos_id": self.eos_id if self.min_new_tokens else -1,
                "bias": list(self.token_bias), "bad_tokens": list(self.bad_token)}

    def __post_init__(self):
        if self.shared_prefix < 0:
            raise ValueError(f"shared_prefix must be >= 0 (got {self.shared_prefix})")
        self.bad_token = tuple(int(t) for t in self.bad_token)
        self.token_bias = tuple((int(str(e).split(":")[0]), float(str(e).split(":")[1])) if isinstance(e, str)
                                else (int(e[0]), float(e[1])) for e in self.token_bias)
        self.choice = tuple(tuple(int(t) for t in (c.split(",") if isinstance(c, str) else c)) for c in self.choice)
        if self.guided:
            if (self.speculate or self.sample_speculate or self.num_beams or self.score or self.max_length <= 0
                    or not self.prefill):
                raise ValueError("guided decoding (guide_file, choice) is plain generation with admission prefills: it "
                                 "excludes speculate, sample_speculate, num_beams, score, max_length == 0 and "
                                 "prefill = False")
            if self.guide_file and self.choice:
                raise ValueError("guide_file and choice exclude each other")
            if self.choice and self.eos_id < 0:
                raise ValueError("choice needs eos_id, the token that follows a finished choice")
            if any(len(c) == 0 or min(c) < 0 for c in self.choice):
                raise ValueError("a choice is a non-empty sequence of token ids")
            self.head_split = False  # the whole lm_head on the last stage, as for sample
        if self.processors:
            if (self.speculate or self.sample_speculate or self.num_beams or self.score or self.max_length <= 0
                    or not self.prefill):
                raise ValueError("the logit processors (repetition_penalty, no_repeat_ngram_size, min_new_tokens, "
                                 "bad_token, token_bias) are plain generation with admission prefills: they exclude "
                                 "speculate, sample_speculate, num_beams, score, max_length == 0 and prefill = False")
            if not 0.0 < self.repetition_penalty < float("inf"):
                raise ValueError(f"repetition_penalty must be positive and finite (got {self.repetition_penalty})")
            if not 0 <= self.no_repeat_ngram_size <= 32:
                raise ValueError(f"no_repeat_ngram_size must be in [0, 32] (got {self.no_repeat_ngram_size})")
            if self.min_new_tokens < 0 or (self.min_new_tokens and self.eos_id < 0):
                raise ValueError("min_new_tokens must be >= 0 and needs eos_id, the token it bans")
            if len(self.bad_token) + len(self.token_bias) > 64:
                raise ValueError("at most 64 bad_token and token_bias entries together")
            if any(v != v or v == float("inf") for _, v in self.token_bias):
                raise ValueError("a token_bias value must be finite (or -inf: a ban)")
            self.head_split = False  # the whole lm_head on the last stage, as for sample
        if self.shared_prefix:
            if (not self.prefill or self.score or self.max_length <= 0 or self.speculate or self.sample_speculate):
                raise ValueError("shared_prefix is plain generation with admission prefills: it excludes "
                                 "prefill = False, score, max_length == 0, speculate and sample_speculate")
        if self.num_beams:
            if not 1 <= self.num_beams <= 8:
                raise ValueError(f"num_beams must be in [1, 8] (got {self.num_beams}): a top-k pass returns 16 candidates")
            if (self.sample or self.speculate or self.sample_speculate or self.score or self.shared_prefix
                    or self.max_length <= 0):
                raise ValueError("num_beams is beam search, a generation task of its own: it excludes sample, speculate, "
                                 "sample_speculate, score, shared_prefix and max_length <= 0")
            if self.eos_id < -1:
                raise ValueError(f"eos_id must be a token id or -1 for none (got {self.eos_id})")
            if not float("-inf") < self.length_penalty < float("inf"):
                raise ValueError(f"length_penalty must be finite (got {self.length_penalty})")
        if self.kv not in ("bf16", "int8"):
            raise ValueError(f"kv must be 'bf16' or 'int8' (got {self.kv!r})")
        if self.speculate:
            if not 1 <= self.speculate <= 7:
                raise ValueError(f"speculate must be in [1, 7] (got {self.speculate}): a verify pass holds 8 positions")
            if self.kv != "bf16":
                raise ValueError("speculative decoding needs kv = 'bf16' (no verify pass over an int8 KV cache yet)")
            if self.max_length <= 0:
                raise ValueError("speculative decoding is a generation task: max_length must be > 0")
            if self.score:
                raise ValueError("speculative decoding and the scoring task exclude each other")
        if self.sample:
            if self.speculate or self.score or self.max_length <= 0:
                raise ValueError("sample is plain generation: it excludes speculate, score and max_length == 0")
            if not self.prefill:
                raise ValueError("sample needs prefill: a row's sampler is set at admission, before its prefill pass")
            if self.top_k < 0 or not 0.0 < self.top_p <= 1.0 or not 0.0 < self.temperature < float("inf"):
                raise ValueError("sampling needs top_k >= 0, top_p in (0, 1] and a positive finite temperature "
                                 f"(got {self.top_k}, {self.top_p}, {self.temperature})")
            self.head_split = False
        if self.sample_speculate:
            if not self.sample:
                raise ValueError("sample_speculate is sampled speculative decoding: it needs sample (greedy: speculate)")
            if not 1 <= self.sample_speculate <= 7:
                raise ValueError(f"sample_speculate must be in [1, 7] (got {self.sample_speculate}): a verify pass "
                                 "holds 8 positions")
            if self.kv != "bf16":
                raise ValueError("sampled speculative decoding needs kv = 'bf16' (no verify pass over an int8 KV cache yet)")


def request_seed(sample_seed, i):
    """The seed of sample i's draws: a 64-bit splitmix64 mix of (sample_seed, i), so neighbouring sample ids and
    neighbouring base seeds give unrelated streams.  Stable: part of a run's reproducibility."""
    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        return x ^ (x >> 31)
    return mix((int(sample_seed) & M64) ^ mix((int(i) + 1) & M64))


def synthetic_prompts(cfg: RunConfig, vocab):
    """shared_prefix: every sample begins with prompt 0's first shared_prefix tokens."""
    from .stage import prompt_ids
    P = cfg.shared_prefix
    if P and cfg.prompt_len <= P:
        raise ValueError(f"prompt_len ({cfg.prompt_len}) must exceed shared_prefix ({P}): a token of its own per sample")
    out = [prompt_ids(1234 + i, 1, cfg.prompt_len, vocab).reshape(-1).tolist() for i in range(cfg.num_sample)]
    return [out[0][:P] + p[P:] for p in out] if P else out


def admission_schedule(lens, max_length, rows, prefill=True):
    """Row-level continuous admission: sample i (in order) takes the row that frees first (lowest row
    on ties) at the round it frees.
      prefill=True : the sample's whole prompt is one prefill pass of that row just before decode round t0
                     (Pipeline.prefill_row; it yields generated token 1), then it decodes max_length - 1 rounds
                     (tokens 2..max_length); the row frees at t0 + max_length - 1.
      prefill=False: the prompt is fed one token a round (the reference header's single-token feed), so the
                     row is held len(prompt) - 1 + max_length rounds.
    Returns ([(row, t0)] per sample, total decode rounds)."""
    import heapq
    free = [(0, r) for r in range(rows)]
    heapq.heapify(free)
    out = []
    hold = (lambda n: max_length - 1) if prefill else (lambda n: n - 1 + max_length)
    for n in lens:
        t, r = heapq.heappop(free)
        out.append((r, t))
        heapq.heappush(free, (t + hold(n), r))
    return out, max(t + hold(n) for (r, t), n in zip(out, lens))


def run_rank(cfg: RunConfig, rank, world, device, prompts=None, executor_factory=None, log=None):
    """Run the whole job on this rank.  `prompts` (rank 0): num_sample lists of token ids of any
    lengths (None: synthetic).  Returns {"samples": [[max_length ids] per sample], ...} on rank 0,
    None elsewhere.  Collective: every rank calls it with the same cfg."""
    say = log if (log is not None and rank == 0) else (lambda *_: None)
    if (cfg.speculate or cfg.sample_speculate) and world != 1:
        raise ValueError("speculative decoding runs on one stage (world == 1): acceptance is data-dependent, the "
                         "pipeline's schedule is not")
    if cfg.num_beams and world != 1:
        raise ValueError("beam search runs on one stage (world == 1): which rows are copied is data-dependent, the "
                         "pipeline's schedule is not")
    if cfg.sample and executor_factory is not None:
        raise ValueError("sample is the HIP stage's per-row sampler: not available with an executor_factory")
    proc = cfg.processors
    if proc and executor_factory is not None:
        raise ValueError("the logit processors are the HIP stage's: not available with an executor_factory")
    if cfg.guided and executor_factory is not None:
        raise ValueError("guided decoding is the HIP stage's: not available with an executor_factory")
    if cfg.num_sample < 1 or cfg.max_length < 0 or cfg.core_pool_size < 1:
        raise ValueError("num_sample and core_pool_size must be >= 1, max_length >= 0 (0: classification)")
    model = config.get(cfg.model) if isinstance(cfg.model, str) else cfg.model
    if rank == 0:
        prompts = synthetic_prompts(cfg, model.vocab) if prompts is None else [list(p) for p in prompts]
        if len(prompts) != cfg.num_sample:
            raise ValueError(f"{len(prompts)} prompts for num_sample = {cfg.num_sample}")
        if any(len(p) < 1 for p in prompts):
            raise ValueError("every prompt needs at least one token")
        lens = [len(p) for p in prompts]
    else:
        lens = [0] * cfg.num_sample
    P = cfg.shared_prefix
    if P:  # rank 0's verdict on the prefixes travels behind the lengths, so every rank raises together
        lens.append(int(rank == 0 and any(p[:P] != prompts[0][:P] for p in prompts if len(p) > P)))
    if world > 1:  # the prompt lengths travel with the config (server -> devices)
        t = torch.tensor(lens, dtype=torch.int64)
        if dist.get_backend() == "nccl":
            t = t.to(device)
        dist.broadcast(t, src=0)
        lens = [int(v) for v in t.tolist()]
    if P:
        differ = lens.pop()
        if min(lens) <= P:
            raise ValueError(f"shared_prefix = {P}: every prompt must be longer (shortest: {min(lens)}); the "
                             "continuation pass needs a token")
        if differ:
            raise ValueError(f"shared_prefix = {P}: the prompts' first {P} tokens differ")
    if proc:
        if any(not 0 <= t < model.vocab for t in list(cfg.bad_token) + [t for t, _ in cfg.token_bias]):
            raise ValueError(f"a bad_token / token_bias id lies outside the vocabulary ({model.vocab})")
        if cfg.min_new_tokens and cfg.eos_id >= model.vocab:
            raise ValueError(f"eos_id ({cfg.eos_id}) outside the vocabulary ({model.vocab})")
        if world > 1:  # the last rank notes every sample's prompt: the prompts travel once, behind their lengths
            flat = torch.tensor([t for p in prompts for t in p] if rank == 0 else [0] * sum(lens), dtype=torch.int64)
            if dist.get_backend() == "nccl":
                flat = flat.to(device)
            dist.broadcast(flat, src=0)
            if rank == world - 1 and rank != 0:
                flat, prompts, at = flat.tolist(), [], 0
                for n in lens:
                    prompts.append(flat[at:at + n])
                    at += n
    guide = cfg.make_guide(model.vocab)  # every rank reads it; the last loads it, rank 0 walks the results through it
    if cfg.score:
        return _score_run(cfg, model, rank, world, device, prompts, lens, executor_factory, say)
    if cfg.max_length == 0:
        return _classify_run(cfg, model, rank, world, device, prompts, lens, executor_factory, say)
    if cfg.speculate or cfg.sample_speculate:
        return _spec_run(cfg, model, device, prompts, lens, say)
    if cfg.num_beams:
        return _beam_run(cfg, model, device, prompts, lens, say)
    # samples in flight = n_mb micro-batches x mb rows: one micro-batch per stage keeps every stage
    # busy; the rest of the pool rides as rows of a micro-batch (one GPU: one batched decode)
    n_mb = min(cfg.core_pool_size, world)
    mb = -(-cfg.core_pool_size // n_mb)
    rows = n_mb * mb
    pf = cfg.prefill
    fork = bool(P) and cfg.prefix_fork  # the prefix is prefilled once into a template row and forked at admission
    sched, T = admission_schedule(lens, cfg.max_length, rows, prefill=pf)
    # per decode round and row: position, and (rank 0) the fed token / whether it overrides the returned one;
    # with prefill, `take_pf` marks a sample's first decode round, whose input is its prefill's token
    pos = [[0] * rows for _ in range(T)]
    feed_tok = [[0] * rows for _ in range(T)]
    feed_mask = [[True] * rows for _ in range(T)]
    take_pf = [[False] * rows for _ in range(T)]
    admit = [[] for _ in range(T + 1)]  # prefill passes before decode round t: (sample, row)
    for i, ((r, t0), n) in enumerate(zip(sched, lens)):
        if pf:
            admit[t0].append((i, r))
            for t in range(t0, t0 + cfg.max_length - 1):
                pos[t][r] = n + (t - t0)
                feed_mask[t][r] = t == t0
                take_pf[t][r] = t == t0
        else:
            for t in range(t0, t0 + n - 1 + cfg.max_length):
                pos[t][r] = t - t0
                if t - t0 < n:
                    feed_tok[t][r] = prompts[i][t - t0] if rank == 0 else 0
                else:
                    feed_mask[t][r] = False
    # ---- init (Ready)
    max_seq = -(-max(lens) // mb) if pf else 1  # a prefill pass of one row fits a micro-batch's hop buffers
    pipe, (lb, le) = build_rank(model, rank, world, device, dtype=cfg.dtype, mb_rows=mb, n_mb=n_mb,
                                max_ctx=max(lens) + cfg.max_length + 1, max_seq=max_seq, seed=cfg.seed,
                                head_split=cfg.head_split, executor_factory=executor_factory,
                                kv_int8=cfg.kv == "int8", sample=cfg.sample or bool(proc) or cfg.guided,
                                extra_rows=int(fork))
    guide_id = pipe.load_guide(guide) if guide is not None else None  # once, outside the decode loop (last rank)
    say(STATES[0], {"rank_layers": [lb, le], "stages": world, "core_pool_size": cfg.core_pool_size,
                    "micro_batches": n_mb, "rows_per_micro_batch": mb, "rounds": T, "prefill": pf,
                    **({"shared_prefix": P, "prefix_fork": fork} if P else {})})
    sampling = ({"top_k": cfg.top_k, "top_p": cfg.top_p, "temperature": cfg.temperature} if cfg.sample else None)
    cuda = device.type == "cuda"
    if cuda:
        torch.cuda.set_stream(torch.cuda.Stream(device))  # decode steps are captured as hipGraphs
    shape = (max(T, 1), n_mb, mb)
    ft = torch.tensor(feed_tok or [[0] * rows], dtype=torch.int32, device=device).view(shape)
    fm = torch.tensor(feed_mask or [[True] * rows], dtype=torch.bool, device=device).view(shape)
    tp = torch.tensor(take_pf or [[False] * rows], dtype=torch.bool, device=device).view(shape)
    pids = ([torch.tensor(p, dtype=torch.int32, device=device).view(1, -1) for p in prompts]
            if (pf and rank == 0) else None)
    # shared_prefix: each prompt as (prefix, rest) views (rank 0)
    pre = [p[:, :P] if pids is not None else None for p in (pids or [None] * cfg.num_sample)] if P else None
    rest = [p[:, P:] if pids is not None else None for p in (pids or [None] * cfg.num_sample)] if P else None
    if world > 1:
        dist.barrier()
    # ---- run (Running)
    say(STATES[1], {"num_sample": cfg.num_sample, "max_length": cfg.max_length})
    rec = [[] for _ in range(n_mb)] if pipe.is_first else None
    first = [None] * cfg.num_sample  # prefill: each sample's first generated token (rank 0)
    pipe.tokens_held = True  # round 0 feeds every row
    prefill_tokens = 0
    t_start = time.perf_counter()
    if fork:  # the template: one ordinary prefill pass of the shared prefix into the row after the pool's; its
        # token is discarded and the row never holds sampler state
        pipe.prefill_row(0, 0, pre[0], P, slot=pipe.template_slot)
        prefill_tokens += P
    for t in range(T + 1):
        for i, r in admit[t] if pf else ():
            if sampling:  # the row's sampler for this request, ordered before its prefill pass (last rank)
                pipe.set_row_sampler(r // mb, r % mb, seed=request_seed(cfg.sample_seed, i), **sampling)
            if fork:
                pipe.fork_row(pipe.template_slot, r // mb, r % mb, P)
            elif P:  # the A/B baseline: a pass of the template's shape computes the prefix in the row itself
                pipe.prefill_row(r // mb, r % mb, pre[i], P)
                prefill_tokens += P
            if proc and rank == world - 1:  # the row's processor state and its history, the whole prompt (a forked or
                # prefilled prefix included), ordered before the pass whose tail yields the first generated token
                pipe.set_row_processor(r // mb, r % mb, prompt=prompts[i], **proc)
            if guide is not None:  # the start state, ordered before that pass: the guide sees generated tokens only
                pipe.set_row_guide(r // mb, r % mb, guide_id)
            if P:  # the rest of the prompt behind the prefix; its tail yields the first generated token
                tok = pipe.prefill_row(r // mb, r % mb, rest[i], lens[i] - P, past=P)
            else:
                tok = pipe.prefill_row(r // mb, r % mb, pids[i] if pids is not None else None, lens[i])
            prefill_tokens += lens[i] - P
            if rank == 0:
                first[i] = tok.clone()
        if t == T:
            break
        pasts = [pos[t][j * mb:(j + 1) * mb] for j in range(n_mb)]
        feed = None
        if pipe.is_first:
            feed = [((torch.where(tp[t, j], pipe.pf_tok[j], ft[t, j]) if pf else ft[t, j]), fm[t, j])
                    for j in range(n_mb)]
        pipe.step(1, record=rec, feed=feed, pasts=pasts)
    if T:
        pipe.finish(record=rec)
    if cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    # ---- finish (Finish, Close)
    if world > 1:
        dist.barrier()
    if rank != 0:
        return None
    y = torch.stack([torch.stack(r, 0) for r in rec], 1).view(T, rows).cpu() if T else None  # round t's tokens
    if pf:
        out = [[int(first[i].item())] + (y[t0:t0 + cfg.max_length - 1, r].tolist() if T else [])
               for i, (r, t0) in enumerate(sched)]
    else:
        out = [y[t0 + n - 1:t0 + n - 1 + cfg.max_length, r].tolist() for (r, t0), n in zip(sched, lens)]
    res = {"samples": out, "num_sample": cfg.num_sample, "max_length": cfg.max_length,
           "core_pool_size": cfg.core_pool_size, "stages": world, "prompt_lens": lens, "rounds": T,
           "prefill": pf, "seconds": dt, "tokens_per_s": cfg.num_sample * cfg.max_length / dt}
    if sampling:
        res.update(sample=True, sample_seed=cfg.sample_seed, **sampling)
    if proc:
        res.update(processors={k: v for k, v in proc.items() if k not in ("bias", "bad_tokens")},
                   token_bias=[list(e) for e in cfg.token_bias], bad_token=list(cfg.bad_token))
    if guide is not None:  # per sample: the state its tokens lead to, the picks the guide rejected, the first EOS (the
        # host's walk of the sample's tokens: a row's device state is overwritten at the next admission and goes on
        # stepping while the row idles)
        recs = []
        for o in out:
            q, rej = guide.walk(o)
            recs.append({"state": q, "n_rejected": rej, "eos_at": o.index(cfg.eos_id) if cfg.eos_id in o else None})
        res.update(guide={"n_states": int(guide.n_states), "choice": [list(c) for c in cfg.choice],
                          "guide_file": cfg.guide_file, "eos_id": cfg.eos_id}, guide_records=recs)
    if P:  # prefill_tokens: the tokens pushed through prefill passes, the template's included
        res.update(shared_prefix=P, prefix_fork=fork, prefill_tokens=prefill_tokens)
    say(STATES[2], {k: v for k, v in res.items() if k != "samples"})
    say(STATES[3], {})
    return res


def classify_batches(lens, rows):
    """The classification passes: samples grouped by prompt length (a pass is one prompt length for every
    row, Pipeline.step), in sample order within a group, `rows` samples a pass.  Returns [(length, [sample
    ids])]; a short last pass of a group is padded by the caller."""
    groups = {}
    for i, n in enumerate(lens):
        groups.setdefault(n, []).append(i)
    return [(n, ids[k:k + rows]) for n, ids in groups.items() for k in range(0, len(ids), rows)]


def _classify_run(cfg, model, rank, world, device, prompts, lens, executor_factory, say):
    """max_length == 0 (Communication.java:591-603): every sample is one pass through the stages from empty KV
    rows; the last stage's classifier tail returns its class id."""
    from .pipeline import classify
    if cfg.n_labels < 1:
        raise ValueError("classification needs n_labels >= 1")
    n_mb = min(cfg.core_pool_size, world)
    mb = -(-cfg.core_pool_size // n_mb)
    rows = n_mb * mb
    passes = classify_batches(lens, rows)
    pipe, (lb, le) = build_rank(model, rank, world, device, dtype=cfg.dtype, mb_rows=mb, n_mb=n_mb,
                                max_ctx=max(lens) + 1, max_seq=max(lens), seed=cfg.seed, head_split=False,
                                executor_factory=executor_factory, n_labels=cfg.n_labels, kv_int8=cfg.kv == "int8")
    say(STATES[0], {"rank_layers": [lb, le], "stages": world, "core_pool_size": cfg.core_pool_size,
                    "micro_batches": n_mb, "rows_per_micro_batch": mb, "passes": len(passes),
                    "task": "classification", "n_labels": cfg.n_labels})
    cuda = device.type == "cuda"
    if cuda:
        torch.cuda.set_stream(torch.cuda.Stream(device))  # as the generation task (1-token prompts replay graphs)
    if world > 1:
        dist.barrier()
    say(STATES[1], {"num_sample": cfg.num_sample, "max_length": 0})
    out = [None] * cfg.num_sample
    t_start = time.perf_counter()
    for n, ids in passes:
        prompt = None
        if rank == 0:  # a short pass repeats its first sample in the spare rows (their classes are dropped)
            prompt = torch.tensor([prompts[i] for i in ids] + [prompts[ids[0]]] * (rows - len(ids)),
                                  dtype=torch.int32, device=device)
        cls = classify(pipe, prompt, n)
        if rank == 0:
            for i, c in zip(ids, cls.tolist()):
                out[i] = int(c)
    if cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    if world > 1:
        dist.barrier()
    if rank != 0:
        return None
    res = {"samples": out, "task": "classification", "n_labels": cfg.n_labels, "num_sample": cfg.num_sample,
           "max_length": 0, "core_pool_size": cfg.core_pool_size, "stages": world, "prompt_lens": lens,
           "passes": len(passes), "seconds": dt, "samples_per_s": cfg.num_sample / dt}
    say(STATES[2], {k: v for k, v in res.items() if k != "samples"})
    say(STATES[3], {})
    return res


def _score_run(cfg, model, rank, world, device, prompts, lens, executor_factory, say):
    """--score: every sample's prompt is one teacher-forced pass from empty KV rows (pipeline.score), `core_pool_size`
    samples a pass in sample order.  Ragged prompts are padded at the tail to the pass's longest (token 0, no
    target): attention is causal, so the real positions do not see the padding.  Rank 0 returns per sample the
    summed log-likelihood of tokens 2..n given their prefixes, their count and the perplexity exp(-sum / count)."""
    import math
    from .pipeline import score
    n_mb = min(cfg.core_pool_size, world)
    mb = -(-cfg.core_pool_size // n_mb)
    rows = n_mb * mb
    passes = [list(range(k, min(k + rows, cfg.num_sample))) for k in range(0, cfg.num_sample, rows)]
    pipe, (lb, le) = build_rank(model, rank, world, device, dtype=cfg.dtype, mb_rows=mb, n_mb=n_mb,
                                max_ctx=max(lens) + 1, max_seq=max(lens), seed=cfg.seed, head_split=False,
                                executor_factory=executor_factory, kv_int8=cfg.kv == "int8")
    say(STATES[0], {"rank_layers": [lb, le], "stages": world, "core_pool_size": cfg.core_pool_size,
                    "micro_batches": n_mb, "rows_per_micro_batch": mb, "passes": len(passes), "task": "score"})
    cuda = device.type == "cuda"
    if cuda:
        torch.cuda.set_stream(torch.cuda.Stream(device))
    if world > 1:
        dist.barrier()
    say(STATES[1], {"num_sample": cfg.num_sample, "task": "score"})
    out = [None] * cfg.num_sample
    t_start = time.perf_counter()
    for ids in passes:
        n = max(lens[i] for i in ids)
        prompt = None
        if rank == 0:  # spare rows of a short pass repeat its first sample (their scores are dropped)
            prompt = torch.tensor([prompts[i] + [0] * (n - lens[i]) for i in ids + [ids[0]] * (rows - len(ids))],
                                  dtype=torch.int32, device=device)
        res = score(pipe, prompt, n)
        if rank == 0:
            lp = res[1][..., 0].double().cpu()
            for r, i in enumerate(ids):
                cnt = lens[i] - 1
                ll = float(lp[r, :cnt].sum())  # position t scores token t + 1; the padding is not counted
                out[i] = {"loglik": ll, "tokens": cnt, "perplexity": math.exp(-ll / cnt) if cnt else None}
    if cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    if world > 1:
        dist.barrier()
    if rank != 0:
        return None
    ntok = sum(lens)
    res = {"samples": out, "task": "score", "num_sample": cfg.num_sample, "core_pool_size": cfg.core_pool_size,
           "stages": world, "prompt_lens": lens, "passes": len(passes), "seconds": dt, "tokens_per_s": ntok / dt}
    say(STATES[2], {k: v for k, v in res.items() if k != "samples"})
    say(STATES[3], {})
    return res


def _spec_run(cfg, model, device, prompts, lens, say):
    """--speculate K (world == 1): the whole model as one stage, the samples decoded one after another in KV row 0
    by speculative.SpeculativeDecoder.  Returns the generation task's record plus the acceptance statistics.
    --sample --sample-speculate K: the same loop, sample i decoded with the sampler state of the config and
    request_seed(sample_seed, i); a model drafter holds the same state."""
    from .speculative import NgramDrafter, SpeculativeDecoder, StageChain, StageDrafter
    from .stage import Stage
    dev = device.index if device.type == "cuda" and device.index is not None else 0
    max_ctx = max(lens) + cfg.max_length + 1

    def whole(m):
        return Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype=cfg.dtype, device=dev, max_batch=1,
                     max_ctx=max_ctx, max_tokens=max(lens) + 32, seed=cfg.seed, int8_weights=m.int8_weights,
                     mxfp4_weights=m.mxfp4_weights)

    k = cfg.sample_speculate or cfg.speculate
    sampling = ({"top_k": cfg.top_k, "top_p": cfg.top_p, "temperature": cfg.temperature} if cfg.sample_speculate
                else None)
    if cfg.draft == "ngram":
        drafter = NgramDrafter(k)
    else:
        dm = config.get(cfg.draft) if isinstance(cfg.draft, str) else cfg.draft
        if dm.vocab != model.vocab:
            raise ValueError(f"draft model {dm.name} has another vocabulary ({dm.vocab}) than {model.name} ({model.vocab})")
        drafter = StageDrafter([whole(dm)], k)
    chain = StageChain([whole(model)])
    say(STATES[0], {"rank_layers": [0, model.n_layer], "stages": 1, "speculate": k, "draft": cfg.draft,
                    **({"sample": True} if sampling else {})})
    say(STATES[1], {"num_sample": cfg.num_sample, "max_length": cfg.max_length})
    out, tot = [], {"passes": 0, "drafted": 0, "accepted": 0, "plain_steps": 0}
    t_start = time.perf_counter()
    for i, p in enumerate(prompts):
        sampler = dict(sampling, seed=request_seed(cfg.sample_seed, i)) if sampling else None
        if sampler and isinstance(drafter, StageDrafter):
            drafter.chain.set_sampler(sampler)  # the draft row draws with this request's u
        toks, st = SpeculativeDecoder(chain, drafter, k, sampler=sampler).generate(p, cfg.max_length)
        out.append(toks)
        for name in tot:
            tot[name] += st[name]
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    res = {"samples": out, "num_sample": cfg.num_sample, "max_length": cfg.max_length,
           "core_pool_size": cfg.core_pool_size, "stages": 1, "prompt_lens": lens, "seconds": dt,
           "tokens_per_s": cfg.num_sample * cfg.max_length / dt, "speculate": cfg.speculate, "draft": cfg.draft, **tot,
           "acceptance_rate": tot["accepted"] / tot["drafted"] if tot["drafted"] else None}
    if sampling:
        res.update(sample=True, sample_seed=cfg.sample_seed, sample_speculate=k, **sampling)
    say(STATES[2], {k: v for k, v in res.items() if k != "samples"})
    say(STATES[3], {})
    return res


def _beam_run(cfg, model, device, prompts, lens, say):
    """--num-beams W (world == 1): the whole model as one stage with W KV rows, the samples decoded one after another
    by beam.BeamSearcher.  Returns the generation task's record (a sample's tokens: its best hypothesis, which an
    eos may end before max_length) plus the hypotheses' scores and the KV row pairs copied."""
    from .beam import BeamSearcher
    from .stage import Stage
    dev = device.index if device.type == "cuda" and device.index is not None else 0
    W = cfg.num_beams
    if cfg.eos_id >= model.vocab:
        raise ValueError(f"eos_id ({cfg.eos_id}) outside the vocabulary ({model.vocab})")
    stage = Stage(model.hidden, model.n_head, model.n_layer, model.vocab, 0, model.n_layer, dtype=cfg.dtype, device=dev,
                  max_batch=W, max_ctx=max(lens) + cfg.max_length + 1, max_tokens=max(max(lens), W), seed=cfg.seed,
                  int8_weights=model.int8_weights, mxfp4_weights=model.mxfp4_weights, kv_int8=cfg.kv == "int8")
    searcher = BeamSearcher([stage], W, length_penalty=cfg.length_penalty, eos=cfg.eos_id)
    say(STATES[0], {"rank_layers": [0, model.n_layer], "stages": 1, "num_beams": W})
    say(STATES[1], {"num_sample": cfg.num_sample, "max_length": cfg.max_length})
    out, scores = [], []
    t_start = time.perf_counter()
    for p in prompts:
        seqs, sc, _ = searcher.generate(p, cfg.max_length)
        out.append(seqs[0])
        scores.append(sc[0])
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    res = {"samples": out, "num_sample": cfg.num_sample, "max_length": cfg.max_length,
           "core_pool_size": cfg.core_pool_size, "stages": 1, "prompt_lens": lens, "seconds": dt,
           "tokens_per_s": sum(len(t) for t in out) / dt, "num_beams": W, "length_penalty": cfg.length_penalty,
           "scores": scores, "kv_copies": searcher.kv_copies}
    say(STATES[2], {k: v for k, v in res.items() if k != "samples"})
    say(STATES[3], {})
    stage.close()
    return res


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for f in dataclasses.fields(RunConfig):
        flag = "--" + f.name.replace("_", "-")
        if f.type is tuple or f.type == "tuple":  # repeatable: --bad-token ID, --token-bias ID:VALUE
            p.add_argument(flag, action="append", default=[], type=int if f.name == "bad_token" else str)  # and --choice
        elif f.type is bool or f.type == "bool":
            p.add_argument(flag, type=int, nargs="?", const=1, default=int(f.default))  # `--score` == `--score 1`
        else:
            p.add_argument(flag, type=type(f.default), default=f.default)
    p.add_argument("--prompts-file", default=None, help="JSON list of token-id lists (one per sample)")
    p.add_argument("--out", default=None, help="write the samples' token ids here (JSON)")
    a = p.parse_args(argv)
    cfg = RunConfig(**{f.name: (bool(getattr(a, f.name)) if f.type is bool or f.type == "bool"
                                else getattr(a, f.name)) for f in dataclasses.fields(RunConfig)})
    rank, world, local = init_distributed() if int(os.environ.get("WORLD_SIZE", "1")) > 1 else (0, 1, 0)
    device = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    prompts = json.load(open(a.prompts_file)) if (a.prompts_file and rank == 0) else None
    log = lambda state, info: print(json.dumps({"state": state, **info}), flush=True)  # noqa: E731
    res = run_rank(cfg, rank, world, device, prompts=prompts, log=log)
    if res is not None:
        if a.out:
            json.dump(res["samples"], open(a.out, "w"))
        print(json.dumps({k: v for k, v in res.items() if k != "samples"}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
