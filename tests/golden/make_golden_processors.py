"""tests/golden/make_golden_processors.py — builds tests/golden/tiny_processors.npz (run in the dev container only).

The per-row logit processors are pinned on the locally installed transformers: BloomForCausalLM.generate(do_sample=
False, max_new_tokens=24, ...) on the tiny HF BLOOM built from the repo generator's weights (make_golden.build), fp32 on
the CPU.  Cases: repetition_penalty 1.3 alone; no_repeat_ngram_size 2 alone; sequence_bias and bad_words_ids;
min_new_tokens 8 with an EOS; all of them together.  Recorded: the generated ids of every case (up to and including the
EOS where one ends the sequence) and the processed `scores` of the first 4 steps, with -inf stored as -FLT_MAX.

The synthetic model's tied embedding makes the last token's own logit about 1.3 against at most 0.5 for the rest, so
plain greedy repeats one token and a penalty of 1.3 moves it below another token for one prompt of the 60 000 searched: the
search runs over model seeds 1..300, prompt seeds 500..539 and prompt lengths 7, 12, 4, 2, 1, and first asks
transformers, one batch per (model seed, length), which prompts the penalty changes at all.

A (model seed, prompt seed, prompt length) is refused unless every case changes the plain greedy output -- for that,
plain greedy must repeat a bigram, and must emit the chosen EOS before step 8 -- and unless tests/logit_proc_ref.py's loop over the
fp32 CPU checker's logits reproduces transformers' ids.  The fixture also records, over all cases and all steps,
  min_gap   the smallest gap between the two largest processed logits of a step (checker + reference), and
  max_diff  the largest |checker logit - transformers score| over the entries that are not banned,
and a pair is refused unless min_gap >= 100 * max_diff (the margin rule of make_golden_beam.py): max_diff is the
distance of two fp32 evaluations of the same model, the fp32 device is a third, and the GPU end-to-end test relies on
the margin when it demands the same ids.

Usage:  python tests/golden/make_golden_processors.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import gen_np  # noqa: E402
from oracle.oracle import OracleStage  # noqa: E402
import logit_proc_ref as ref  # noqa: E402
from make_golden import build  # noqa: E402

torch.set_grad_enabled(False)

H, NH, L, V = 64, 4, 2, 512
N_NEW = 24
N_SCORES = 4
PROMPT_LENS = (7, 12, 4, 2, 1)
PROMPT_SEEDS = range(500, 540)
MIN_NEW = 8
PENALTY = 1.3
CASES = ("penalty", "ngram", "bias_bad", "min_new", "all")


def checker_logits_fn(o):
    def fn(tokens):
        return o.forward(np.asarray(tokens, np.int32), 1, len(tokens), slot=0, past_len=0, want_logits=True)[1][0]
    return fn


def hf_generate(m, prompt, p):
    kw = {}
    fin = {(t,): v for t, v in p["bias"] if np.isfinite(v)}
    bad = [[t] for t, v in p["bias"] if v == float("-inf")]
    if p["repetition_penalty"] != 1.0:
        kw["repetition_penalty"] = p["repetition_penalty"]
    if p["no_repeat_ngram"]:
        kw["no_repeat_ngram_size"] = p["no_repeat_ngram"]
    if fin:
        kw["sequence_bias"] = fin
    if bad:
        kw["bad_words_ids"] = bad
    if p["eos_id"] >= 0:
        kw.update(eos_token_id=p["eos_id"], pad_token_id=p["eos_id"], min_new_tokens=p["min_new_tokens"])
    out = m.generate(torch.tensor([prompt], dtype=torch.int64), do_sample=False, max_new_tokens=N_NEW,
                     return_dict_in_generate=True, output_scores=True, **kw)
    ids = out.sequences[0, len(prompt):].tolist()
    if p["eos_id"] >= 0 and p["eos_id"] in ids:
        ids = ids[:ids.index(p["eos_id"]) + 1]
    scores = np.stack([s[0].numpy() for s in out.scores[:len(ids)]]).astype(np.float32)
    scores[np.isneginf(scores)] = ref.BAN
    return ids, scores


def case_bias(plain):
    return [(plain[1], -4.0), ((plain[0] + 1) % V, 0.5)]


def case_params(plain, eos, bad):
    """The five states, chosen from the plain greedy output so that each of them bites.  bad: the first token of the
    bias-only output, so the ban bites on top of the bias; it is not the EOS, which generate() drops from
    bad_words_ids."""
    bias = case_bias(plain)
    return {
        "penalty": ref.params(repetition_penalty=PENALTY),
        "ngram": ref.params(no_repeat_ngram=2),
        "bias_bad": ref.params(bias=bias, bad_tokens=bad),
        "min_new": ref.params(min_new_tokens=MIN_NEW, eos_id=eos),
        "all": ref.params(repetition_penalty=PENALTY, no_repeat_ngram=2, min_new_tokens=MIN_NEW, eos_id=eos, bias=bias,
                          bad_tokens=bad),
    }


def penalty_bites(m, plen):
    """The prompt seeds of PROMPT_SEEDS whose greedy output the penalty alone changes (one batch each way)."""
    batch = torch.tensor(np.stack([gen_np.prompt_ids(ps, 1, plen, V).reshape(-1) for ps in PROMPT_SEEDS]).astype(np.int64))
    a = m.generate(batch, do_sample=False, max_new_tokens=N_NEW)
    b = m.generate(batch, do_sample=False, max_new_tokens=N_NEW, repetition_penalty=PENALTY)
    return [ps for i, ps in enumerate(PROMPT_SEEDS) if not torch.equal(a[i], b[i])]


def try_seeds(m, model_seed, prompt_seed, plen):
    prompt = gen_np.prompt_ids(prompt_seed, 1, plen, V).reshape(-1).tolist()
    plain, _ = hf_generate(m, prompt, ref.params())
    seq = prompt + plain
    grams = list(zip(seq, seq[1:]))
    if len(set(grams)) == len(grams):
        return None, "plain greedy repeats no bigram"
    eos = plain[2]  # emitted at step 2 < MIN_NEW by plain greedy
    with_eos, _ = hf_generate(m, prompt, ref.params(eos_id=eos))
    if len(with_eos) >= MIN_NEW:
        return None, "the EOS does not end plain greedy before step 8"
    o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=1, max_ctx=64, seed=model_seed)
    fn = checker_logits_fn(o)
    res, min_gap, max_diff = {}, np.inf, 0.0
    bad = [hf_generate(m, prompt, ref.params(bias=case_bias(plain)))[0][0]]
    if bad[0] == eos or bad[0] == plain[0]:
        return None, "the bias alone changes nothing"
    for name, p in case_params(plain, eos, bad).items():
        ids, scores = hf_generate(m, prompt, p)
        base = with_eos if p["eos_id"] >= 0 else plain
        if ids == base:
            return None, f"{name}: changes nothing"
        rids, rscores = ref.generate(fn, prompt, p, len(ids))
        if rids != ids:
            return None, f"{name}: the reference over the checker's logits differs from transformers"
        for mine, theirs in zip(rscores, scores):
            live = (mine != ref.BAN) | (theirs != ref.BAN)
            if not np.array_equal(mine == ref.BAN, theirs == ref.BAN):
                return None, f"{name}: banned sets differ"
            max_diff = max(max_diff, float(np.abs(mine[live].astype(np.float64) - theirs[live]).max()))
            top2 = np.sort(mine.astype(np.float64))[-2:]
            min_gap = min(min_gap, float(top2[1] - top2[0]))
        res[name] = (p, ids, scores[:N_SCORES])
    o.close()
    if not min_gap >= 100 * max_diff:
        return None, f"min_gap {min_gap:.3e} against max_diff {max_diff:.3e}"
    return (prompt, plain, eos, res, min_gap, max_diff), "ok"


def main():
    for model_seed in range(1, 301):
        m = build(H, NH, L, V, model_seed)
        m.generation_config.eos_token_id = None
        m.generation_config.pad_token_id = None
        m.generation_config.bos_token_id = None
        for plen, prompt_seed in [(n, ps) for n in PROMPT_LENS for ps in penalty_bites(m, n)]:
            r, why = try_seeds(m, model_seed, prompt_seed, plen)
            print(f"model seed {model_seed} prompt seed {prompt_seed} length {plen}: {why}", flush=True)
            if r is None:
                continue
            prompt, plain, eos, res, min_gap, max_diff = r
            ids = np.full((len(CASES), N_NEW), -1, np.int32)
            lens = np.zeros(len(CASES), np.int32)
            scores = np.zeros((len(CASES), N_SCORES, V), np.float32)
            bias_ids = np.full((len(CASES), 4), -1, np.int32)
            bias_values = np.zeros((len(CASES), 4), np.float32)
            scal = np.zeros((len(CASES), 4), np.float64)  # penalty, ngram, min_new, eos
            for i, name in enumerate(CASES):
                p, cid, sc = res[name]
                ids[i, :len(cid)] = cid
                lens[i] = len(cid)
                scores[i] = sc
                for j, (t, v) in enumerate(p["bias"]):
                    bias_ids[i, j], bias_values[i, j] = t, v
                scal[i] = [p["repetition_penalty"], p["no_repeat_ngram"], p["min_new_tokens"], p["eos_id"]]
            np.savez_compressed(
                os.path.join(HERE, "tiny_processors.npz"),
                config=np.array([H, NH, L, V, model_seed, N_NEW, N_SCORES]), cases=np.array(CASES),
                prompt=np.array(prompt, np.int32), plain=np.array(plain, np.int32), eos=np.int32(eos), ids=ids,
                lengths=lens, scores=scores, bias_ids=bias_ids, bias_values=bias_values, scalars=scal,
                min_gap=np.float64(min_gap), max_diff=np.float64(max_diff),
                ratio=np.float64(min_gap / max_diff if max_diff else np.inf))
            print(f"tiny_processors ok: min_gap {min_gap:.3e}, max_diff {max_diff:.3e}, lengths {lens.tolist()}")
            return
    raise SystemExit("no seed passed")


if __name__ == "__main__":
    main()
