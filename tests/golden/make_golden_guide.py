"""tests/golden/make_golden_guide.py — builds tests/golden/tiny_guide.npz (run in the dev container only).

Guided decoding is pinned on the locally installed transformers: BloomForCausalLM.generate(do_sample=False,
max_new_tokens=24, prefix_allowed_tokens_fn=...) on the tiny HF BLOOM built from the repo generator's weights
(make_golden.build), fp32 on the CPU.  The function walks the generated ids through Guide.step and returns
Guide.allowed of the state it reaches.  Cases:
  choice          one of three sequences of lengths 1, 3 and 5 that share their first token, then the EOS (from_choices;
                  the second sequence continues with the prompt's last token, the synthetic model's favourite)
  successor_bans  a default-allow machine over the eight most likely first tokens t_0..t_7: after t_i the tokens t_i and
                  t_(i+1) are banned by explicit edges, every other token is allowed (from_state_maps)
  choice_penalty  the first case with repetition_penalty 1.3, which must end in another choice than the first case
Recorded: the generated ids of every case (up to and including the EOS where one ends the sequence), the processed
`scores` of the first 4 steps with -inf stored as -FLT_MAX, and each case's guide tables.

A (model seed, prompt seed, prompt length) is refused unless every case changes the plain greedy output and unless
tests/guide_ref.py's loop over the fp32 CPU checker's logits reproduces transformers' ids.  The fixture also records,
over all cases and all steps and over ALLOWED entries only,
  min_gap   the smallest gap between the two largest allowed logits of a step with at least two allowed tokens, and
  max_diff  the largest |checker logit - transformers score|,
and a pair is refused unless min_gap >= 100 * max_diff (the margin rule of make_golden_processors.py).  The search runs
over that script's ranges: model seeds 1..300, prompt seeds 500..539, prompt lengths 7, 12, 4, 2, 1.

Usage:  python tests/golden/make_golden_guide.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from distributed_inference_demo_amd import guide as gd  # noqa: E402
from oracle import gen_np  # noqa: E402
from oracle.oracle import OracleStage  # noqa: E402
import guide_ref as gref  # noqa: E402
import logit_proc_ref as ref  # noqa: E402
from make_golden import build  # noqa: E402

torch.set_grad_enabled(False)

H, NH, L, V = 64, 4, 2, 512
N_NEW = 24
N_SCORES = 4
PROMPT_LENS = (7, 12, 4, 2, 1)
PROMPT_SEEDS = range(500, 540)
PENALTY = 1.3
CASES = ("choice", "successor_bans", "choice_penalty")


def checker_logits_fn(o):
    def fn(tokens):
        return o.forward(np.asarray(tokens, np.int32), 1, len(tokens), slot=0, past_len=0, want_logits=True)[1][0]
    return fn


def hf_generate(m, prompt, guide, eos, penalty):
    P = len(prompt)

    def allowed(batch_id, sent):
        q, rej = guide.walk(sent[P:].tolist())
        assert rej == 0
        return guide.allowed(q, V).tolist()

    kw = {"prefix_allowed_tokens_fn": allowed} if guide is not None else {}
    if penalty != 1.0:
        kw["repetition_penalty"] = penalty
    if eos >= 0:
        kw.update(eos_token_id=eos, pad_token_id=eos)
    out = m.generate(torch.tensor([prompt], dtype=torch.int64), do_sample=False, max_new_tokens=N_NEW,
                     return_dict_in_generate=True, output_scores=True, **kw)
    ids = out.sequences[0, P:].tolist()
    if eos >= 0 and eos in ids:
        ids = ids[:ids.index(eos) + 1]
    scores = np.stack([s[0].numpy() for s in out.scores[:len(ids)]]).astype(np.float32)
    scores[np.isneginf(scores)] = ref.BAN
    return ids, scores


def make_cases(prompt, first_logits, rng):
    """name -> (guide, eos, penalty)."""
    used = set(prompt)
    fresh = [int(t) for t in rng.permutation(V) if int(t) not in used][:7]
    a, c, d, e, f, g, eos = fresh
    b = prompt[-1]
    choice = gd.from_choices([[a], [a, b, c], [a, d, e, f, g]], eos, vocab=V)
    top = [int(t) for t in np.argsort(-first_logits, kind="stable")[:8]]
    maps = {0: {v: 0 for v in range(V)}}
    for i, t in enumerate(top):
        maps[0][t] = 1 + i
    for i, t in enumerate(top):
        m = dict(maps[0])
        del m[t], m[top[(i + 1) % 8]]
        maps[1 + i] = m
    bans = gd.from_state_maps(maps, 0, (), -1, V)
    assert all(x >= 0 for x in bans.default_next) and choice.default_next.max() < 0
    return {"choice": (choice, eos, 1.0), "successor_bans": (bans, -1, 1.0), "choice_penalty": (choice, eos, PENALTY)}


def try_seeds(m, model_seed, prompt_seed, plen):
    prompt = gen_np.prompt_ids(prompt_seed, 1, plen, V).reshape(-1).tolist()
    plain, _ = hf_generate(m, prompt, None, -1, 1.0)
    o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=1, max_ctx=64, seed=model_seed)
    fn = checker_logits_fn(o)
    cases = make_cases(prompt, fn(prompt), np.random.default_rng(1000 * model_seed + prompt_seed))
    res, min_gap, max_diff = {}, np.inf, 0.0
    try:
        for name, (guide, eos, penalty) in cases.items():
            ids, scores = hf_generate(m, prompt, guide, eos, penalty)
            if ids == plain[:len(ids)]:
                return None, f"{name}: changes nothing"
            p = ref.params(repetition_penalty=penalty) if penalty != 1.0 else None
            rids, rscores, q, rej = gref.generate(fn, prompt, guide, len(ids), proc=p)
            if rids != ids or rej:
                return None, f"{name}: the reference over the checker's logits differs from transformers"
            for mine, theirs in zip(rscores, scores):
                if not np.array_equal(mine == ref.BAN, theirs == ref.BAN):
                    return None, f"{name}: banned sets differ"
                live = mine != ref.BAN
                max_diff = max(max_diff, float(np.abs(mine[live].astype(np.float64) - theirs[live]).max()))
                if live.sum() >= 2:
                    top2 = np.sort(mine[live].astype(np.float64))[-2:]
                    min_gap = min(min_gap, float(top2[1] - top2[0]))
            res[name] = (guide, eos, penalty, ids, scores[:N_SCORES], q)
    finally:
        o.close()
    if res["choice"][3] == res["choice_penalty"][3]:
        return None, "the penalty does not change the choice"
    if not min_gap >= 100 * max_diff:
        return None, f"min_gap {min_gap:.3e} against max_diff {max_diff:.3e}"
    return (prompt, plain, res, min_gap, max_diff), "ok"


def main():
    for model_seed in range(1, 301):
        m = build(H, NH, L, V, model_seed)
        m.generation_config.eos_token_id = None
        m.generation_config.pad_token_id = None
        m.generation_config.bos_token_id = None
        for plen, prompt_seed in [(n, ps) for n in PROMPT_LENS for ps in PROMPT_SEEDS]:
            r, why = try_seeds(m, model_seed, prompt_seed, plen)
            print(f"model seed {model_seed} prompt seed {prompt_seed} length {plen}: {why}", flush=True)
            if r is None:
                continue
            prompt, plain, res, min_gap, max_diff = r
            ids = np.full((len(CASES), N_NEW), -1, np.int32)
            lens = np.zeros(len(CASES), np.int32)
            scores = np.zeros((len(CASES), N_SCORES, V), np.float32)
            scal = np.zeros((len(CASES), 3), np.float64)  # eos, penalty, final state
            tables = {}
            for i, name in enumerate(CASES):
                guide, eos, penalty, cid, sc, q = res[name]
                ids[i, :len(cid)] = cid
                lens[i] = len(cid)
                scores[i, :len(sc)] = sc
                scal[i] = [eos, penalty, q]
                tables[f"g{i}_meta"] = np.array([guide.n_states, guide.start], np.int32)
                for k in gd.TABLES:
                    tables[f"g{i}_{k}"] = getattr(guide, k)
            np.savez_compressed(
                os.path.join(HERE, "tiny_guide.npz"),
                config=np.array([H, NH, L, V, model_seed, N_NEW, N_SCORES]), cases=np.array(CASES),
                prompt=np.array(prompt, np.int32), plain=np.array(plain, np.int32), ids=ids, lengths=lens,
                scores=scores, scalars=scal, min_gap=np.float64(min_gap), max_diff=np.float64(max_diff),
                ratio=np.float64(min_gap / max_diff if max_diff else np.inf), **tables)
            print(f"tiny_guide ok: min_gap {min_gap:.3e}, max_diff {max_diff:.3e}, lengths {lens.tolist()}")
            return
    raise SystemExit("no seed passed")


if __name__ == "__main__":
    main()
