"""tests/golden/make_golden_beam.py — builds tests/golden/tiny_beam.npz (run in the dev container only).

Beam search is pinned on the locally installed transformers: BloomForCausalLM.generate(num_beams=W, do_sample=False,
early_stopping=False, length_penalty=..., num_return_sequences=..., max_new_tokens=12) on the tiny HF BLOOM built from
the repo generator's weights (make_golden.build), fp32 on the CPU.  Cases: W in {2, 4, 8} x {no eos, an eos that
fires} x length_penalty in {1.0, 0.6}.  "Fires": with the eos the returned hypotheses differ from those without it at
either penalty, and at one of them a returned hypothesis ends in the eos before 12 tokens (the synthetic model's
per-token log-probs are nearly flat, so at length_penalty 1.0 a long hypothesis rarely loses to a short one).

Besides transformers' sequences and sequences_scores the fixture records, over all cases,
  min_gap   the smallest score gap at any of the decisions tests/beam_ref.py names (last kept against first dropped
            candidate, ...), measured by beam_ref over the fp32 CPU checker's logits, and
  max_diff  the largest |beam_ref score - transformers score| of a returned hypothesis.
A (model seed, prompt seed) is refused unless beam_ref reproduces transformers' sequences and min_gap >= 100 *
max_diff: the synthetic model's logits span only +-1.2, so near-ties are likely, and a decision closer than the fp32
noise of two implementations is not a test of either.  max_diff is the distance of two fp32 evaluations of the same
model (transformers and the checker); the fp32 device is a third, and the GPU end-to-end test relies on the same
margin when it demands the same sequences.

Usage:  python tests/golden/make_golden_beam.py
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
import beam_ref  # noqa: E402
from make_golden import build  # noqa: E402

torch.set_grad_enabled(False)

H, NH, L, V = 64, 4, 2, 512
N_NEW = 12
BEAMS = (2, 4, 8)
PENALTIES = (1.0, 0.6)
PROMPT_LENS = {2: 6, 4: 9, 8: 5}
N_RETURN = 2


def checker_logits_fn(o):
    def fn(seqs):
        return np.stack([o.forward(np.asarray(s, np.int32), 1, len(s), slot=0, past_len=0, want_logits=True)[1][0]
                         for s in seqs])
    return fn


def hf_generate(m, prompt, W, lp, eos):
    out = m.generate(torch.tensor([prompt], dtype=torch.int64), num_beams=W, do_sample=False, early_stopping=False,
                     length_penalty=lp, num_return_sequences=N_RETURN, max_new_tokens=N_NEW, eos_token_id=eos,
                     pad_token_id=eos, return_dict_in_generate=True, output_scores=True)
    seqs = []
    for row in out.sequences[:, len(prompt):].tolist():
        n = row.index(eos) + 1 if (eos is not None and eos in row) else N_NEW
        seqs.append(row[:n])
    return seqs, out.sequences_scores.double().tolist()


def try_seeds(model_seed, prompt_seed):
    m = build(H, NH, L, V, model_seed)
    m.generation_config.eos_token_id = None
    m.generation_config.pad_token_id = None
    m.generation_config.bos_token_id = None
    o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=1, max_ctx=64, seed=model_seed)
    fn = checker_logits_fn(o)
    cases, min_gap, max_diff = [], np.inf, 0.0
    for W in BEAMS:
        prompt = gen_np.prompt_ids(prompt_seed + W, 1, PROMPT_LENS[W], V).reshape(-1).tolist()
        plain, _ = hf_generate(m, prompt, W, 1.0, None)
        eos_id = plain[1][-1]  # the token with which the second hypothesis departs from the first
        without, early = {}, False
        for eos in (None, eos_id):
            for lp in PENALTIES:
                seqs, scores = hf_generate(m, prompt, W, lp, eos)
                if eos is None:
                    without[lp] = seqs
                else:  # the eos fires: it changes what comes back at every penalty, and ends a returned hypothesis
                    if seqs == without[lp]:
                        return None, f"W={W} lp={lp}: the eos changes nothing"
                    early = early or any(len(s) < N_NEW and s[-1] == eos for s in seqs)
                st = {}
                rs, rsc = beam_ref.search(fn, prompt, N_NEW, W, length_penalty=lp, eos=eos, num_return=N_RETURN,
                                          stats=st)
                if rs != seqs:
                    return None, f"W={W} eos={eos} lp={lp}: beam_ref differs from transformers"
                min_gap = min(min_gap, st["min_gap"])
                max_diff = max(max_diff, float(np.abs(np.array(rsc) - np.array(scores)).max()))
                cases.append((W, -1 if eos is None else eos, lp, prompt, seqs, scores))
        if not early:
            return None, f"W={W}: the eos ends no returned hypothesis before {N_NEW} tokens"
    o.close()
    if not min_gap >= 100 * max_diff:
        return None, f"min_gap {min_gap:.3e} against max_diff {max_diff:.3e}"
    return (cases, min_gap, max_diff), "ok"


def main():
    for model_seed in range(1, 40):
        for prompt_seed in (500, 600, 700):
            res, why = try_seeds(model_seed, prompt_seed)
            print(f"model seed {model_seed} prompt seed {prompt_seed}: {why}", flush=True)
            if res is None:
                continue
            cases, min_gap, max_diff = res
            n = len(cases)
            seqs = np.full((n, N_RETURN, N_NEW), -1, np.int32)
            lens = np.zeros((n, N_RETURN), np.int32)
            prompts = np.full((n, max(PROMPT_LENS.values())), -1, np.int32)
            for i, (W, eos, lp, prompt, ss, sc) in enumerate(cases):
                prompts[i, :len(prompt)] = prompt
                for r, s in enumerate(ss):
                    seqs[i, r, :len(s)] = s
                    lens[i, r] = len(s)
            np.savez_compressed(
                os.path.join(HERE, "tiny_beam.npz"),
                config=np.array([H, NH, L, V, model_seed, N_NEW, N_RETURN]),
                num_beams=np.array([c[0] for c in cases], np.int32), eos=np.array([c[1] for c in cases], np.int32),
                length_penalty=np.array([c[2] for c in cases], np.float64), prompts=prompts,
                prompt_lens=np.array([len(c[3]) for c in cases], np.int32), sequences=seqs, lengths=lens,
                scores=np.array([c[5] for c in cases], np.float64), min_gap=np.float64(min_gap),
                max_diff=np.float64(max_diff), ratio=np.float64(min_gap / max_diff if max_diff else np.inf))
            print(f"tiny_beam ok: min_gap {min_gap:.3e}, max_diff {max_diff:.3e}")
            return
    raise SystemExit("no seed passed")


if __name__ == "__main__":
    main()
