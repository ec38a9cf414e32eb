"""The logit processor rule's numpy reference (tests/logit_proc_ref.py) against the installed transformers processors
chained in generate's order, bitwise on fp32 CPU tensors (no GPU).

Two translations separate transformers' output from the rule's, both applied to transformers' side before comparing:
  * a ban is -inf there and -FLT_MAX here;
  * SequenceBiasLogitsProcessor (and NoBadWordsLogitsProcessor, its subclass) adds a dense bias tensor, so every
    logit passes through `l + 0.0` and a -0.0 comes out as +0.0 -- also where no entry names the token.  The rule adds
    nothing to a token without an entry.  Where a chain holds one of the two, the comparison therefore maps the
    reference's zeros through `+ 0.0` as well, which changes only the sign of a zero; chains without them compare
    as they are."""
import numpy as np
import pytest
import torch
from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor,
                                                    NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                    RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)

import logit_proc_ref as ref

V = 64
EOS = 7


def hf_chain(p, prompt_len):
    procs = LogitsProcessorList()
    fin = {(t,): v for t, v in p["bias"] if np.isfinite(v)}
    bad = [[t] for t, v in p["bias"] if v == float("-inf")]
    if fin:
        procs.append(SequenceBiasLogitsProcessor(sequence_bias=fin))
    if p["repetition_penalty"] != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=p["repetition_penalty"]))
    if p["no_repeat_ngram"] > 0:
        procs.append(NoRepeatNGramLogitsProcessor(p["no_repeat_ngram"]))
    if bad:
        procs.append(NoBadWordsLogitsProcessor(bad, eos_token_id=None))
    if p["eos_id"] >= 0 and p["min_new_tokens"] > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, p["min_new_tokens"], p["eos_id"], device="cpu"))
    return procs, bool(fin or bad)


def hf_apply(logits, history, p, n_generated):
    procs, dense = hf_chain(p, len(history) - n_generated)
    out = procs(torch.tensor([history], dtype=torch.int64), torch.tensor(logits, dtype=torch.float32)[None].clone())
    out = out[0].numpy().copy()
    out[np.isneginf(out)] = ref.BAN
    return out, dense


def logits_fixture(seed):
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal(V) * 3).astype(np.float32)
    l[3], l[4], l[5], l[6] = 0.0, -0.0, 2.5, -2.5  # +0.0, -0.0, positive, negative, all of them in the histories below
    return l


CASES = {
    "penalty": (ref.params(repetition_penalty=1.3), [3, 4, 5, 6, 9, 9, 5, 12], 2),
    "penalty<1": (ref.params(repetition_penalty=0.7), [3, 4, 5, 6, 6, 6], 0),
    "ngram2": (ref.params(no_repeat_ngram=2), [5, 6, 9, 5, 6, 11, 5], 3),
    "ngram3": (ref.params(no_repeat_ngram=3), [5, 6, 9, 5, 6, 11, 5, 6], 3),
    "ngram1": (ref.params(no_repeat_ngram=1), [5, 6, 9, 5, 0, V - 1], 1),
    "ngram-short-history": (ref.params(no_repeat_ngram=5), [5, 6, 5], 1),       # len + 1 < n: nothing happens
    "ngram-exact-history": (ref.params(no_repeat_ngram=4), [5, 6, 5], 1),       # len + 1 == n: runs, no full n-gram yet
    "bias": (ref.params(bias=[(3, 1.5), (4, -2.0), (0, 0.25), (V - 1, -0.5)]), [3, 9], 0),
    "bad-words": (ref.params(bad_tokens=[5, 0, V - 1]), [3, 9], 0),
    "min-new": (ref.params(min_new_tokens=4, eos_id=EOS), [3, 9, 5], 3),
    "min-new-done": (ref.params(min_new_tokens=3, eos_id=EOS), [3, 9, 5], 3),
    # one token (EOS) that is biased, seen (twice), banned by the bigram rule and the EOS under min_new_tokens at once
    "all-on-one-token": (ref.params(repetition_penalty=1.7, no_repeat_ngram=2, min_new_tokens=6, eos_id=EOS,
                                    bias=[(EOS, 3.0), (4, 1.0)], bad_tokens=[12]), [9, EOS, 4, 4, 9, EOS, 12, 9], 2),
    "all-zero-signs": (ref.params(repetition_penalty=1.3, no_repeat_ngram=3, bias=[(5, -2.5), (6, 2.5)]),
                       [3, 4, 5, 6, 3, 4], 0),
    "empty-history": (ref.params(repetition_penalty=1.3, no_repeat_ngram=1, min_new_tokens=1, eos_id=EOS), [], 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_transformers_bitwise(name, seed):
    p, history, ngen = CASES[name]
    l = logits_fixture(seed)
    got = ref.apply(l, history, p, ngen)
    if not history:  # transformers' processors cannot take an empty input_ids row: the rule there is the EOS ban alone
        want = l.copy()
        want[EOS] = ref.BAN
        assert ref.bits_equal(got, want)
        return
    want, dense = hf_apply(l, history, p, ngen)
    mine = got + np.float32(0.0) if dense else got  # module docstring: only the sign of a zero can change
    assert ref.bits_equal(mine, want), np.flatnonzero(mine.view(np.uint32) != want.view(np.uint32))
    # untouched logits are the input's bits
    touched = set(history) | {t for t, _ in p["bias"]} | {p["eos_id"]}
    rest = [v for v in range(V) if v not in touched]
    assert ref.bits_equal(got[rest], l[rest])
    assert np.all(np.isfinite(got))


def test_negative_zero_takes_the_divide_branch():
    l = np.array([-0.0, 0.0, -1.0, 1.0], np.float32)
    out = ref.apply(l, [0, 1, 2, 3], ref.params(repetition_penalty=2.0))
    assert ref.bits_equal(out, np.array([-0.0, 0.0, -2.0, 0.5], np.float32))
    want, _ = hf_apply(l, [0, 1, 2, 3], ref.params(repetition_penalty=2.0), 0)
    assert ref.bits_equal(out, want)


def test_comparison_rejects_a_penalty_per_occurrence():
    p, history, ngen = CASES["penalty"]  # 9 and 5 appear twice
    l = logits_fixture(0)
    want, _ = hf_apply(l, history, p, ngen)
    wrong = ref.apply(l, history, p, ngen, penalty_per_occurrence=True)
    assert not ref.bits_equal(wrong, want)
    assert ref.bits_equal(ref.apply(l, history, p, ngen), want)


def test_comparison_rejects_bias_and_penalty_swapped():
    p = ref.params(repetition_penalty=1.3, bias=[(5, -4.0), (6, 4.0)])  # the bias flips the sign the penalty looks at
    history, l = [5, 6, 9], logits_fixture(0)
    want, dense = hf_apply(l, history, p, 0)
    assert dense
    wrong = ref.apply(l, history, p, 0, bias_after_penalty=True) + np.float32(0.0)
    assert not ref.bits_equal(wrong, want)
    assert ref.bits_equal(ref.apply(l, history, p, 0) + np.float32(0.0), want)


def test_banned_token_has_no_mass_at_any_temperature():
    """-FLT_MAX through the sampler's weight: (l - max) / temperature in fp32 is a large negative number or -inf, never
    a NaN, and its exp is 0 -- at temperature 0.5 (the division overflows) and at 2.0."""
    for mx in (np.float32(30.0), np.float32(-30.0), np.float32(3e38)):
        for temp in (np.float32(0.5), np.float32(2.0), np.float32(1e-3)):
            with np.errstate(over="ignore"):
                arg = np.float32(np.float32(ref.BAN - mx) / temp)
            assert not np.isnan(arg) and arg < -1e30
            assert np.exp(arg) == 0.0


def test_generate_loop_matches_transformers_processors():
    """ref.generate over a toy logits function against the same loop through transformers' processors."""
    rng = np.random.default_rng(5)
    table = (rng.standard_normal((V, V)) * 2).astype(np.float32)

    def fn(tokens):
        return table[tokens[-1]] + np.float32(0.01) * np.float32(len(tokens))

    p = ref.params(repetition_penalty=1.2, no_repeat_ngram=2, min_new_tokens=5, eos_id=EOS, bad_tokens=[11])
    prompt = [1, 2, 3, 1]
    ids, _ = ref.generate(fn, prompt, p, 12)
    T = list(prompt)
    for g in range(12):
        want, _ = hf_apply(fn(T), T, p, g)
        T.append(int(np.argmax(want)))
    assert ids == T[len(prompt):]
    assert 11 not in ids and EOS not in ids[:5]
    assert all((ids[i], ids[i + 1]) not in {(a, b) for a, b in zip(T[:len(prompt) + i], T[1:len(prompt) + i])}
               for i in range(len(ids) - 1))
