"""Speculative decoding (distributed_inference_demo_amd/speculative.py, serve --speculate).

Host logic on the CPU (not marked gpu): the acceptance rule over every accepted length with scripted stages, the
n-gram drafter on hand-made histories, the stage drafter's rollback and catch-up, and serve's validation.

End to end on the GPU (marked gpu): config (64, 4, 2, 512), seed 1, a 12-token prompt, 32 new tokens.  Every drafter
-- always right, always wrong, right for j tokens with j cycling 0..K, an int8-weight draft model, the n-gram
drafter -- must reproduce the plain greedy decode of a twin stage EXACTLY.  The exact comparison is justified on the
CPU checker: a synthetic model echoes its last input token (the tied head's self-dot dominates), and over model seeds
1-8, 2 rows and 32 steps the smallest top-2 logit margin of this config is 0.56, against the 2e-2 the batched and
the single-row kernels may differ by (tests/test_gpu_parity.py BF16_TOL).
"""
import numpy as np
import pytest

from distributed_inference_demo_amd.speculative import (NgramDrafter, SpeculativeDecoder, StageChain, StageDrafter,
                                                        accept)

V = 97


def _next(tok, pos):
    """The scripted model: the greedy token after `tok` at position `pos` (depends on both, so a wrong position or a
    stale token shows)."""
    return (tok * 31 + pos * 7 + 3) % V


class ScriptedStage:
    """A first + last stage with forward_host's interface and a KV row that remembers which token sits where: the
    output after position p is _next(token at p, p), and a call must continue exactly at the row's position or
    overwrite from an earlier one (rollback)."""
    is_first = is_last = True
    max_ctx = 256

    def __init__(self):
        self.past = [0]
        self.row = []
        self.calls = []  # (seq, past, verify)

    def forward_host(self, x, batch, seq, slot=0, past_len=None, want_logits=False, verify=False):
        assert batch == 1 and slot == 0 and past_len <= len(self.row), (past_len, len(self.row))
        if verify:
            assert 2 <= seq <= 8
        ids = [int(t) for t in np.asarray(x).reshape(-1)]
        self.row[past_len:] = ids  # positions at or beyond past_len are overwritten, whatever they held
        self.calls.append((seq, past_len, verify))
        outs = [_next(t, past_len + i) for i, t in enumerate(ids)]
        return np.array(outs if verify else outs[-1:], np.int32)


def _plain(prompt, n):
    toks, hist = [], list(prompt)
    for _ in range(n):
        toks.append(_next(hist[-1], len(hist) - 1))
        hist.append(toks[-1])
    return toks


class ScriptedDrafter:
    """Right for lens[i % len(lens)] tokens in round i, wrong after that."""

    def __init__(self, truth, prompt_len, lens):
        self.truth, self.n0, self.lens, self.round = truth, prompt_len, lens, 0

    def propose(self, history, k):
        done = len(history) - self.n0
        good = self.lens[self.round % len(self.lens)]
        self.round += 1
        d = [self.truth[done + j] if done + j < len(self.truth) else 0 for j in range(k)]
        return [t if j < good else (t + 1) % V for j, t in enumerate(d)]


# ---- accept
@pytest.mark.parametrize("k", [1, 4, 7])
def test_accept_every_length(k):
    top = [10 + j for j in range(k + 1)]
    for n in range(k + 1):
        draft = [top[j] if j < n else 999 for j in range(k)]
        assert accept(draft, top) == (n, top[:n + 1])
    # a later agreement after a mismatch does not count
    if k >= 3:
        assert accept([top[0], 999] + top[2:k], top) == (1, top[:2])
    with pytest.raises(ValueError):
        accept([1, 2], [1, 2])


@pytest.mark.parametrize("k", [1, 3, 4, 7])
def test_decoder_with_scripted_stages_every_accepted_length(k):
    """j correct drafts a round, j cycling 0..k: every pass emits j + 1 tokens, the output is the plain decode, and the
    target's row never holds a rejected token at a position it went on from."""
    prompt, n_new = [5, 17, 42, 8], 40
    truth = _plain(prompt, n_new)
    st = ScriptedStage()
    dr = ScriptedDrafter(truth, len(prompt), list(range(k + 1)))
    toks, stats = SpeculativeDecoder([st], dr, k, host_io=True).generate(prompt, n_new)
    assert toks == truth
    assert st.row[:len(prompt) + n_new - 1] == (prompt + truth)[:len(prompt) + n_new - 1]
    assert st.calls[0] == (len(prompt), 0, False)
    assert stats["passes"] + stats["plain_steps"] == len(st.calls) - 1
    assert stats["passes"] == sum(1 for c in st.calls if c[2])
    assert stats["accepted"] + stats["passes"] + stats["plain_steps"] == n_new - 1
    assert 0 < stats["accepted"] < stats["drafted"]
    assert all(2 <= c[0] <= k + 1 for c in st.calls if c[2])
    assert st.past[0] == len(prompt) + n_new - 1


def test_decoder_always_right_always_wrong_and_silent_drafters():
    prompt, n_new, k = [3, 1, 4], 31, 4
    truth = _plain(prompt, n_new)
    right = ScriptedDrafter(truth, len(prompt), [k])
    toks, stats = SpeculativeDecoder([ScriptedStage()], right, k, host_io=True).generate(prompt, n_new)
    assert toks == truth and stats["accepted"] == stats["drafted"] and stats["plain_steps"] == 0
    assert stats["passes"] == (n_new - 1) // (k + 1)  # 30 tokens after the prefill's, 5 a pass
    wrong = ScriptedDrafter(truth, len(prompt), [0])
    toks, stats = SpeculativeDecoder([ScriptedStage()], wrong, k, host_io=True).generate(prompt, n_new)
    assert toks == truth and stats["accepted"] == 0 and stats["passes"] == n_new - 2 and stats["plain_steps"] == 1

    class Silent:
        def propose(self, history, k):
            return []

    st = ScriptedStage()
    toks, stats = SpeculativeDecoder([st], Silent(), k, host_io=True).generate(prompt, n_new)
    assert toks == truth and stats == {"passes": 0, "drafted": 0, "accepted": 0, "plain_steps": n_new - 1}
    assert all(c[0] == 1 and not c[2] for c in st.calls[1:])
    with pytest.raises(ValueError):
        SpeculativeDecoder([ScriptedStage()], Silent(), 8, host_io=True)


def test_stage_drafter_rolls_back_and_catches_up():
    """The draft model is the scripted model itself: every draft is right, and its row is rolled back to the shared
    prefix and caught up (one S = 1 step or a short prefill) before each round."""
    prompt, n_new, k = [9, 2, 6, 5], 23, 3
    truth = _plain(prompt, n_new)
    dst = ScriptedStage()
    dr = StageDrafter([dst], k, host_io=True)
    toks, stats = SpeculativeDecoder([ScriptedStage()], dr, k, host_io=True).generate(prompt, n_new)
    assert toks == truth and stats["accepted"] == stats["drafted"]
    assert dst.calls[0] == (len(prompt) + 1, 0, False)              # the prompt and the prefill's token
    assert (2, len(prompt) + k, False) in dst.calls                 # catch-up on the last draft + the bonus token
    assert not any(c[2] for c in dst.calls)                         # a drafter never verifies
    # a history that diverges from what the draft's row holds: rolled back to the shared prefix
    d = dr.propose([9, 2, 7], 2)
    assert dst.calls[-2][:2] == (1, 2) and d[0] == _next(7, 2) and d[1] == _next(d[0], 3)


# ---- NgramDrafter
def test_ngram_longest_suffix_most_recent_occurrence():
    d = NgramDrafter(3, n_max=3)
    #    0  1  2  3  4  5  6  7  8  9 10 11
    h = [1, 2, 3, 7, 9, 2, 3, 8, 4, 1, 2, 3]
    # suffix [1, 2, 3] occurred at 0: the longest match wins over the more recent [2, 3] at 5
    assert d.propose(h) == [7, 9, 2]
    # only [2, 3] repeats (n = 2): occurrences at 1 and 5, the most recent one is followed by 8, 4, 6
    assert d.propose([1, 2, 3, 7, 9, 2, 3, 8, 4, 6, 2, 3]) == [8, 4, 6]
    # single-token match, most recent occurrence
    assert NgramDrafter(2, n_max=3).propose([5, 1, 5, 2, 9, 5]) == [2, 9]


def test_ngram_no_match_and_short_proposals():
    d = NgramDrafter(4, n_max=3)
    assert d.propose([1, 2, 3, 4, 5]) == []
    assert d.propose([7]) == [] and d.propose([]) == []
    # the match sits near the end: fewer than k tokens follow it
    assert d.propose([4, 6, 9, 4, 6]) == [9, 4, 6]
    assert d.propose([3, 3]) == [3]
    # the decoder may ask for fewer than the drafter's k
    assert d.propose([1, 2, 3, 7, 9, 1, 2, 3], k=2) == [7, 9]
    assert d.propose([1, 2, 3, 7, 9, 1, 2, 3], k=0) == []
    with pytest.raises(ValueError):
        NgramDrafter(0)


# ---- serve validation
def test_run_config_validation():
    import torch
    from distributed_inference_demo_amd.serve import RunConfig, run_rank
    assert RunConfig().speculate == 0 and RunConfig().draft == "ngram"
    for bad in (dict(speculate=8), dict(speculate=-1), dict(speculate=2, kv="int8"),
                dict(speculate=2, max_length=0), dict(speculate=2, score=True)):
        with pytest.raises(ValueError):
            RunConfig(**bad)
    RunConfig(speculate=1), RunConfig(speculate=7, draft="bloom-560m-int8")
    with pytest.raises(ValueError, match="world == 1"):
        run_rank(RunConfig(model="tiny", speculate=2), 0, 2, torch.device("cpu"))


# ---- end to end on the GPU
EH, ENH, EL, EV, ESEED, EP, EN = 64, 4, 2, 512, 1, 12, 32


def _gpu_stage(**kw):
    from distributed_inference_demo_amd.stage import Stage
    return Stage(EH, ENH, EL, EV, 0, EL, dtype="bf16", max_batch=1, max_ctx=EP + EN + 8, max_tokens=32, seed=ESEED,
                 **kw)


_PLAIN = {}


def _gpu_plain():
    """The plain greedy decode of a twin stage (prefill + S = 1 steps), computed once."""
    if not _PLAIN:
        from oracle import gen_np
        prompt = gen_np.prompt_ids(5, 1, EP, EV).reshape(-1).tolist()
        ch = StageChain([_gpu_stage()])
        toks = [ch.prefill(prompt, 0)]
        for i in range(EN - 1):
            toks.append(ch.step(toks[-1], EP + i))
        _PLAIN["v"] = (prompt, toks)
    return _PLAIN["v"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 7])
def test_gpu_replay_wrong_and_scripted_drafters_equal_plain_decode(k):
    prompt, truth = _gpu_plain()
    toks, stats = SpeculativeDecoder([_gpu_stage()], ScriptedDrafter(truth, EP, [k]), k).generate(prompt, EN)
    print(f"replay drafter k={k}: {stats}")
    assert toks == truth
    assert stats["accepted"] == stats["drafted"]  # every pass emits all it drafted + 1: k + 1 until the tail
    # EN - 1 tokens after the prefill's, k + 1 a round; a single token left over is a plain step
    assert stats["passes"] + stats["plain_steps"] == -(-(EN - 1) // (k + 1)) and stats["plain_steps"] <= 1
    assert stats["drafted"] + stats["passes"] + stats["plain_steps"] == EN - 1
    toks, stats = SpeculativeDecoder([_gpu_stage()], ScriptedDrafter(truth, EP, [0]), k).generate(prompt, EN)
    print(f"wrong drafter k={k}: {stats}")
    assert toks == truth and stats["accepted"] == 0 and stats["passes"] == EN - 2  # one token a pass
    toks, stats = SpeculativeDecoder([_gpu_stage()], ScriptedDrafter(truth, EP, list(range(k + 1))), k).generate(
        prompt, EN)
    print(f"scripted drafter k={k}: {stats}")
    assert toks == truth and 0 < stats["accepted"] < stats["drafted"]


@pytest.mark.gpu
def test_gpu_int8_stage_drafter_and_ngram_drafter_equal_plain_decode():
    prompt, truth = _gpu_plain()
    k = 4
    dr = StageDrafter([_gpu_stage(int8_weights=True)], k)
    toks, stats = SpeculativeDecoder([_gpu_stage()], dr, k).generate(prompt, EN)
    print(f"int8 self-draft: {stats}")
    assert toks == truth and stats["passes"] > 0
    toks, stats = SpeculativeDecoder([_gpu_stage()], NgramDrafter(k), k).generate(prompt, EN)
    print(f"n-gram drafter: {stats}")
    assert toks == truth and stats["passes"] + stats["plain_steps"] + stats["accepted"] == EN - 1


@pytest.mark.gpu
def test_gpu_serve_speculate_returns_the_plain_samples():
    import torch
    from distributed_inference_demo_amd.config import BloomDims
    from distributed_inference_demo_amd.serve import RunConfig, run_rank
    m = BloomDims("tiny-spec", EH, EL, ENH, EV)
    kw = dict(model=m, num_sample=3, max_length=EN, prompt_len=EP, dtype="bf16", seed=ESEED)
    dev = torch.device("cuda", 0)
    plain = run_rank(RunConfig(**kw), 0, 1, dev)
    spec = run_rank(RunConfig(speculate=4, **kw), 0, 1, dev)
    assert spec["samples"] == plain["samples"]
    assert spec["speculate"] == 4 and spec["passes"] + spec["plain_steps"] + spec["accepted"] == 3 * (EN - 1)
    print({k: v for k, v in spec.items() if k != "samples"})
