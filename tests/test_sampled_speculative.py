"""Sampled speculative decoding, host logic on the CPU: serve's validation of sample_speculate and the decoder against
a scripted chain -- draw=True is passed exactly when a sampler is set, the sampler is set before the prefill, and
rollbacks continue from the accepted position.  The GPU side is tests/test_gpu_verify_draw.py."""
import numpy as np
import pytest

from distributed_inference_demo_amd.speculative import SpeculativeDecoder, StageChain, StageDrafter

V = 101


def _next(tok, pos, seed):
    """The scripted model's token after `tok` at position `pos`; with a sampler state it depends on the seed too."""
    return (tok * 29 + pos * 5 + 11 + 7 * (seed or 0)) % V


class ScriptedSamplingStage:
    """forward_host's interface with the draw flag and set_row_sampler: a verify pass on a row with state must be
    flagged draw (as the library answers BS_ERR_STATE otherwise), and every call is logged in order."""
    is_first = is_last = True
    max_ctx = 256

    def __init__(self):
        self.past = [0]
        self.row = []
        self.state = None
        self.log = []

    def set_row_sampler(self, slot, top_k=0, top_p=1.0, temperature=1.0, seed=0, count=1, stream=None):
        assert slot == 0 and stream is None
        self.state = dict(top_k=top_k, top_p=top_p, temperature=temperature, seed=seed)
        self.log.append(("set", dict(self.state)))

    def clear_row_sampler(self, slot=None, count=1, stream=None):
        self.state = None
        self.log.append(("clear",))

    def forward_host(self, x, batch, seq, slot=0, past_len=None, want_logits=False, verify=False, draw=False):
        assert batch == 1 and slot == 0 and past_len <= len(self.row), (past_len, len(self.row))
        assert not draw or verify
        if verify:
            assert 2 <= seq <= 8
            assert draw == (self.state is not None), "a verify pass on a row with state needs the draw flag"
        ids = [int(t) for t in np.asarray(x).reshape(-1)]
        self.row[past_len:] = ids
        self.log.append(("fwd", seq, past_len, verify, draw))
        seed = self.state["seed"] if self.state else None
        outs = [_next(t, past_len + i, seed) for i, t in enumerate(ids)]
        return np.array(outs if verify else outs[-1:], np.int32)


def _plain(prompt, n, seed):
    toks, hist = [], list(prompt)
    for _ in range(n):
        toks.append(_next(hist[-1], len(hist) - 1, seed))
        hist.append(toks[-1])
    return toks


class Cycling:
    """Right for lens[i % len(lens)] tokens in round i, wrong after that."""

    def __init__(self, truth, n0, lens):
        self.truth, self.n0, self.lens, self.round = truth, n0, lens, 0

    def propose(self, history, k):
        done = len(history) - self.n0
        good = self.lens[self.round % len(self.lens)]
        self.round += 1
        return [t if j < good else (t + 1) % V for j, t in enumerate(self.truth[done:done + k])]


SAMPLER = dict(top_k=20, top_p=0.9, temperature=1.3, seed=4)


@pytest.mark.parametrize("k", [1, 4, 7])
def test_sampled_decoder_sets_the_state_first_flags_every_pass_and_rolls_back(k):
    prompt, n_new = [5, 17, 42, 8], 40
    truth = _plain(prompt, n_new, SAMPLER["seed"])
    assert truth != _plain(prompt, n_new, None)
    st = ScriptedSamplingStage()
    dec = SpeculativeDecoder([st], Cycling(truth, len(prompt), list(range(k + 1))), k, host_io=True, sampler=SAMPLER)
    toks, stats = dec.generate(prompt, n_new)
    assert toks == truth
    assert st.log[0] == ("set", SAMPLER), "the sampler is set before the prefill: the first token is sampled"
    assert st.log[1] == ("fwd", len(prompt), 0, False, False)
    fwd = [e for e in st.log[2:] if e[0] == "fwd"]
    assert len(fwd) == len(st.log) - 2, "the state is set once a generation"
    assert all(e[4] == e[3] for e in fwd), "draw is passed to every verify pass and to nothing else"
    assert stats["passes"] == sum(1 for e in fwd if e[3]) and stats["plain_steps"] == sum(1 for e in fwd if not e[3])
    assert stats["accepted"] + stats["passes"] + stats["plain_steps"] == n_new - 1
    assert 0 < stats["accepted"] < stats["drafted"]
    # every call continues where the accepted tokens end: a pass of s positions advances the row by 1 .. s, and the
    # positions of its rejected drafts are fed again (overwritten) by the next call
    starts = [e[2] for e in fwd] + [len(prompt) + n_new - 1]
    assert starts[0] == len(prompt)
    for e, nxt in zip(fwd, starts[1:]):
        assert 1 <= nxt - e[2] <= e[1], f"a call of {e[1]} positions at {e[2]} was followed by one at {nxt}"
    assert {nxt - e[2] for e, nxt in zip(fwd, starts[1:]) if e[3]} >= set(range(1, min(k, 3) + 2)), "accepted lengths"
    assert st.row[:len(prompt) + n_new - 1] == (prompt + truth)[:len(prompt) + n_new - 1]
    assert st.past[0] == len(prompt) + n_new - 1


def test_greedy_decoder_never_sets_a_state_or_passes_the_flag():
    prompt, n_new, k = [3, 1, 4], 25, 4
    truth = _plain(prompt, n_new, None)
    st = ScriptedSamplingStage()
    toks, stats = SpeculativeDecoder([st], Cycling(truth, len(prompt), [k, 0, 2]), k, host_io=True).generate(prompt, n_new)
    assert toks == truth and stats["passes"] > 0
    assert all(e[0] == "fwd" and not e[4] for e in st.log)


def test_stage_drafter_holds_the_same_state():
    """The draft model is the scripted model with the same state: every draft is the target's own draw."""
    prompt, n_new, k = [9, 2, 6, 5], 23, 3
    truth = _plain(prompt, n_new, SAMPLER["seed"])
    dst = ScriptedSamplingStage()
    dr = StageDrafter([dst], k, host_io=True, sampler=SAMPLER)
    assert dst.log == [("set", SAMPLER)], "the draft row's state is set with the drafter"
    toks, stats = SpeculativeDecoder([ScriptedSamplingStage()], dr, k, host_io=True, sampler=SAMPLER).generate(prompt, n_new)
    assert toks == truth and stats["accepted"] == stats["drafted"] > 0
    assert not any(e[0] == "fwd" and e[3] for e in dst.log), "a drafter never verifies"
    # a greedy drafter against the sampling target proposes the other model's tokens: nothing is accepted
    gd = ScriptedSamplingStage()
    toks, stats = SpeculativeDecoder([ScriptedSamplingStage()], StageDrafter([gd], k, host_io=True), k, host_io=True,
                                     sampler=SAMPLER).generate(prompt, n_new)
    assert toks == truth and stats["accepted"] == 0 and all(e[0] == "fwd" for e in gd.log)


def test_chain_verify_passes_draw_only_when_asked():
    st = ScriptedSamplingStage()
    ch = StageChain([st], host_io=True)
    ch.prefill([1, 2, 3], 0)
    ch.verify([4, 5], 3)
    ch.set_sampler(dict(seed=9))
    ch.verify([4, 5, 6], 3, draw=True)
    ch.set_sampler(None)
    assert [e for e in st.log if e[0] == "fwd"] == [("fwd", 3, 0, False, False), ("fwd", 2, 3, True, False),
                                                    ("fwd", 3, 3, True, True)]
    assert st.log[2][0] == "set" and st.log[2][1]["seed"] == 9 and st.log[-1] == ("clear",)


def test_run_config_validation_of_sample_speculate():
    import torch
    from distributed_inference_demo_amd.serve import RunConfig, run_rank
    assert RunConfig().sample_speculate == 0
    for bad in (dict(sample_speculate=2),                                  # needs sample
                dict(sample=True, sample_speculate=8), dict(sample=True, sample_speculate=-1),
                dict(sample=True, sample_speculate=2, kv="int8"),
                dict(sample=True, sample_speculate=2, score=True),
                dict(sample=True, sample_speculate=2, max_length=0),
                dict(sample=True, speculate=2),                            # the greedy flag stays excluded
                dict(sample=True, speculate=2, sample_speculate=2)):
        with pytest.raises(ValueError):
            RunConfig(**bad)
    c = RunConfig(sample=True, sample_speculate=7, top_p=0.9, draft="bloom-560m-int8")
    assert c.sample_speculate == 7 and c.speculate == 0 and c.head_split is False
    RunConfig(sample=True, sample_speculate=1)
    with pytest.raises(ValueError, match="world == 1"):
        run_rank(RunConfig(model="tiny", sample=True, sample_speculate=2), 0, 2, torch.device("cpu"))


def test_cli_flag():
    import dataclasses
    from distributed_inference_demo_amd.serve import RunConfig
    assert "sample_speculate" in {f.name for f in dataclasses.fields(RunConfig)}  # main() derives --sample-speculate
