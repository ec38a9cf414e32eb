"""Beam search, host side (distributed_inference_demo_amd/beam.py, serve --num-beams), on the CPU.

  assign_slots     every property its docstring states, exhaustively for W <= 4 and on 2000 seeded vectors for W = 8,
                   and that replaying the copies on a list of row labels gives each child its parent's label.
  beam_ref.search  the numpy restatement of transformers' _beam_search, over the fp32 CPU checker's logits, against
                   tests/golden/tiny_beam.npz (tests/golden/make_golden_beam.py): transformers' sequences exactly, its
                   scores within ten times the recorded checker-to-transformers difference; the recorded decision
                   margin is at least 100 times that difference.
  BeamSearcher     host_io=True over a stand-in stage built on the checker (its top-k from the checker's logits, its
                   fork_kv / copy_kv through read_kv / write_kv): beam_ref's sequences exactly on the same cases, so
                   the KV reordering is exercised; a stand-in whose copy_kv does nothing must not pass.
  RunConfig        validation of num_beams, length_penalty, eos_id.
"""
import itertools
import os

import numpy as np
import pytest

import beam_ref
from distributed_inference_demo_amd.beam import BeamSearcher, assign_slots
from oracle.oracle import OracleStage

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_beam.npz"))
H, NH, L, V, SEED, N_NEW, N_RETURN = (int(v) for v in G["config"])
CASES = list(range(len(G["num_beams"])))


def case(i):
    W, eos, lp = int(G["num_beams"][i]), int(G["eos"][i]), float(G["length_penalty"][i])
    prompt = G["prompts"][i, :int(G["prompt_lens"][i])].tolist()
    seqs = [G["sequences"][i, r, :int(G["lengths"][i, r])].tolist() for r in range(N_RETURN)]
    return W, (None if eos < 0 else eos), lp, prompt, seqs, G["scores"][i].tolist()


def case_id(i):
    W, eos, lp = int(G["num_beams"][i]), int(G["eos"][i]), float(G["length_penalty"][i])
    return f"W{W}-{'eos' if eos >= 0 else 'noeos'}-lp{lp}"


# ---- assign_slots
def check_assignment(parents):
    W = len(parents)
    slots, copies = assign_slots(parents)
    assert sorted(slots) == list(range(W)), "every row holds exactly one child"
    living = set(parents)
    dead = set(range(W)) - living
    first = {}
    for i, p in enumerate(parents):
        first.setdefault(p, i)
    for i, p in enumerate(parents):
        if first[p] == i:
            assert slots[i] == p, "the best-ranked child keeps its parent's row"
        else:
            assert slots[i] in dead and (p, slots[i]) in copies
    assert len(copies) == len(dead)
    dsts = [d for _, d in copies]
    assert set(dsts) == dead and len(set(dsts)) == len(dsts), "every destination is a dead row, once"
    assert all(s in living for s, _ in copies), "every source is a living row"
    assert not set(dsts) & {s for s, _ in copies}, "no destination is a source"
    labels = [f"row{r}" for r in range(W)]  # replay in list order: the result does not depend on it (no aliasing)
    before = list(labels)
    for s, d in copies:
        labels[d] = labels[s]
    for i, p in enumerate(parents):
        assert labels[slots[i]] == before[p]


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_assign_slots_exhaustive(W):
    for parents in itertools.product(range(W), repeat=W):
        check_assignment(list(parents))


def test_assign_slots_random_w8():
    rng = np.random.default_rng(8)
    for _ in range(2000):
        check_assignment(rng.integers(0, 8, size=8).tolist())
    check_assignment([3] * 8)
    check_assignment(list(range(8))[::-1])
    with pytest.raises(ValueError):
        assign_slots([0, 2])


# ---- beam_ref against transformers
@pytest.fixture(scope="module")
def checker():
    o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=8, max_ctx=32, seed=SEED)
    yield o
    o.close()


def checker_logits_fn(o):
    def fn(seqs):
        return np.stack([o.forward(np.asarray(s, np.int32), 1, len(s), slot=0, past_len=0, want_logits=True)[1][0]
                         for s in seqs])
    return fn


_REF = {}


def ref_result(o, i):
    """beam_ref over the checker for case i, computed once and shared."""
    if i not in _REF:
        W, eos, lp, prompt, _, _ = case(i)
        _REF[i] = beam_ref.search(checker_logits_fn(o), prompt, N_NEW, W, length_penalty=lp, eos=eos,
                                  num_return=N_RETURN)
    return _REF[i]


def test_fixture_margin():
    assert float(G["min_gap"]) >= 100 * float(G["max_diff"]) > 0
    assert float(G["ratio"]) >= 100
    assert sorted(set(G["num_beams"].tolist())) == [2, 4, 8]
    assert sorted(set(G["length_penalty"].tolist())) == [0.6, 1.0]
    for W in (2, 4, 8):  # an eos that fires: it ends a returned hypothesis early in one of the W's cases
        assert any(int(G["num_beams"][i]) == W and int(G["eos"][i]) >= 0 and
                   any(0 < n < N_NEW for n in G["lengths"][i]) for i in CASES)


@pytest.mark.parametrize("i", CASES, ids=case_id)
def test_beam_ref_is_transformers(checker, i):
    _, _, _, _, seqs, scores = case(i)
    rs, rsc = ref_result(checker, i)
    assert rs == seqs
    assert np.abs(np.array(rsc) - np.array(scores)).max() <= 10 * float(G["max_diff"])


# ---- BeamSearcher over a CPU stand-in stage
class CheckerStage:
    """A first + last stage with the numpy interface BeamSearcher(host_io=True) uses, on the fp32 checker: the top-k
    pass ranks the checker's logits (stable descending order, fp32 l - lse), fork_kv / copy_kv move cached positions
    through read_kv / write_kv."""
    is_first = is_last = True

    def __init__(self, max_batch, max_ctx, copies=True):
        self.o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=max_batch, max_ctx=max_ctx, seed=SEED)
        self.max_batch, self.max_ctx, self.vocab, self.hidden = max_batch, max_ctx, V, H
        self.copies = copies
        self.copied = []

    def forward_topk_host(self, x, batch, seq, k, slot=0, past_len=None, want_logits=False):
        _, lg = self.o.forward(x, batch, seq, slot=slot, past_len=past_len, want_logits=True)
        ids = np.argsort(-lg, axis=-1, kind="stable")[:, :k].astype(np.int32)
        l64 = lg.astype(np.float64)
        m = l64.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(l64 - m).sum(-1, keepdims=True))).astype(np.float32)
        return ids, np.take_along_axis(lg, ids, -1) - lse, lse.reshape(-1)

    def _move(self, src, dst, npos):
        hd = H // NH
        for layer in range(L):
            kv = np.stack([np.stack([np.stack([self.o.read_kv(layer, w, src, h, p, hd) for p in range(npos)])
                                     for h in range(NH)]) for w in range(2)])
            self.o.write_kv(layer, dst, 0, kv)

    def fork_kv(self, src, dst, npos=None, count=1, stream=None):
        for d in range(dst, dst + count):
            self._move(src, d, npos)
        self.copied += [(src, d) for d in range(dst, dst + count)]

    def copy_kv(self, pairs, npos, stream=None):
        self.copied += list(pairs)
        if not self.copies:
            return
        assert not {s for s, _ in pairs} & {d for _, d in pairs}
        for s, d in pairs:
            self._move(s, d, npos)

    def close(self):
        self.o.close()


# The searcher (KV rows reused) against beam_ref (every sequence fed again), both on the fp32 checker: two fp32
# evaluations of one model, the distance the fixture recorded between transformers and the checker, times ten.
SCORE_TOL = 10 * float(G["max_diff"])


@pytest.mark.parametrize("i", CASES, ids=case_id)
def test_searcher_over_checker_stage_equals_beam_ref(checker, i):
    W, eos, lp, prompt, _, _ = case(i)
    st = CheckerStage(W, len(prompt) + N_NEW)
    bs = BeamSearcher([st], W, length_penalty=lp, eos=eos, num_return=N_RETURN, host_io=True)
    seqs, scores, tlps = bs.generate(prompt, N_NEW)
    rs, rsc = ref_result(checker, i)
    assert seqs == rs
    assert np.abs(np.array(scores) - np.array(rsc)).max() <= SCORE_TOL
    for s, sc, t in zip(seqs, scores, tlps):
        assert len(t) == len(s) and abs(sum(t) / len(s) ** lp - sc) <= 1e-9
    assert bs.kv_copies == len(st.copied) > 0
    st.close()


def test_a_searcher_whose_copies_do_nothing_is_caught(checker):
    """The test above sees the cache: with copy_kv a no-op (a row keeps a stale hypothesis) it fails.  The synthetic
    model mostly echoes its last token, so a stale row moves the scores, not the sequences: 1.3e-4 here against the
    tolerance of 1.7e-5 (the scripted model below makes the sequences depend on every cached token)."""
    i = next(i for i in CASES if int(G["num_beams"][i]) == 4 and int(G["eos"][i]) < 0 and G["length_penalty"][i] == 0.6)
    W, eos, lp, prompt, _, _ = case(i)
    st = CheckerStage(W, len(prompt) + N_NEW, copies=False)
    _, scores, _ = BeamSearcher([st], W, length_penalty=lp, eos=eos, num_return=N_RETURN, host_io=True).generate(
        prompt, N_NEW)
    assert len(st.copied) > W - 1, "the case reorders rows after the first fork"
    assert np.abs(np.array(scores) - np.array(ref_result(checker, i)[1])).max() > SCORE_TOL
    st.close()


# ---- a scripted model whose logits depend on every token its KV row holds
SV = 64


def scripted_logits(seq):
    rng = np.random.default_rng([int(t) for t in seq])
    return rng.normal(size=SV).astype(np.float32) * 2.0


class ScriptedStage:
    """KV rows that remember which token sits where; the logits after a row are scripted_logits(the row's tokens)."""
    is_first = is_last = True
    max_ctx, vocab, hidden = 64, SV, 8

    def __init__(self, max_batch, copies=True):
        self.max_batch, self.copies = max_batch, copies
        self.rows = [[] for _ in range(max_batch)]
        self.ncopies = 0

    def forward_topk_host(self, x, batch, seq, k, slot=0, past_len=None, want_logits=False):
        x = np.asarray(x).reshape(batch, seq)
        lg = []
        for b in range(batch):
            assert past_len <= len(self.rows[slot + b])
            self.rows[slot + b][past_len:] = [int(t) for t in x[b]]
            lg.append(scripted_logits(self.rows[slot + b]))
        lg = np.stack(lg)
        ids = np.argsort(-lg, axis=-1, kind="stable")[:, :k].astype(np.int32)
        lp = beam_ref.log_softmax64(lg).astype(np.float32)
        return ids, np.take_along_axis(lp, ids, -1), None

    def fork_kv(self, src, dst, npos=None, count=1, stream=None):
        for d in range(dst, dst + count):
            self.rows[d][:npos] = self.rows[src][:npos]

    def copy_kv(self, pairs, npos, stream=None):
        self.ncopies += len(pairs)
        if self.copies:
            for s, d in pairs:
                self.rows[d][:npos] = self.rows[s][:npos]


@pytest.mark.parametrize("W,eos,lp", [(2, None, 1.0), (3, 5, 1.0), (4, 9, 0.6), (8, None, 0.6), (8, 17, 1.3)])
def test_searcher_over_scripted_rows(W, eos, lp):
    prompt, n_new = [3, 1, 4, 1, 5], 10
    rs, rsc = beam_ref.search(lambda seqs: np.stack([scripted_logits(s) for s in seqs]), prompt, n_new, W,
                              length_penalty=lp, eos=eos, num_return=W)
    seqs, scores, _ = BeamSearcher([ScriptedStage(W)], W, length_penalty=lp, eos=eos, num_return=W,
                                   host_io=True).generate(prompt, n_new)
    assert seqs == rs and np.abs(np.array(scores) - np.array(rsc)).max() <= 1e-5  # fp32 log-probs, <= 10 a score
    st = ScriptedStage(W, copies=False)
    stale, _, _ = BeamSearcher([st], W, length_penalty=lp, eos=eos, num_return=W, host_io=True).generate(prompt, n_new)
    if W >= 4:  # with two rows the stale one may lose every later selection; from four on these cases show it
        assert st.ncopies > 0, "the case reorders rows after the first fork"
        assert stale != rs, "rows that are not copied must show"


def test_w1_is_greedy(checker):
    prompt = case(0)[3]
    st = CheckerStage(1, len(prompt) + N_NEW)
    seqs, scores, tlps = BeamSearcher([st], 1, host_io=True).generate(prompt, N_NEW)
    hist = list(prompt)
    for _ in range(N_NEW):
        hist.append(int(checker_logits_fn(checker)([hist])[0].argmax()))
    assert seqs == [hist[len(prompt):]] and st.copied == []
    st.close()


def test_searcher_arguments():
    st = CheckerStage(2, 16)
    for kw in ({"num_beams": 0}, {"num_beams": 9}, {"num_beams": 3}, {"num_beams": 2, "num_return": 3}):
        with pytest.raises(ValueError):
            BeamSearcher([st], host_io=True, **kw)
    bs = BeamSearcher([st], 2, host_io=True)
    with pytest.raises(ValueError):
        bs.generate([], 4)
    with pytest.raises(ValueError):
        bs.generate([1, 2, 3], 14)
    st.close()


# ---- serve's validation
def test_run_config_validation():
    from distributed_inference_demo_amd.serve import RunConfig
    cfg = RunConfig(num_beams=4, length_penalty=0.6, eos_id=7)
    assert (cfg.num_beams, cfg.length_penalty, cfg.eos_id) == (4, 0.6, 7)
    assert RunConfig().num_beams == 0 and RunConfig().eos_id == -1 and RunConfig().length_penalty == 1.0
    for kw in ({"num_beams": 9}, {"num_beams": -1}, {"num_beams": 2, "sample": True}, {"num_beams": 2, "speculate": 3},
               {"num_beams": 2, "sample": True, "sample_speculate": 3}, {"num_beams": 2, "score": True},
               {"num_beams": 2, "shared_prefix": 4}, {"num_beams": 2, "max_length": 0}, {"num_beams": 2, "eos_id": -2},
               {"num_beams": 2, "length_penalty": float("inf")}):
        with pytest.raises(ValueError):
            RunConfig(**kw)
    RunConfig(num_beams=8, kv="int8")
