"""Per-row sampling on the GPU, kernel level: bs_sample_logits (the kernels the tail runs) on constructed logits of a
tiny stage, every draw through the tolerant checker of tests/row_sampling_ref.py.

Vocabulary sizes: 512 (under one block), 2064 (two blocks a row, not a multiple of 1024), 250 880 (the real head, 64
blocks a row)."""
import numpy as np
import pytest

import row_sampling_ref as ref
from distributed_inference_demo_amd.stage import BloomStageError, Stage

pytestmark = pytest.mark.gpu

VOCABS = [512, 2064, 250880]
POSITIONS = [0, 1, 2 ** 20]
FIXTURES = [("normal", 0), ("normal", 1), ("normal", 2), ("tied", 0), ("spike", 0), ("equal", 0)]


def states(V):
    return [(0, 0.9, 1.0), (0, 1.0, 0.7), (50, 0.95, 1.3), (5, 0.5, 1.0), (0, 1e-6, 1.0), (V + 5, 1.0, 2.0),
            (1, 1.0, 1.0), (0, 0.9, 0.01)]


_stages = {}
_logits = {}


def stage(V):
    if V not in _stages:
        _stages[V] = Stage(64, 4, 1, V, 0, 1, dtype="bf16", max_batch=4, max_ctx=16, seed=2)
    return _stages[V]


def logits(kind, V, seed):
    """The shared fixtures: computed once, never written."""
    key = (kind, V, seed)
    if key not in _logits:
        a = ref.fixture(kind, V, seed)
        a.setflags(write=False)
        _logits[key] = a
    return _logits[key]


def draw(g, l, state, pos, slot=0):
    k, p, temp, seed = state
    g.set_row_sampler(slot, top_k=k, top_p=p, temperature=temp, seed=seed)
    tok = g.sample_logits(l.reshape(1, -1), [pos], slot=slot)
    d = g.read_row_draw(slot)
    assert d["token"] == int(tok[0]) and d["position"] == pos
    return d


@pytest.mark.parametrize("kind,fseed", FIXTURES)
@pytest.mark.parametrize("V", VOCABS)
def test_draws_pass_the_checker(V, kind, fseed):
    g, l = stage(V), logits(kind, V, fseed)
    for i, (k, p, temp) in enumerate(states(V)):
        for pos in POSITIONS:
            st = (k, p, temp, 1000 + 17 * i)
            d = draw(g, l, st, pos)
            what = f"V={V} {kind}{fseed} state {i} pos {pos}"
            ref.check_readout(l, st, pos, d, what)
            if kind == "spike" and (p < 1.0 or k == 1):  # top_p == 1 keeps N = C
                assert d["n_nucleus"] == 1 and d["token"] == int(np.argmax(l)), what
            if kind == "equal":  # one level: the pick is exactly floor(u24 * V / 2^24)
                assert d["n_nucleus"] == V and d["token"] == d["u24"] * V // 2 ** 24, what
            if k == 1:
                assert d["n_candidates"] == int((l == l.max()).sum()), what


@pytest.mark.parametrize("V", VOCABS)
def test_three_rows_three_states_and_a_row_without_state(V):
    """B = 3 at slot 1 of max_batch 4, ld > V (the padding holds huge values no row may see), three different
    states; then row 2 loses its state and takes the first index of its largest logit."""
    g = stage(V)
    ld = V + 16
    rows = np.full((3, ld), 1e30, np.float32)
    src = [logits("normal", V, 0), logits("tied", V, 0), logits("normal", V, 2)]
    for b in range(3):
        rows[b, :V] = src[b]
    sts = [(0, 0.9, 1.0, 5), (50, 0.95, 1.3, 6), (0, 1.0, 0.7, 7)]
    pos = [3, 2 ** 20, 0]
    g.clear_row_sampler()
    g.set_row_sampler(1, top_k=[s[0] for s in sts], top_p=[s[1] for s in sts], temperature=[s[2] for s in sts],
                      seed=[s[3] for s in sts], count=3)
    tok = g.sample_logits(rows, pos, slot=1)
    for b in range(3):
        d = g.read_row_draw(1 + b)
        assert d["token"] == int(tok[b]) and d["position"] == pos[b]
        ref.check_readout(src[b], sts[b], pos[b], d, f"V={V} row {1 + b}")
    first = [g.read_row_draw(1 + b) for b in range(3)]
    g.clear_row_sampler(2)
    tok2 = g.sample_logits(rows, pos, slot=1)
    assert int(tok2[1]) == ref.first_argmax(src[1]) and g.read_row_draw(2)["token"] == int(tok2[1])
    assert g.read_row_draw(1) == first[0] and g.read_row_draw(3) == first[2]  # the neighbours' draws did not move
    g.clear_row_sampler()
    tok3 = g.sample_logits(rows, pos, slot=1)
    assert [int(t) for t in tok3] == [ref.first_argmax(s) for s in src]


@pytest.mark.parametrize("V", VOCABS)
def test_row_and_batch_independence_and_determinism(V):
    """The same logits, state and position in row 0 alone and in row 3 of a batch of three give the same token and
    read-out, bit for bit; so do two runs."""
    g = stage(V)
    l, other = logits("normal", V, 1), logits("tied", V, 0)
    for st, pos in (((0, 0.9, 1.0, 42), 7), ((50, 0.95, 1.3, 43), 2 ** 20)):
        g.clear_row_sampler()
        a = draw(g, l, st, pos, slot=0)
        b = draw(g, l, st, pos, slot=0)
        assert a == b, "two runs differ"
        g.clear_row_sampler()
        g.set_row_sampler(1, top_k=[0, 5, st[0]], top_p=[1.0, 0.5, st[1]], temperature=[0.7, 1.0, st[2]],
                          seed=[1, 2, st[3]], count=3)
        tok = g.sample_logits(np.stack([other, other, l]), [0, 1, pos], slot=1)
        c = g.read_row_draw(3)
        assert c == a and int(tok[2]) == a["token"], f"V={V}: row 3 of a batch of 3 differs from row 0 alone"
        tok_b = g.sample_logits(np.stack([other, l]), [1, pos], slot=2)  # another batch size
        assert g.read_row_draw(3) == a and int(tok_b[1]) == a["token"]
    g.clear_row_sampler()


def test_range_checks():
    g = stage(512)
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(temperature=0.0),
                dict(temperature=-1.0), dict(temperature=float("nan"))):
        with pytest.raises(BloomStageError, match="error -1"):
            g.set_row_sampler(0, **bad)
    with pytest.raises(BloomStageError, match="error -1"):
        g.set_row_sampler(3, count=2)
    with pytest.raises(BloomStageError, match="error -1"):
        g.sample_logits(np.zeros((1, 256), np.float32), [0])  # ld < vocab
    with pytest.raises(BloomStageError, match="error -1"):
        g.sample_logits(np.zeros((1, 512), np.float32), [-1])
