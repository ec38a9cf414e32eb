"""Guided decoding on the host (no GPU): the builders and the JSON form of distributed_inference_demo_amd/guide.py,
Guide.validate against every malformed table bs_load_guide names, the numpy reference (tests/guide_ref.py) bitwise
against the installed transformers PrefixConstrainedLogitsProcessor -- alone and chained behind the processors of
tests/logit_proc_ref.py, which pins the order -- serve's RunConfig validation, and the ctypes struct against the header.

One translation separates transformers' output from the rule's: a ban is -inf there and -FLT_MAX here.  And
PrefixConstrainedLogitsProcessor adds a dense mask (0 where allowed), so an allowed -0.0 comes out as +0.0; the rule
does not touch allowed logits.  The comparison therefore maps the reference's zeros through `+ 0.0` as well, which
changes only the sign of a zero (tests/test_logit_proc_host.py does the same for transformers' dense bias add)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from transformers.generation.logits_process import (LogitsProcessorList, PrefixConstrainedLogitsProcessor,
                                                    RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor)

import guide_ref as gref
import logit_proc_ref as ref
from distributed_inference_demo_amd import guide as gd
from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.serve import RunConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 64
EOS = 7


def accepts(guide, seq):
    q, rej = guide.walk(seq)
    return rej == 0, q


# ---- builders
def test_choices_with_shared_prefixes_a_prefix_choice_and_duplicates():
    choices = [[5, 6, 9], [5, 6, 10, 11], [5, 8], [5, 6], [5, 8], [12]]  # [5, 6] is a prefix of two others; [5, 8] twice
    g = gd.from_choices(choices, EOS).validate(V)
    assert g.default_next.max() < 0, "a trie state allows a handful of tokens: default-ban"
    assert g.allowed(g.start).tolist() == [5, 12]
    q56 = g.walk([5, 6])[0]
    assert g.allowed(q56).tolist() == [EOS, 9, 10], "a choice that is a prefix of another may end or go on"
    sinks = set()
    for c in choices:
        ok, q = accepts(g, c + [EOS])
        assert ok and g.allowed(q).tolist() == [EOS] and g.step(q, EOS) == q, "the sink allows only the EOS, for ever"
        sinks.add(q)
    assert len(sinks) == 1
    q = g.walk([5, 6, 9])[0]
    assert g.allowed(q).tolist() == [EOS], "a finished choice that is no prefix enters the sink directly"
    for wrong in ([6], [5, 9], [5, 6, 9, 9], [5, 6, 10, EOS], [EOS], [12, 12]):
        assert not accepts(g, wrong)[0], wrong
    assert g.n_states == 4 + 1, "(),(5), (5, 6), (5, 6, 10) and the sink: duplicates add nothing"
    assert gd.from_choices(choices, EOS).to_json() == gd.from_choices(choices[::-1], EOS).to_json()
    with pytest.raises(ValueError):
        gd.from_choices([], EOS)
    with pytest.raises(ValueError):
        gd.from_choices([[1], []], EOS)


def test_state_maps_take_the_denser_encoding_per_state():
    most = {t: "free" for t in range(V) if t not in (3, 4)}
    most[9] = "digits"
    maps = {"free": most, "digits": {1: "digits", 2: "digits", 9: "free"}}
    g = gd.from_state_maps(maps, "free", ["digits"], EOS, V).validate(V)
    names = {n: i for i, n in enumerate(sorted(maps))}  # states are numbered in sorted order, the sink last
    free, digits, sink = names["free"], names["digits"], g.n_states - 1
    assert g.n_states == 3 and g.start == free
    assert g.default_next[free] == free and g.default_next[digits] == -1 and g.default_next[sink] == -1
    lo, hi = g.row_ptr[free], g.row_ptr[free + 1]
    assert g.edge_token[lo:hi].tolist() == [3, 4, 9] and g.edge_next[lo:hi].tolist() == [-1, -1, digits]
    assert g.allowed(free, V).tolist() == sorted(most) and g.allowed(digits).tolist() == [1, 2, EOS, 9]
    assert g.step(digits, EOS) == sink and g.step(free, EOS) == free and g.allowed(sink).tolist() == [EOS]
    with pytest.raises(ValueError, match="needs the vocabulary size"):
        g.allowed(free)
    for q in range(g.n_states):  # both encodings say the same as the maps
        assert gref.allowed_mask(g, q, V).nonzero()[0].tolist() == g.allowed(q, V).tolist()
    # a small vocabulary turns a trie state default-allow as well
    small = gd.from_choices([[0], [1], [2]], 3, vocab=4)
    assert small.default_next[0] >= 0 and small.allowed(0, 4).tolist() == [0, 1, 2]
    # a state nobody describes allows nothing: refused, with its number
    with pytest.raises(ValueError, match="no token is allowed in state"):
        gd.from_state_maps({0: {1: 5}}, 0, [], EOS, V)


def test_json_round_trip_holds_only_the_tables(tmp_path):
    g = gd.from_choices([[5, 6, 9], [5, 8]], EOS)
    text = g.to_json()
    import json
    assert sorted(json.loads(text)) == sorted(("n_states", "start") + gd.TABLES)
    h = gd.Guide.from_json(text)
    assert h.n_states == g.n_states and h.start == g.start
    assert all(np.array_equal(getattr(g, k), getattr(h, k)) and getattr(h, k).dtype == np.int32 for k in gd.TABLES)
    path = tmp_path / "g.json"
    path.write_text(text)
    assert gd.Guide.from_file(str(path)).to_json() == text


def raw(n, start, row_ptr, tok, nxt, dn):
    return gd.Guide(n, start, row_ptr, tok, nxt, dn)


BAD = {
    "n_states = 0": (raw(0, 0, [0], [], [], []), "n_states"),
    "n_states > 2^20": (raw((1 << 20) + 1, 0, [0], [], [], []), "n_states"),
    "start": (raw(1, 1, [0, 1], [5], [0], [-1]), "start"),
    "negative start": (raw(1, -1, [0, 1], [5], [0], [-1]), "start"),
    "row_ptr[0]": (raw(1, 0, [1, 1], [5], [0], [0]), "start at 0"),
    "row_ptr decreases": (raw(2, 0, [0, 1, 0], [5], [0], [0, 0]), "decreases at state 1"),
    "descending tokens": (raw(2, 0, [0, 0, 2], [6, 5], [0, 0], [0, -1]), "ascending in state 1"),
    "a token twice": (raw(1, 0, [0, 2], [5, 5], [0, 0], [-1]), "ascending in state 0"),
    "token = vocab": (raw(1, 0, [0, 1], [V], [0], [-1]), r"\[0, vocab\) in state 0"),
    "negative token": (raw(1, 0, [0, 1], [-1], [0], [0]), r"\[0, vocab\) in state 0"),
    "edge_next = n_states": (raw(2, 0, [0, 0, 1], [5], [2], [0, -1]), "edge_next .* in state 1"),
    "edge_next < -1": (raw(1, 0, [0, 1], [5], [-2], [0]), "edge_next .* in state 0"),
    "default_next = n_states": (raw(2, 0, [0, 0, 0], [], [], [0, 2]), "default_next .* in state 1"),
    "default_next < -1": (raw(1, 0, [0, 0], [], [], [-2]), "default_next .* in state 0"),
    "default-ban, no allowed edge": (raw(2, 0, [0, 1, 2], [5, 5], [0, -1], [-1, -1]), "no token is allowed in state 1"),
    "default-allow, every token banned": (raw(1, 0, [0, 4], [0, 1, 2, 3], [-1] * 4, [0]), "no token is allowed in state 0"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_validate_rejects(name):
    g, msg = BAD[name]
    with pytest.raises(ValueError, match=msg):
        g.validate(4 if "every token banned" in name else V)


def test_validate_accepts_the_smallest_guides():
    raw(1, 0, [0, 0], [], [], [0]).validate(1)
    raw(1, 0, [0, 1], [0], [0], [-1]).validate(1)


# ---- the reference against transformers
def logits_fixture(seed):
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal(V) * 3).astype(np.float32)
    l[3], l[4], l[5], l[6] = 0.0, -0.0, 2.5, -2.5
    return l


def machine():
    """A default-ban start, a default-allow state with bans, a state where the two zeros are allowed."""
    return gd.from_state_maps({"s": {3: "z", 5: "a", 9: "a"},
                               "a": {t: ("z" if t in (4, 6) else "a") for t in range(V) if t not in (0, 5, V - 1)},
                               "z": {3: "s", 4: "s", 6: "a"}}, "s", ["a"], EOS, V)


def hf_fn(guide, prompt_len):
    def fn(batch_id, sent):
        q, rej = guide.walk(sent[prompt_len:].tolist())
        assert rej == 0
        return guide.allowed(q, V).tolist()
    return fn


def hf_apply(procs, history, logits):
    out = procs(torch.tensor([history], dtype=torch.int64), torch.tensor(logits, dtype=torch.float32)[None].clone())
    out = out[0].numpy().copy()
    assert not np.isnan(out).any()
    out[np.isneginf(out)] = ref.BAN
    return out


@pytest.mark.parametrize("generated", [[], [5], [5, 10, 4], [3], [3, 4, 9, 11, 6, 3], [9, 12, EOS, EOS]])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_transformers_bitwise(generated, seed):
    g = machine()
    prompt = [3, 1, 5]  # the guide never sees it
    l = logits_fixture(seed)
    q, rej = g.walk(generated)
    assert rej == 0
    want = hf_apply(LogitsProcessorList([PrefixConstrainedLogitsProcessor(hf_fn(g, len(prompt)), 1)]),
                    prompt + generated, l)
    got = gref.apply(l, g, q)
    allowed = g.allowed(q, V)
    assert np.array_equal(np.flatnonzero(want != ref.BAN), allowed), "the banned set"
    assert np.array_equal(np.flatnonzero(got != ref.BAN), allowed)
    assert ref.bits_equal(got[allowed], l[allowed]), "allowed logits are not touched, bit for bit"
    assert ref.bits_equal(got + np.float32(0.0), want), "module docstring: only the sign of a zero can differ"
    assert ref.first_argmax(got) == int(np.argmax(want))
    assert np.all(np.isfinite(got))


def test_the_guide_runs_behind_the_processors():
    """Chained as generate() chains them -- penalty, n-gram, then prefix_allowed_tokens_fn -- the reference chain is
    transformers' bitwise; and the order matters: a guide ahead of the penalty would multiply its own -FLT_MAX."""
    g = machine()
    prompt, generated = [3, 1, 5, 9], [5, 10, 4]
    T = prompt + generated
    p = ref.params(repetition_penalty=1.3, no_repeat_ngram=2)
    q = g.walk(generated)[0]
    procs = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=1.3), NoRepeatNGramLogitsProcessor(2),
                                 PrefixConstrainedLogitsProcessor(hf_fn(g, len(prompt)), 1)])
    for seed in (0, 1):
        l = logits_fixture(seed)
        want = hf_apply(procs, T, l)
        got = gref.apply(ref.apply(l, T, p, len(generated)), g, q)
        assert ref.bits_equal(got + np.float32(0.0), want)
        assert ref.first_argmax(got) == int(np.argmax(want))
        with np.errstate(over="ignore"):
            swapped = ref.apply(gref.apply(l, g, q), T, p, len(generated))
        assert not np.all(np.isfinite(swapped)) or not ref.bits_equal(swapped + np.float32(0.0), want)


def test_generate_loop_matches_transformers_and_counts_a_rejected_pick():
    rng = np.random.default_rng(5)
    table = (rng.standard_normal((V, V)) * 2).astype(np.float32)

    def fn(tokens):
        return table[tokens[-1]] + np.float32(0.01) * np.float32(len(tokens))

    g = machine()
    prompt = [1, 2, 3, 1]
    ids, scores, q, rej = gref.generate(fn, prompt, g, 12)
    procs = LogitsProcessorList([PrefixConstrainedLogitsProcessor(hf_fn(g, len(prompt)), 1)])
    T = list(prompt)
    for _ in range(12):
        T.append(int(np.argmax(hf_apply(procs, T, fn(T)))))
    assert ids == T[len(prompt):] and rej == 0 and (q, 0) == g.walk(ids)
    # the processors ban the start state's every allowed token: the pick is the first index, the state stays
    p = ref.params(bad_tokens=[3, 5, 9])
    ids, scores, q, rej = gref.generate(fn, prompt, g, 2, proc=p)
    assert ids == [0, 0] and q == g.start and rej == 2 and np.all(scores[0] == ref.BAN)
    assert gref.walk(g, g.start, [5, V, -1, 10], V) == (g.walk([5, 10])[0], 4, 2)


# ---- serve's options
def test_run_config_validation():
    c = RunConfig(choice=("5,6,9", [5, 8]), eos_id=2)
    assert c.choice == ((5, 6, 9), (5, 8)) and c.guided and c.head_split is False
    g = c.make_guide(V)
    assert g.walk([5, 8, 2])[1] == 0 and RunConfig().make_guide(V) is None and not RunConfig().guided
    for kw in (dict(choice=("5",)), dict(choice=("5",), eos_id=2, guide_file="x.json"), dict(choice=("",), eos_id=2),
               dict(choice=([-1],), eos_id=2)):
        with pytest.raises(ValueError):
            RunConfig(**kw)
    for kw in (dict(speculate=2), dict(sample=True, sample_speculate=2), dict(num_beams=2), dict(score=True),
               dict(max_length=0), dict(prefill=False)):
        with pytest.raises(ValueError):
            RunConfig(choice=("5",), eos_id=2, **kw)
        with pytest.raises(ValueError):
            RunConfig(guide_file="g.json", **kw)
    RunConfig(choice=("5",), eos_id=2, sample=True, repetition_penalty=1.2, shared_prefix=4, kv="int8")  # these combine
    with pytest.raises(ValueError):
        RunConfig(choice=("5", "70"), eos_id=2).make_guide(V)  # a token outside the vocabulary
    with pytest.raises(ValueError):
        RunConfig(choice=("5",), eos_id=V).make_guide(V)


def test_guide_file_option(tmp_path):
    path = tmp_path / "guide.json"
    path.write_text(machine().to_json())
    g = RunConfig(guide_file=str(path)).make_guide(V)
    assert g.to_json() == machine().to_json()
    with pytest.raises(ValueError):
        RunConfig(guide_file=str(path)).make_guide(V - 1)  # its tokens reach V - 2 ... V - 1 is banned by an edge


# ---- the binding against the header
def test_ctypes_struct_and_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "bloomstage.h")).read()
    body = re.search(r"typedef struct bs_guide_desc \{(.*?)\} bs_guide_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(2), "*" in m.group(1)) for m in re.finditer(r"(?:const\s+)?int32_t\s*(\*?)\s*(\w+)\s*;", body)]
    assert [n for n, _ in fields] == [n for n, _ in bs.GuideDesc._fields_]
    for (name, is_ptr), (_, ctype) in zip(fields, bs.GuideDesc._fields_):
        assert (ctype is ctypes.c_int32) != is_ptr and (not is_ptr or ctype == ctypes.POINTER(ctypes.c_int32)), name
    n_ptr = sum(p for _, p in fields)
    assert ctypes.sizeof(bs.GuideDesc) == 4 * (len(fields) - n_ptr) + ctypes.sizeof(ctypes.c_void_p) * n_ptr == 40
    defines = dict(re.findall(r"#define (BS_GUIDE_\w+) +\(?([\d <]+)\)?", header))
    assert int(defines["BS_GUIDE_MAX"]) == bs.BS_GUIDE_MAX == 16
    assert int(defines["BS_GUIDE_SLICE"]) == bs.BS_GUIDE_SLICE
    assert eval(defines["BS_GUIDE_MAX_STATES"]) == gd.MAX_STATES == 1 << 20
    assert {"bs_load_guide", "bs_unload_guide", "bs_set_row_guide", "bs_advance_row_guide", "bs_guide_logits",
            "bs_read_row_guide"} <= set(bs.EXPORTS)
