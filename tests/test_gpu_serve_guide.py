"""serve's guided-decoding options on one GPU (fp32 tiny model, 2 rows in flight, ragged prompts): with --choice three
times every sample's tokens are one of the choices followed only by the EOS, and equal a per-sample loop over the fp32
CPU checker's logits with the references (tests/logit_proc_ref.py, then tests/guide_ref.py, then the first-index argmax
or, with --sample, tests/row_sampling_ref.py) -- alone, with --sample, with --repetition-penalty, with --shared-prefix
and on an int8 KV cache; --guide-file through the command line; the per-sample records; the exclusions."""
import json

import numpy as np
import pytest
import torch

import guide_ref as gref
import logit_proc_ref as ref
import row_sampling_ref as sref
from distributed_inference_demo_amd import config
from distributed_inference_demo_amd import guide as gd
from distributed_inference_demo_amd.serve import RunConfig, main, request_seed, run_rank
from oracle.oracle import OracleStage

pytestmark = pytest.mark.gpu

M = config.get("tiny")  # hidden 64, 4 layers, 4 heads, V 512; by name on the command line
SEED, N_NEW, EOS = 13, 8, 41
P = 3
PREFIX = [7, 300, 41]
PROMPTS = [PREFIX + [3, 17, 200, EOS], PREFIX + [EOS], PREFIX + [500, 1, 2, 3, 4, 5, EOS], PREFIX + [9, 9, EOS],
           PREFIX + [88, 17]]
CHOICES = ([17], [17, 200, 9], [300, 88, 3, 500, 1])  # two share their first token, one is a prefix of another
SAMPLING = dict(sample=True, top_k=40, top_p=0.9, temperature=1.5, sample_seed=5)


def cfg(**kw):
    base = dict(model=M, num_sample=len(PROMPTS), max_length=N_NEW, core_pool_size=2, seed=SEED, dtype="fp32",
                choice=tuple(",".join(map(str, c)) for c in CHOICES), eos_id=EOS)
    base.update(kw)
    return RunConfig(**base)


def serve(c):
    return run_rank(c, 0, 1, torch.device("cuda", 0), prompts=PROMPTS)


@pytest.fixture(scope="module")
def checker():
    o = OracleStage(M.hidden, M.n_head, M.n_layer, M.vocab, 0, M.n_layer, bf16=False, max_batch=1, max_ctx=32, seed=SEED)
    yield lambda T: o.forward(np.asarray(T, np.int32), 1, len(T), slot=0, past_len=0, want_logits=True)[1][0]
    o.close()


def by_reference(c, fn):
    guide = c.make_guide(M.vocab)
    p = ref.params(**c.processors) if c.processors else None
    out = []
    for i, prompt in enumerate(PROMPTS):
        pick = None
        if c.sample:
            seed = request_seed(c.sample_seed, i)
            pick = lambda l, pos: sref.reference(l, c.top_k, c.top_p, c.temperature, seed, pos)["token"]  # noqa: E731
        out.append(gref.generate(fn, prompt, guide, N_NEW, proc=p, pick=pick)[0])
    return out


def ends_in_a_choice(res):
    for s, r in zip(res["samples"], res["guide_records"]):
        n = s.index(EOS)
        assert s[:n] in [list(c) for c in CHOICES] and set(s[n:]) == {EOS}, s
        assert r["n_rejected"] == 0 and r["eos_at"] == n
    sink = {r["state"] for r in res["guide_records"]}
    assert len(sink) == 1, "every sample ends in the sink"


@pytest.mark.parametrize("extra", [{}, SAMPLING, dict(repetition_penalty=3.0), dict(repetition_penalty=1.3, **SAMPLING),
                                   dict(shared_prefix=P), dict(shared_prefix=P, token_bias=("300:-2.0",), **SAMPLING)],
                         ids=["choice", "sample", "penalty", "penalty+sample", "shared-prefix", "prefix+bias+sample"])
def test_choices_equal_the_reference_loop(checker, extra):
    c = cfg(**extra)
    res = serve(c)
    ends_in_a_choice(res)
    assert res["samples"] == by_reference(c, checker)
    assert res["guide"]["choice"] == [list(x) for x in CHOICES]


def test_the_guide_changes_the_output_and_the_penalty_changes_the_choice():
    plain = serve(cfg(choice=()))
    assert "guide" not in plain
    a, b = serve(cfg())["samples"], serve(cfg(repetition_penalty=3.0))["samples"]
    assert a != plain["samples"] and a != b


def test_int8_kv_still_ends_in_a_choice():
    c = cfg(kv="int8", dtype="bf16")
    res = serve(c)
    ends_in_a_choice(res)
    assert serve(c)["samples"] == res["samples"]


def test_guide_file_on_the_command_line(tmp_path, checker):
    """A default-allow machine from a file: after 300 the tokens 41, 17 and 300 itself are banned by explicit edges."""
    V = M.vocab
    free = {t: ("after300" if t == 300 else "free") for t in range(V)}
    maps = {"free": free, "after300": {t: v for t, v in free.items() if t not in (EOS, 17, 300)}}
    guide = gd.from_state_maps(maps, "free", [], -1, V)
    assert guide.default_next.min() >= 0
    gf, pf, out = tmp_path / "guide.json", tmp_path / "prompts.json", tmp_path / "out.json"
    gf.write_text(guide.to_json())
    prompts = [[300], [5, 300], [300, 300, 7]]  # the synthetic model echoes: plain greedy would repeat 300
    pf.write_text(json.dumps(prompts))
    main(["--model", "tiny", "--num-sample", "3", "--max-length", "4", "--core-pool-size", "2", "--seed", str(SEED),
          "--dtype", "fp32", "--prompts-file", str(pf), "--out", str(out), "--guide-file", str(gf)])
    got = json.loads(out.read_text())
    assert got == [gref.generate(checker, p, guide, 4)[0] for p in prompts]
    assert got != [ref.generate(checker, p, ref.params(), 4)[0] for p in prompts], "the guide bites"


def test_exclusions():
    for kw in (dict(speculate=2), dict(sample=True, sample_speculate=2), dict(num_beams=2), dict(score=True),
               dict(max_length=0), dict(prefill=False), dict(eos_id=-1), dict(guide_file="g.json")):
        with pytest.raises(ValueError):
            cfg(**kw)
    with pytest.raises(ValueError, match="executor_factory"):
        run_rank(cfg(), 0, 1, torch.device("cuda", 0), prompts=PROMPTS, executor_factory=lambda *a, **k: None)
    with pytest.raises(ValueError, match="vocab"):
        serve(cfg(choice=("512",)))
