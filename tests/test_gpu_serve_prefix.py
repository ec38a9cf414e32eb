"""serve's --shared-prefix on one GPU: forking the template row returns token for token what every sample prefilling
the prefix itself returns (greedy and sampled, bf16 and int8 KV cache), a hand-driven Stage chunked the same way
reproduces the tokens, and prefill_tokens counts the prefix once."""
import numpy as np
import pytest
import torch

from distributed_inference_demo_amd.config import BloomDims
from distributed_inference_demo_amd.serve import RunConfig, run_rank
from distributed_inference_demo_amd.stage import Stage

pytestmark = pytest.mark.gpu

M = BloomDims("tiny-sample", 64, 2, 4, vocab=512)
P = 6
_R = np.random.default_rng(31)
PREFIX = _R.integers(0, M.vocab, size=P).tolist()
PROMPTS = [PREFIX + _R.integers(0, M.vocab, size=n - P).tolist() for n in (7, 13, 9, 8, 11)]
LENS = [len(p) for p in PROMPTS]
SAMPLING = dict(sample=True, top_k=30, top_p=0.9, temperature=1.5, sample_seed=5)


def cfg(**kw):
    base = dict(model=M, num_sample=5, max_length=6, core_pool_size=2, seed=13, shared_prefix=P)
    base.update(kw)
    return RunConfig(**base)


def serve(c):
    return run_rank(c, 0, 1, torch.device("cuda", 0), prompts=PROMPTS)


@pytest.mark.parametrize("kv", ["bf16", "int8"])
@pytest.mark.parametrize("sampling", [{}, SAMPLING], ids=["greedy", "sample"])
def test_fork_on_equals_fork_off(kv, sampling):
    on = serve(cfg(kv=kv, **sampling))
    off = serve(cfg(kv=kv, prefix_fork=False, **sampling))
    assert on["samples"] == off["samples"]
    assert all(len(s) == 6 and all(0 <= t < M.vocab for t in s) for s in on["samples"])
    assert (on["shared_prefix"], on["prefix_fork"], off["prefix_fork"]) == (P, True, False)
    assert on["prefill_tokens"] == P + sum(n - P for n in LENS)
    assert off["prefill_tokens"] == sum(LENS)
    assert on["rounds"] == off["rounds"] and on["prompt_lens"] == LENS


def test_a_hand_driven_stage_reproduces_the_tokens():
    """Per sample: the prefix pass, the remainder at past 6, then the decode batches of the run's schedule.  With two
    rows in flight serve decodes B = 2 batches; a batched decode row equals the B = 1 step bit for bit only by
    kernel choice, so the hand-driven loop replays the same batches: one run of the schedule with own prefills."""
    from distributed_inference_demo_amd.serve import admission_schedule
    res = serve(cfg())
    sched, T = admission_schedule(LENS, 6, 2)
    g = Stage(M.hidden, M.n_head, M.n_layer, M.vocab, 0, M.n_layer, dtype="bf16", max_batch=2,
              max_ctx=max(LENS) + 7, max_tokens=2 * max(LENS), seed=13)
    admit = {}
    for i, (r, t0) in enumerate(sched):
        admit.setdefault(t0, []).append((i, r))
    out = [[] for _ in PROMPTS]
    cur, owner, pos = [0, 0], [None, None], [0, 0]
    for t in range(T + 1):
        for i, r in admit.get(t, ()):
            g.forward_host(np.array([PROMPTS[i][:P]], np.int32), 1, P, slot=r, past_len=0)
            tok = g.forward_host(np.array([PROMPTS[i][P:]], np.int32), 1, LENS[i] - P, slot=r, past_len=P)
            out[i].append(int(tok[0]))
            cur[r], owner[r], pos[r] = int(tok[0]), i, LENS[i]
        if t == T:
            break
        for r in range(2):  # a row whose sample is done idles on token 0 at position 0, as in serve
            if owner[r] is None or len(out[owner[r]]) == 6:
                cur[r], owner[r], pos[r] = 0, None, 0
        toks = g.forward_host(np.array(cur, np.int32).reshape(2, 1), 2, 1, slot=0, past_len=list(pos))
        for r in range(2):
            cur[r], pos[r] = int(toks[r]), pos[r] + 1
            if owner[r] is not None:
                out[owner[r]].append(int(toks[r]))
    assert res["samples"] == out
    g.close()
