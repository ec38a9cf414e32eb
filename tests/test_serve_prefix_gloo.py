"""serve's --shared-prefix on CPU (gloo ranks, stage math = the CPU checker): the template pass, fork_row and the
continuation prefill through 1 and 2 ranks.  Forking the template returns the samples of every sample prefilling the
prefix itself, and both equal the single-stage checker run on each sample alone, chunked the same way."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_inference_demo_amd.serve import RunConfig, run_rank, synthetic_prompts
from oracle.oracle import OracleStage
from test_pipeline_gloo import MODEL, SEED, OracleExecutor, _free_port

P = 4
_R = np.random.default_rng(17)
PREFIX = _R.integers(0, MODEL.vocab, size=P).tolist()
PROMPTS = [PREFIX + _R.integers(0, MODEL.vocab, size=n - P).tolist() for n in (5, 9, 6, 7, 5)]
CFG = RunConfig(model=MODEL, num_sample=5, max_length=5, core_pool_size=2, dtype="fp32", shared_prefix=P)


class ForkingExecutor(OracleExecutor):
    """The gloo tests' executor plus fork_kv, built from the checker's read_kv / write_kv."""

    def __init__(self, lb, le, *a, **kw):
        super().__init__(lb, le, *a, **kw)
        self.layers = le - lb

    def fork_kv(self, src, dst, npos, count=1):
        nh = self.model.n_head
        hd = self.model.hidden // nh
        for l in range(self.layers):
            kv = np.array([[[self.st.read_kv(l, w, src, h, p, hd) for p in range(npos)] for h in range(nh)]
                           for w in range(2)], np.float32)
            for d in range(dst, dst + count):
                self.st.write_kv(l, d, 0, kv)


def _reference(prompts, max_length, p):
    """Each sample alone: the prefix, the remainder at past = p, then greedy decode."""
    out = []
    for q in prompts:
        st = OracleStage(MODEL.hidden, MODEL.n_head, MODEL.n_layer, MODEL.vocab, 0, MODEL.n_layer, max_batch=1,
                         max_ctx=len(q) + max_length + 1, seed=SEED)
        st.forward(np.array(q[:p], np.int32).reshape(1, -1), 1, p)
        tok = st.forward(np.array(q[p:], np.int32).reshape(1, -1), 1, len(q) - p, past_len=p)
        ids = [int(tok[0])]
        for i in range(max_length - 1):
            tok = st.forward(tok.reshape(1, 1), 1, 1, past_len=len(q) + i)
            ids.append(int(tok[0]))
        out.append(ids)
    return out


def _check(on, off):
    assert on["samples"] == off["samples"] == _reference(PROMPTS, CFG.max_length, P)
    assert (on["shared_prefix"], on["prefix_fork"], off["prefix_fork"]) == (P, True, False)
    lens = [len(q) for q in PROMPTS]
    assert on["prefill_tokens"] == P + sum(n - P for n in lens) and off["prefill_tokens"] == sum(lens)
    assert on["rounds"] == off["rounds"]


def _run(cfg, rank=0, world=1, prompts=PROMPTS):
    return run_rank(cfg, rank, world, torch.device("cpu"), prompts=prompts if rank == 0 else None,
                    executor_factory=ForkingExecutor)


def test_fork_on_and_off_single_rank():
    _check(_run(CFG), _run(RunConfig(**{**CFG.__dict__, "prefix_fork": False})))


def _worker(rank, world, port, q, head_split):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      OMP_NUM_THREADS="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = [_run(RunConfig(**{**CFG.__dict__, "head_split": head_split, "prefix_fork": fork}), rank, world)
               for fork in (True, False)]
        if rank == 0:
            q.put(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("head_split", [True, False])
def test_fork_on_and_off_two_ranks(head_split):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, head_split)) for r in range(2)]
    for p in procs:
        p.start()
    on, off = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert on["stages"] == 2
    _check(on, off)


def test_synthetic_prompts_share_prompt_zeros_prefix():
    cfg = RunConfig(model=MODEL, num_sample=3, prompt_len=7, shared_prefix=3)
    ps = synthetic_prompts(cfg, MODEL.vocab)
    plain = synthetic_prompts(RunConfig(model=MODEL, num_sample=3, prompt_len=7), MODEL.vocab)
    assert all(q[:3] == plain[0][:3] and q[3:] == o[3:] for q, o in zip(ps, plain))
    with pytest.raises(ValueError):
        synthetic_prompts(RunConfig(model=MODEL, num_sample=3, prompt_len=3, shared_prefix=3), MODEL.vocab)


@pytest.mark.parametrize("bad", [dict(shared_prefix=-1), dict(prefill=False), dict(score=True), dict(max_length=0),
                                 dict(speculate=2), dict(sample=True, sample_speculate=2)])
def test_config_validation(bad):
    with pytest.raises(ValueError):
        RunConfig(**{**CFG.__dict__, **bad})


def test_prompt_validation():
    with pytest.raises(ValueError, match="differ"):
        _run(CFG, prompts=PROMPTS[:4] + [[PREFIX[0] ^ 1] + PROMPTS[4][1:]])
    with pytest.raises(ValueError, match="longer"):
        _run(CFG, prompts=PROMPTS[:4] + [PREFIX])
    with pytest.raises(ValueError, match="longer"):
        _run(CFG, prompts=PROMPTS[:4] + [PREFIX[:2]])


def test_defaults_leave_an_ordinary_run_as_it_is():
    from test_serve_gloo import _reference as whole_prompt_reference
    c = RunConfig()
    assert c.shared_prefix == 0 and c.prefix_fork is True
    cfg = RunConfig(model=MODEL, num_sample=5, max_length=5, core_pool_size=2, dtype="fp32")
    res = _run(cfg)
    assert res["samples"] == whole_prompt_reference(PROMPTS, 5)
    assert sorted(res) == sorted(["samples", "num_sample", "max_length", "core_pool_size", "stages", "prompt_lens",
                                  "rounds", "prefill", "seconds", "tokens_per_s"])
