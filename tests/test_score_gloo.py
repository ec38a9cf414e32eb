"""The scoring task's pipeline protocol on CPU (gloo): pipeline.score on 1, 2 and 3 ranks and serve --score on one.
Each rank's stage math is the CPU checker; the last rank's executor scores teacher-forced (one position a call, with
logits), the twin of test_pipeline_gloo.OracleExecutor with a `score` method.  Rank 0's result equals one whole-model
checker stage scoring the same prompts."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_inference_demo_amd.pipeline import build_rank, score
from distributed_inference_demo_amd.serve import RunConfig, run_rank
from oracle.oracle import OracleStage, prompt_ids
from test_pipeline_gloo import MB, MODEL, SEED, _free_port

P = 6
TOL = 1e-4  # fp32 checker: a prefill through the earlier stages against one whole-model stage stepping a token a call


def teacher_forced(st, x, B, S, slot=0, past_len=0):
    """float64 logits [B][S][V] of a last checker stage, one position a call."""
    x = np.asarray(x)
    x = x.reshape(B, S) if st.is_first else x.reshape(B, S, st.hidden)
    lg = np.empty((B, S, st.vocab), np.float64)
    for t in range(S):
        _, l = st.forward(x[:, t:t + 1], B, 1, slot=slot, past_len=past_len + t, want_logits=True)
        lg[:, t] = l
    return lg


def scores_of(lg, targets):
    """(top_ids, scores [..][3]) of bs_forward_score from logits, in float64."""
    mx = lg.max(axis=-1)
    lse = mx + np.log(np.exp(lg - mx[..., None]).sum(axis=-1))
    tg = np.asarray(targets)
    has = (tg >= 0) & (tg < lg.shape[-1])
    lt = np.take_along_axis(lg, np.where(has, tg, 0)[..., None].astype(np.int64), axis=-1)[..., 0]
    return lg.argmax(axis=-1).astype(np.int32), np.stack([np.where(has, lt - lse, 0.0), mx - lse, lse], axis=-1)


class ScoreExecutor:
    def __init__(self, lb, le, first, last, max_batch, max_ctx, hslice=None, model=MODEL):
        self.st = OracleStage(model.hidden, model.n_head, model.n_layer, model.vocab, lb, le, max_batch=max_batch,
                              max_ctx=max_ctx, seed=SEED, is_first=first, is_last=last)

    def forward(self, inp, out, batch, seq, slot, past_len):
        y = self.st.forward(inp.numpy(), batch, seq, slot=slot, past_len=past_len)
        out.copy_(torch.from_numpy(np.ascontiguousarray(y).reshape(-1)[: out.numel()]).view(out.shape))

    def score(self, inp, targets, top_ids, scores, batch, seq, slot, past_len):
        lg = teacher_forced(self.st, inp.numpy(), batch, seq, slot, past_len)
        tg = np.full((batch, seq), -1) if targets is None else targets.numpy().reshape(batch, seq)
        top, sc = scores_of(lg, tg)
        if top_ids is not None:
            top_ids.copy_(torch.from_numpy(top).view(top_ids.shape))
        if scores is not None:
            scores.copy_(torch.from_numpy(sc.astype(np.float32)).view(scores.shape))


def _single_stage(prompt):
    B, S = prompt.shape
    ref = OracleStage(MODEL.hidden, MODEL.n_head, MODEL.n_layer, MODEL.vocab, 0, MODEL.n_layer, max_batch=B,
                      max_ctx=S + 1, seed=SEED)
    lg = teacher_forced(ref, prompt, B, S)
    tg = np.full((B, S), -1)
    tg[:, :-1] = prompt[:, 1:]
    return lg, scores_of(lg, tg)


def _check(got_top, got_sc, prompt):
    lg, (top, sc) = _single_stage(prompt)
    assert got_top.shape == top.shape and got_sc.shape == sc.shape
    assert np.abs(got_sc - sc).max() <= TOL, np.abs(got_sc - sc).max()
    assert np.all(got_sc[:, -1, 0] == 0.0)
    for b, t in zip(*np.nonzero(got_top != top)):  # a near-tie may pick either
        two = np.sort(lg[b, t])[-2:]
        assert two[1] - two[0] < TOL, (b, t, got_top[b, t], top[b, t], two)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      OMP_NUM_THREADS="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pipe, _ = build_rank(MODEL, rank, world, torch.device("cpu"), mb_rows=MB, max_ctx=P + 1, max_seq=P,
                             executor_factory=ScoreExecutor, dtype="fp32", head_split=False)
        out = []
        for seed in (1234, 99):  # two passes: the KV rows are reused from position 0
            prompt = torch.from_numpy(prompt_ids(seed, MB * pipe.n_mb, P, MODEL.vocab)) if rank == 0 else None
            res = score(pipe, prompt, P)
            assert (res is None) == (rank != 0)
            if rank == 0:
                out.append((res[0].numpy().copy(), res[1].numpy().copy()))
        if rank == 0:
            q.put(out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_pipeline_score_matches_single_stage(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for seed, (top, sc) in zip((1234, 99), out):
        _check(top, sc, prompt_ids(seed, MB * world, P, MODEL.vocab))


def test_single_rank_pipeline_scores_without_hops():
    pipe, _ = build_rank(MODEL, 0, 1, torch.device("cpu"), mb_rows=MB, n_mb=2, max_ctx=P + 1, max_seq=P,
                         executor_factory=ScoreExecutor, dtype="fp32")
    for seed in (1234, 99):
        prompt = prompt_ids(seed, 2 * MB, P, MODEL.vocab)
        top, sc = score(pipe, torch.from_numpy(prompt), P)
        _check(top.numpy(), sc.numpy(), prompt)


def test_score_rejects_a_split_head():
    class _Pipe:
        head_split = True
    with pytest.raises(ValueError, match="head_split"):
        score(_Pipe(), None, P)


def test_serve_score_reports_per_sample_perplexity():
    """serve --score on one rank, ragged prompts, 3 rows a pass (padded at the tail, a short last pass): every
    sample's log-likelihood, token count and perplexity against the checker scoring that sample alone."""
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, MODEL.vocab, size=n).tolist() for n in (5, 9, 2, 9, 1, 7, 4)]
    cfg = RunConfig(model=MODEL, num_sample=len(prompts), core_pool_size=3, dtype="fp32", score=True)
    res = run_rank(cfg, 0, 1, torch.device("cpu"), prompts=prompts, executor_factory=ScoreExecutor)
    assert res["task"] == "score" and res["passes"] == 3 and len(res["samples"]) == len(prompts)
    for p, got in zip(prompts, res["samples"]):
        ids = np.array(p, np.int32).reshape(1, -1)
        _, (_, sc) = _single_stage(ids)
        ll = float(sc[0, :-1, 0].sum())
        assert got["tokens"] == len(p) - 1
        assert abs(got["loglik"] - ll) <= TOL * max(1, len(p))
        if len(p) > 1:
            assert got["perplexity"] == pytest.approx(np.exp(-ll / (len(p) - 1)), rel=1e-4)
        else:
            assert got["perplexity"] is None
