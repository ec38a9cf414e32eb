"""Beam search on the GPU: bs_forward_topk (Stage.forward_topk), bs_copy_kv (Stage.copy_kv), beam.BeamSearcher and
serve --num-beams.

  the tail   exact against the logits the same call returns: ids = a stable descending argsort, lse and logprobs
             within 2^-23 (|l| + |lse| + 1) + (D + 4) 2^-24 of float64, D as the kernel's header declares it
             (csrc/beam_topk.hip); ties and all-equal logits built from host weights; bit-identity across rows, runs,
             graph replay / eager launch / host I/O; the K / V rows and the next decode step against a plain twin.
  the copy   an exact copy that writes nothing else on bf16 (hd 64 and 80), fp32 and int8 caches, equal to the same
             pairs done with bs_fork_kv, and a decode step after it.
  end to end the device searcher against tests/beam_ref.py over the fp32 checker on the cases of tiny_beam.npz.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from distributed_inference_demo_amd.beam import BeamSearcher
from distributed_inference_demo_amd.config import BloomDims
from distributed_inference_demo_amd.stage import (BS_STEP_HOST_IO, BS_STEP_LOGITS, BS_STEP_VERIFY, BS_STEP_VERIFY_DRAW,
                                                  Stage, Step, lib)
from test_beam_host import CASES, G, H, L, N_NEW, N_RETURN, NH, SEED, V, case, case_id, ref_result
from test_gpu_parity import BF16_TOL, record_error
from oracle.oracle import OracleStage

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V1, V3 = 512, 2 * 2048 + 816  # one slice of 2048 logits; three slices, the last one short
MB, CTX = 3, 24


def declared_chain_length():
    src = open(os.path.join(ROOT, "distributed_inference_demo_amd", "csrc", "beam_topk.hip")).read()
    m = re.search(r"^//\s+D = [0-9+ ]+= (\d+):", src, re.M)
    assert m, "beam_topk.hip's header states D"
    return int(m.group(1))


D = declared_chain_length()


def make(dtype, vocab, **kw):
    kw.setdefault("max_batch", MB)
    kw.setdefault("max_ctx", CTX)
    kw.setdefault("seed", 5)
    return Stage(kw.pop("hidden", 64), 4, 2, vocab, 0, 2, dtype=dtype, **kw)


def check_tail(ids, lp, lse, logits, k, what):
    """ids / lp / lse of a top-k pass against the logits the same pass returned."""
    B = logits.shape[0]
    assert np.isfinite(logits).all()
    want = np.argsort(-(logits + 0.0), axis=-1, kind="stable")[:, :k]
    assert np.array_equal(ids, want), f"{what}: ids"
    l64 = logits.astype(np.float64)
    m = l64.max(-1, keepdims=True)
    lse64 = (m + np.log(np.exp(l64 - m).sum(-1, keepdims=True))).reshape(B)
    top = np.take_along_axis(l64, want, -1)
    tol_lse = 2.0 ** -23 * (np.abs(m.reshape(B)) + np.abs(lse64) + 1) + (D + 4) * 2.0 ** -24
    tol_lp = 2.0 ** -23 * (np.abs(top) + np.abs(lse64)[:, None] + 1) + (D + 4) * 2.0 ** -24
    e1 = record_error(what + " [top-k tail: lse vs float64]", lse, lse64, float(tol_lse.min()), "topk lse")
    e2 = record_error(what + " [top-k tail: logprobs vs float64]", lp, top - lse64[:, None], float(tol_lp.min()),
                      "topk logprobs")
    assert (np.abs(lse - lse64) <= tol_lse).all(), f"{what}: lse error {e1}"
    assert (np.abs(lp - (top - lse64[:, None])) <= tol_lp).all(), f"{what}: logprobs error {e2}"
    # the definition: an fp32 subtraction of the returned lse
    assert np.array_equal(lp, np.take_along_axis(logits, want, -1) - lse[:, None]), f"{what}: logprobs != l - lse"


@pytest.fixture(scope="module", params=[("bf16", V1), ("bf16", V3), ("fp32", V1), ("fp32", V3)],
                ids=lambda p: f"{p[0]}-V{p[1]}")
def stage(request):
    st = make(*request.param)
    yield st
    st.close()


def test_tail_is_exact_against_its_own_logits(stage):
    rng = np.random.default_rng(11)
    for B in (1, 3):
        for S in (1, 7):
            for k in (1, 5, 16):
                x = rng.integers(0, stage.vocab, size=(B, S)).astype(np.int32)
                ids, lp, lse, lg = stage.forward_topk_host(x, B, S, k, slot=0, past_len=0, want_logits=True)
                check_tail(ids, lp, lse, lg, k, f"B{B} S{S} k{k} V{stage.vocab}")
                ids2, lp2, lse2 = stage.forward_topk_host(x, B, S, k, slot=0, past_len=0)  # no logits wanted
                assert np.array_equal(ids, ids2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
                assert np.array_equal(lse.view(np.uint32), lse2.view(np.uint32))
    n = ctypes.c_int32(7)
    assert lib().bs_read_head_screen(stage._h, 0, None, None, None, ctypes.byref(n)) == 0 and n.value == -1


def host_weights(dtype, vocab, edit):
    """The synthetic weights of make(dtype, vocab) with the embedding rows edited by `edit(emb [V][64])`."""
    st = make(dtype, vocab)
    w = st.read_weights()
    st.close()
    edit(w[:vocab * 64].reshape(vocab, 64))
    return w


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_equal_logits_rank_by_the_lower_index(dtype):
    """Duplicate embedding rows in the three slices give equal logits; the fed token's own row is the largest logit."""
    dup = [10, 2048 + 5, 4096 + 700]

    def edit(emb):
        emb[dup[1]] = emb[dup[0]]
        emb[dup[2]] = emb[dup[0]]
    st = make(dtype, V3, host_weights=host_weights(dtype, V3, edit))
    x = np.array([[7, dup[0]], [3, dup[2]]], np.int32)
    ids, lp, lse, lg = st.forward_topk_host(x, 2, 2, 5, want_logits=True)
    assert np.array_equal(lg[:, dup[0]].view(np.uint32), lg[:, dup[1]].view(np.uint32)), "the case has no teeth"
    assert np.array_equal(lg[:, dup[0]].view(np.uint32), lg[:, dup[2]].view(np.uint32)), "the case has no teeth"
    check_tail(ids, lp, lse, lg, 5, f"ties {dtype}")
    for b in range(2):
        got = [int(t) for t in ids[b] if int(t) in dup]
        assert got == dup, f"row {b}: {ids[b]}"
        at = [list(ids[b]).index(t) for t in dup]
        assert at == list(range(at[0], at[0] + 3)) and len(set(lp[b, at].tolist())) == 1
    st.close()


@pytest.mark.parametrize("dtype,vocab", [("bf16", V3), ("fp32", V1)])
def test_all_equal_logits(dtype, vocab):
    def edit(emb):
        emb[:] = emb[3]
    st = make(dtype, vocab, host_weights=host_weights(dtype, vocab, edit))
    ids, lp, lse, lg = st.forward_topk_host(np.array([[1, 2, 3]], np.int32), 1, 3, 16, want_logits=True)
    assert len(set(lg[0].view(np.uint32).tolist())) == 1, "the case has no teeth"
    assert ids[0].tolist() == list(range(16))
    want = float(lg[0, 0]) + np.log(float(vocab))
    tol = 2.0 ** -23 * (abs(float(lg[0, 0])) + abs(want) + 1) + (D + 4) * 2.0 ** -24
    record_error(f"all-equal {dtype} V{vocab} [lse vs l + log V]", lse, np.array([want]), tol, "topk lse")
    assert abs(float(lse[0]) - want) <= tol
    assert np.abs(lp[0].astype(np.float64) + np.log(float(vocab))).max() <= tol
    st.close()


def bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint32) for a in arrays]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def test_rows_and_runs_give_the_same_bits(stage):
    rng = np.random.default_rng(2)
    row = rng.integers(0, stage.vocab, size=7).astype(np.int32)
    x = np.stack([row, rng.integers(0, stage.vocab, size=7).astype(np.int32), row])
    a = stage.forward_topk_host(x, 3, 7, 16, slot=0, past_len=0, want_logits=True)
    b = stage.forward_topk_host(x, 3, 7, 16, slot=0, past_len=0, want_logits=True)
    assert same_bits(a, b), "two runs"
    assert np.array_equal(a[3][0].view(np.uint32), a[3][2].view(np.uint32)), "the head gives rows 0 and 2 the same logits"
    assert same_bits([v[0] for v in a], [v[2] for v in a]), "rows 0 and 2"
    assert not same_bits([v[0] for v in a], [v[1] for v in a])


@pytest.mark.parametrize("dtype,vocab", [("bf16", V3), ("fp32", V3), ("bf16", V1)])
def test_graph_replay_eager_launch_and_host_io_agree(dtype, vocab):
    """Three twins: graph replay on device buffers, eager launch on device buffers, host I/O; two S = 1 steps at
    different positions behind one prefill."""
    rng = np.random.default_rng(4)
    prompt = rng.integers(0, vocab, size=(3, 5)).astype(np.int32)
    steps = [rng.integers(0, vocab, size=(3, 1)).astype(np.int32) for _ in range(2)]
    k, res = 6, []
    for mode in ("graph", "eager", "host"):
        st = make(dtype, vocab)
        if mode == "eager":
            st.set_graphs(False)
        st.forward_host(prompt, 3, 5, slot=0, past_len=0)
        out = []
        if mode == "host":
            for i, x in enumerate(steps):
                out.append(st.forward_topk_host(x, 3, 1, k, slot=0, past_len=5 + i, want_logits=True))
        else:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                xin = torch.empty(3, 1, dtype=torch.int32, device=DEV)
                ids = torch.full((3, k), -1, dtype=torch.int32, device=DEV)
                lp = torch.full((3, k), np.nan, dtype=torch.float32, device=DEV)
                lse = torch.full((3,), np.nan, dtype=torch.float32, device=DEV)
                lg = torch.full((3, vocab), np.nan, dtype=torch.float32, device=DEV)
                for i, x in enumerate(steps):
                    xin.copy_(torch.from_numpy(x))
                    st.forward_topk(xin, ids, lp, 3, 1, k, slot=0, past_len=5 + i, lse=lse, logits=lg,
                                    stream=stream.cuda_stream)
                    stream.synchronize()
                    out.append(tuple(t.cpu().numpy() for t in (ids, lp, lse, lg)))
        res.append(out)
        st.close()
    for i in range(2):
        check_tail(*res[0][i], k, f"replay step {i} {dtype} V{vocab}")
        assert same_bits(res[0][i], res[1][i]), f"step {i}: graph replay vs eager launch"
        assert same_bits(res[0][i], res[2][i]), f"step {i}: device buffers vs host I/O"
    assert not same_bits(res[0][0], res[0][1])


def kv_bits(st, rows, n_layer=2, ctx=CTX):
    return np.stack([np.stack([st.read_kv(l, r, 0, ctx) for r in range(rows)]) for l in range(n_layer)]).view(np.uint32)


@pytest.mark.parametrize("kind", ["bf16", "fp32", "int8"])
def test_cache_and_next_step_equal_a_plain_forward_twin(kind):
    """A top-k pass appends what bs_forward appends, and its last kernel advances the device positions once: the
    next plain decode step (which skips the position upload when the host's positions match) equals the twin's."""
    rng = np.random.default_rng(6)
    prompt = rng.integers(0, V1, size=(3, 7)).astype(np.int32)
    t1, t2 = (rng.integers(0, V1, size=(3, 1)).astype(np.int32) for _ in range(2))
    dtype = "fp32" if kind == "fp32" else "bf16"
    a, b = make(dtype, V1, kv_int8=kind == "int8"), make(dtype, V1, kv_int8=kind == "int8")
    a.forward_topk_host(prompt, 3, 7, 4, slot=0, past_len=0)
    b.forward_host(prompt, 3, 7, slot=0, past_len=0)
    a.forward_topk_host(t1, 3, 1, 4, slot=0, past_len=7)
    b.forward_host(t1, 3, 1, slot=0, past_len=7)
    assert np.array_equal(kv_bits(a, 3), kv_bits(b, 3))
    _, la = a.forward_host(t2, 3, 1, slot=0, past_len=8, want_logits=True)
    _, lb = b.forward_host(t2, 3, 1, slot=0, past_len=8, want_logits=True)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert a.past[:3] == [9, 9, 9]
    # the same on device buffers under graph replay
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xin = torch.from_numpy(t2).to(DEV)
        ids = torch.empty(3, 4, dtype=torch.int32, device=DEV)
        lp = torch.empty(3, 4, dtype=torch.float32, device=DEV)
        tok = torch.empty(3, dtype=torch.int32, device=DEV)
        lga, lgb = (torch.empty(3, V1, dtype=torch.float32, device=DEV) for _ in range(2))
        a.forward_topk(xin, ids, lp, 3, 1, 4, slot=0, past_len=9, stream=stream.cuda_stream)
        a.forward(xin, tok, 3, 1, slot=0, past_len=10, logits=lga, stream=stream.cuda_stream)
        b.forward(xin, tok, 3, 1, slot=0, past_len=9, stream=stream.cuda_stream)
        b.forward(xin, tok, 3, 1, slot=0, past_len=10, logits=lgb, stream=stream.cuda_stream)
        stream.synchronize()
    assert np.array_equal(lga.cpu().numpy().view(np.uint32), lgb.cpu().numpy().view(np.uint32))
    a.close()
    b.close()


@pytest.mark.parametrize("flags", ["int8_weights", "mxfp4_weights"])
def test_quantised_weight_stages_work(flags):
    st = make("bf16", V1, hidden=256, **{flags: True})
    x = np.random.default_rng(9).integers(0, V1, size=(2, 3)).astype(np.int32)
    ids, lp, lse, lg = st.forward_topk_host(x, 2, 3, 8, want_logits=True)
    check_tail(ids, lp, lse, lg, 8, flags)
    st.close()


def call_topk(st, step, x, k, ids, lp, lse=None, logits=None):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return lib().bs_forward_topk(st._h, ctypes.byref(step) if step is not None else None, p(x), k, p(ids), p(lp),
                                 p(lse), p(logits), None)


def test_statuses_and_workspace():
    assert lib().bs_abi_version() == 5
    st = make("bf16", V1)
    x = np.array([[1, 2], [3, 4]], np.int32)
    ids, lp = np.empty((2, 16), np.int32), np.empty((2, 16), np.float32)
    lse, lg = np.empty(2, np.float32), np.empty((2, V1), np.float32)
    ok = Step(2, 2, 0, 0, BS_STEP_HOST_IO, None)
    before = st.info()
    # BS_ERR_INVALID
    assert lib().bs_forward_topk(None, ctypes.byref(ok), x.ctypes.data, 4, ids.ctypes.data, lp.ctypes.data, None, None, None) == -1
    assert call_topk(st, None, x, 4, ids, lp) == -1
    for k in (0, -1, 17):
        assert call_topk(st, ok, x, k, ids, lp) == -1, k
    assert call_topk(st, ok, x, 4, None, lp) == -1 and call_topk(st, ok, x, 4, ids, None) == -1
    assert call_topk(st, ok, None, 4, ids, lp) == -1
    for f in (BS_STEP_VERIFY, BS_STEP_VERIFY | BS_STEP_VERIFY_DRAW, BS_STEP_VERIFY_DRAW, BS_STEP_LOGITS):
        assert call_topk(st, Step(2, 2, 0, 0, BS_STEP_HOST_IO | f, None), x, 4, ids, lp, lse, lg) == -1, f
    for bad in (Step(0, 2, 0, 0, 1, None), Step(2, 0, 0, 0, 1, None), Step(2, 2, -1, 0, 1, None),
                Step(2, 2, MB - 1, 0, 1, None), Step(2, 2, 0, CTX - 1, 1, None), Step(2, 2, 0, -1, 1, None)):
        assert call_topk(st, bad, x, 4, ids, lp) == -1
    assert st.info() == before, "a refused call allocates nothing"
    # workspace: grows at the first call only
    assert call_topk(st, ok, x, 4, ids, lp) == 0
    first = st.info()
    assert first["workspace_bytes"] > before["workspace_bytes"]
    assert call_topk(st, ok, x, 16, ids, lp, lse, lg) == 0
    assert call_topk(st, Step(3, 1, 0, 2, BS_STEP_HOST_IO, None), np.array([[1], [2], [3]], np.int32), 1,
                     np.empty((3, 1), np.int32), np.empty((3, 1), np.float32)) == 0
    assert st.info() == first
    # BS_ERR_STATE: bs_set_sampling holds top_k > 1; a row of the call holds sampler state
    st.set_sampling(4, 1.0, 1)
    assert call_topk(st, ok, x, 4, ids, lp) == -4
    st.set_sampling(1)
    assert call_topk(st, ok, x, 4, ids, lp) == 0
    st.set_row_sampler(1, top_k=5, top_p=0.9, seed=3)
    assert call_topk(st, ok, x, 4, ids, lp) == -4
    assert call_topk(st, Step(1, 2, 0, 0, BS_STEP_HOST_IO, None), x, 4, ids, lp) == 0  # row 0 alone holds none
    st.clear_row_sampler()
    assert call_topk(st, ok, x, 4, ids, lp) == 0
    st.close()
    # BS_ERR_STATE: a classifier stage; stages without the whole lm_head
    cl = make("bf16", V1, n_labels=2)
    assert call_topk(cl, ok, x, 4, ids, lp) == -4
    cl.close()
    nl = Stage(64, 4, 2, V1, 0, 1, dtype="bf16", max_batch=MB, max_ctx=CTX, seed=5)
    assert call_topk(nl, ok, x, 4, ids, lp) == -4
    nl.close()


# ---- bs_copy_kv
CMB, CCTX = 6, 70
PAIRS = [(0, 2), (0, 3), (1, 5)]
COPY_KINDS = [("bf16", 256, 4), ("bf16", 320, 4), ("fp32", 64, 4), ("int8", 64, 4)]
ROWS = [np.random.default_rng(100 + r).integers(0, V1, size=(1, CCTX)).astype(np.int32) for r in range(CMB)]


def make_cache(kind, hidden, n_head):
    st = Stage(hidden, n_head, 2, V1, 0, 2, dtype="fp32" if kind == "fp32" else "bf16", max_batch=CMB, max_ctx=CCTX,
               seed=21, kv_int8=kind == "int8")
    for r in range(CMB):  # every row full, each with its own tokens: positions >= npos hold recognisable content
        st.forward_host(ROWS[r], 1, CCTX, slot=r, past_len=0)
    return st


@pytest.fixture(scope="module", params=COPY_KINDS, ids=lambda p: f"{p[0]}-hd{p[1] // p[2]}")
def caches(request):
    a, b = make_cache(*request.param), make_cache(*request.param)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("npos", [1, 37, 70])
def test_copy_is_exact_writes_nothing_else_and_equals_the_forks(caches, npos):
    a, b = caches
    for st in (a, b):  # earlier cases copied: put every row's own content back
        for r in {d for _, d in PAIRS}:
            st.forward_host(ROWS[r], 1, CCTX, slot=r, past_len=0)
    before = kv_bits(a, CMB, ctx=CCTX)
    assert np.array_equal(before, kv_bits(b, CMB, ctx=CCTX))
    assert all((before[:, r] != 0).any() for r in range(CMB))
    a.copy_kv(PAIRS, npos)
    after = kv_bits(a, CMB, ctx=CCTX)
    dsts = {d: s for s, d in PAIRS}
    for r in range(CMB):
        if r in dsts:
            s = dsts[r]
            assert not np.array_equal(before[:, r, :, :, :npos], before[:, s, :, :, :npos]), "the case has no teeth"
            assert np.array_equal(after[:, r, :, :, :npos], before[:, s, :, :, :npos]), f"row {r}: copied positions"
            assert np.array_equal(after[:, r, :, :, npos:], before[:, r, :, :, npos:]), f"row {r}: positions >= npos"
            assert npos == CCTX or (after[:, r, :, :, npos:] != 0).any()
            assert a.past[r] == npos
        else:
            assert np.array_equal(after[:, r], before[:, r]), f"row {r} was written"
    b.fork_kv(0, 2, npos=npos, count=2)
    b.fork_kv(1, 5, npos=npos, count=1)
    assert np.array_equal(after, kv_bits(b, CMB, ctx=CCTX)), "the pair list against the same pairs as forks"


def test_a_decode_step_after_the_copy_equals_the_source_rows(caches):
    a, b = caches
    npos = 37
    a.copy_kv(PAIRS, npos)
    tok = np.array([[123]], np.int32)
    for s, d in PAIRS:  # the copied row on one stage, the source row on its twin: the slot only offsets addresses
        _, la = a.forward_host(tok, 1, 1, slot=d, past_len=npos, want_logits=True)
        _, lb = b.forward_host(tok, 1, 1, slot=s, past_len=npos, want_logits=True)
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (s, d)
        b.forward_host(ROWS[s], 1, CCTX, slot=s, past_len=0)  # put the source row back


def test_copy_statuses(caches):
    a, _ = caches
    f, h = lib().bs_copy_kv, a._h

    def arr(v):
        return (ctypes.c_int32 * max(len(v), 1))(*v)

    def call(src, dst, npos, count=None):
        return f(h, arr(src), arr(dst), len(src) if count is None else count, npos, None)
    before, info = kv_bits(a, CMB, ctx=CCTX), a.info()
    assert f(None, arr([0]), arr([1]), 1, 1, None) == -1
    assert f(h, None, arr([1]), 1, 1, None) == -1 and f(h, arr([0]), None, 1, 1, None) == -1
    assert call([0], [1], 1, count=-1) == -1 and call([0] * 33, list(range(1, 34)), 1) == -1
    for src, dst in [([-1], [1]), ([CMB], [1]), ([0], [-1]), ([0], [CMB])]:
        assert call(src, dst, 1) == -1, (src, dst)
    assert call([0], [1], -1) == -1 and call([0], [1], CCTX + 1) == -1
    assert call([0, 1], [2, 2], 1) == -1, "a destination twice"
    assert call([0, 2], [2, 3], 1) == -1 and call([0], [0], 1) == -1, "a destination that is a source"
    assert call([], [], 5) == 0 and f(h, None, None, 0, 5, None) == 0 and call([0], [1], 0) == 0
    assert np.array_equal(kv_bits(a, CMB, ctx=CCTX), before), "no launch"
    assert call([0, 0, 0, 1], [2, 3, 4, 5], CCTX) == 0  # a source several times, the whole row
    assert a.info() == info
    nl = Stage(64, 4, 2, V1, 0, 0, dtype="bf16", max_batch=3, max_ctx=8, seed=1, is_first=False, is_last=True)
    assert lib().bs_copy_kv(nl._h, arr([0]), arr([1]), 1, 5, None) == 0
    assert lib().bs_copy_kv(nl._h, arr([0]), arr([0]), 1, 5, None) == -1
    nl.close()


# ---- end to end
@pytest.fixture(scope="module")
def checker():
    o = OracleStage(H, NH, L, V, 0, L, bf16=False, max_batch=1, max_ctx=32, seed=SEED)
    yield o
    o.close()


def fixture_stage(dtype, W, lb=0, le=L, **kw):
    return Stage(H, NH, L, V, lb, le, dtype=dtype, max_batch=W, max_ctx=32, seed=SEED, **kw)


@pytest.mark.parametrize("i", CASES, ids=case_id)
def test_device_search_equals_beam_ref_over_the_fp32_checker(checker, i):
    W, eos, lp, prompt, _, _ = case(i)
    st = fixture_stage("fp32", W)
    bs = BeamSearcher([st], W, length_penalty=lp, eos=eos, num_return=N_RETURN)
    seqs, scores, _ = bs.generate(prompt, N_NEW)
    rs, rsc = ref_result(checker, i)
    err = record_error(f"beam scores {case_id(i)} [fp32 device vs beam_ref over the checker]", scores, rsc,
                       1e-3 * N_NEW, "beam score")
    assert seqs == rs
    assert err <= 1e-3 * N_NEW
    if W == 4:  # the host-I/O route and a first + last chain give the single stage's hypotheses
        h2 = fixture_stage("fp32", W)
        assert BeamSearcher([h2], W, length_penalty=lp, eos=eos, num_return=N_RETURN, host_io=True).generate(
            prompt, N_NEW)[0] == seqs
        h2.close()
        first, last = fixture_stage("fp32", W, 0, 1), fixture_stage("fp32", W, 1, 2)
        chain = BeamSearcher([first, last], W, length_penalty=lp, eos=eos, num_return=N_RETURN)
        assert chain.generate(prompt, N_NEW)[0] == seqs
        assert chain.kv_copies == bs.kv_copies
        first.close()
        last.close()
    st.close()


def test_bf16_token_logprobs_against_the_scoring_pass():
    """Each returned hypothesis' per-token log-probs against bs_forward_score's target log-probs of that sequence
    (test_gpu_score.py's bound for two bf16 routes: 2 * BF16_TOL)."""
    i = next(i for i in CASES if int(G["num_beams"][i]) == 4 and int(G["eos"][i]) >= 0 and G["length_penalty"][i] == 0.6)
    W, eos, lp, prompt, _, _ = case(i)
    st = fixture_stage("bf16", W)
    seqs, scores, tlps = BeamSearcher([st], W, length_penalty=lp, eos=eos, num_return=W).generate(prompt, N_NEW)
    sc = fixture_stage("bf16", 1)
    for s, score, t in zip(seqs, scores, tlps):
        full = np.array(prompt + s, np.int32)
        _, res = sc.score_host(full[:-1], full[1:], 1, len(full) - 1, slot=0, past_len=0)
        want = res[0, len(prompt) - 1:, 0]
        err = record_error("beam token logprobs [vs bs_forward_score]", t, want, 2 * BF16_TOL,
                           "beam logprob bf16")
        assert err <= 2 * BF16_TOL
        assert abs(sum(t) / len(s) ** lp - score) <= 1e-9
    st.close()
    sc.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_beam_is_greedy_decoding(dtype):
    prompt = case(0)[3]
    st, tw = fixture_stage(dtype, 1), fixture_stage(dtype, 1)
    seqs, _, _ = BeamSearcher([st], 1).generate(prompt, N_NEW)
    tok = tw.forward_host(np.array(prompt, np.int32), 1, len(prompt), slot=0, past_len=0)
    want = [int(tok[0])]
    for n in range(N_NEW - 1):
        tok = tw.forward_host(tok, 1, 1, slot=0, past_len=len(prompt) + n)
        want.append(int(tok[0]))
    assert seqs == [want]
    st.close()
    tw.close()


def test_serve_num_beams_returns_the_searchers_sequences():
    """serve --num-beams 4 on bloom-560m's shape at reduced depth."""
    from distributed_inference_demo_amd.serve import RunConfig, run_rank, synthetic_prompts
    model = BloomDims("bloom-560m-2l", 1024, 2, 16)
    cfg = RunConfig(model=model, num_sample=2, max_length=6, prompt_len=5, num_beams=4, length_penalty=0.8, seed=3)
    prompts = synthetic_prompts(cfg, model.vocab)
    res = run_rank(cfg, 0, 1, DEV, prompts=prompts)
    st = Stage(1024, 16, 2, model.vocab, 0, 2, dtype="bf16", max_batch=4, max_ctx=5 + 6 + 1, max_tokens=5, seed=3)
    bs = BeamSearcher([st], 4, length_penalty=0.8)
    want = [bs.generate(p, 6) for p in prompts]
    assert res["samples"] == [w[0][0] for w in want]
    assert res["scores"] == [w[1][0] for w in want]
    assert res["num_beams"] == 4 and res["length_penalty"] == 0.8 and res["kv_copies"] == bs.kv_copies > 0
    assert all(len(s) == 6 for s in res["samples"])
    st.close()
