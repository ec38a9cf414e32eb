"""GPU tests of the teacher-forced scoring pass (bs_forward_score, csrc/head_score.hip).

A. the fused head + log-softmax kernel against a float64 restatement on head-only stages;
B. dynamic range (large logits, rising logits) and exact ties;
C. a whole first + last stage against the CPU checker run teacher-forced, chunked scoring, the KV cache and the
   decode step that follows, on bf16, int8-KV and int8-weight stages;
D. the C-ABI contract: statuses, NULL handling, host I/O, run-to-run bit identity, workspace growth, ABI version.

Bounds of A and B, both computed here: bound_l = K * 2^-23 * max sum_k |xn_k w_k| (fp32 accumulation of exact bf16
products) and floor32 = the largest |lse error| of a float32 numpy restatement (16 sequential running sums, then
combined, on the float64 logits rounded to fp32) against float64: the fp32 noise floor measured by the reference
itself.  Every score lies within 2 bound_l + 8 floor32 of the reference (8: the device's other summation order and
a few ulp per expf / logf).  top_ids equal the reference argmax except where the reference top-2 gap is below
2 bound_l (either of the two is accepted there; at most 5 % of a case's positions may be such).
Each check appends its achieved error and bound to the file $BS_SCORE_LOG names (JSON lines; nothing when unset):
profiles/score_head_errors.txt is such a log.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.stage import BloomStageError, Stage, Step
from oracle import gen_np
from oracle.oracle import OracleStage

from test_gpu_parity import BF16_TOL, assert_ids_match

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _record(case, what, err, bound, **extra):
    path = os.environ.get("BS_SCORE_LOG")
    if not path:
        return
    rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "case": case, "check": what,
           "max_abs": float(err), "bound": float(bound), **extra}
    try:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _head_stage(h, V, M, ctx, seed=7, host_weights=None):
    """Layer-free last stage: fp32 hidden in, ln_f + the tied head."""
    return Stage(h, 16 if h >= 512 else 4, 1, V, 1, 1, dtype="bf16", max_batch=M, max_ctx=ctx, max_tokens=M,
                 seed=seed, is_first=False, is_last=True, host_weights=host_weights)


def _score_dev(st, x, targets, B, S, past_len=0, want_top=True, want_scores=True):
    """Stage.score on device buffers; returns numpy (top_ids, scores)."""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    td = None if targets is None else torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32)).to(DEV)
    top = torch.full((B, S), -7, dtype=torch.int32, device=DEV) if want_top else None
    sc = torch.full((B, S, 3), np.nan, dtype=torch.float32, device=DEV) if want_scores else None
    torch.cuda.synchronize()
    st.score(xd, td, top, sc, B, S, past_len=past_len)
    torch.cuda.synchronize()
    return (None if top is None else top.cpu().numpy(), None if sc is None else sc.cpu().numpy())


def _floor32(L, lse64):
    """Largest |lse error| of a float32 restatement: 16 sequential running sums, then combined."""
    L32 = L.astype(np.float32)
    m = L32.max(axis=1)
    e = np.exp(L32 - m[:, None]).astype(np.float32)
    lanes = np.cumsum(e.reshape(e.shape[0], -1, 16), axis=1, dtype=np.float32)[:, -1, :]
    s = np.cumsum(lanes, axis=1, dtype=np.float32)[:, -1]
    lse32 = (m + np.log(s).astype(np.float32)).astype(np.float32)
    return float(np.abs(lse32.astype(np.float64) - lse64).max())


def _reference(st, hidden, M, V, h, chunk=16384):
    """float64 logits of bf16(ln_f(hidden rows)) (Stage.head_norm) against the head rows (read_weights)."""
    import torch
    hd = torch.from_numpy(np.ascontiguousarray(hidden.reshape(M, 1, h))).to(DEV)
    xn = torch.empty((M, h), dtype=torch.bfloat16, device=DEV)
    st.head_norm(hd, M, 1, xn)
    torch.cuda.synchronize()
    x32 = xn.float().cpu().numpy()
    x64 = x32.astype(np.float64)
    L = np.empty((M, V), np.float64)
    amax = 0.0
    for v0 in range(0, V, chunk):
        n = min(chunk, V - v0)
        W = st.read_weights(v0 * h, n * h).reshape(n, h)
        L[:, v0:v0 + n] = x64 @ W.astype(np.float64).T
        amax = max(amax, float((np.abs(x32) @ np.abs(W).T).max()))
    mx = L.max(axis=1)
    lse = mx + np.log(np.exp(L - mx[:, None]).sum(axis=1))
    bound_l = h * 2.0 ** -23 * amax
    return {"L": L, "lse": lse, "bound_l": bound_l, "floor32": _floor32(L, lse)}


def _check(case, ref, targets, top, sc, M, V, built_ties=False):
    """built_ties: the case ties logits on purpose (every gap is 0), and asserts its own, exact, top_ids."""
    L, lse = ref["L"], ref["lse"]
    bound = 2 * ref["bound_l"] + 8 * ref["floor32"]
    rows = np.arange(M)
    rtop = L.argmax(axis=1)
    L2 = L.copy()
    L2[rows, rtop] = -np.inf
    rsec = L2.argmax(axis=1)
    gap = L[rows, rtop] - L[rows, rsec]
    exempt = gap < 2 * ref["bound_l"]
    tg = targets.reshape(-1)
    has = (tg >= 0) & (tg < V)
    want_t = np.where(has, L[rows, np.where(has, tg, 0)] - lse, 0.0)
    sc = sc.reshape(M, 3).astype(np.float64)
    errs = {"target": np.abs(sc[:, 0] - want_t).max(), "top": np.abs(sc[:, 1] - (L[rows, rtop] - lse)).max(),
            "lse": np.abs(sc[:, 2] - lse).max()}
    for k, e in errs.items():
        print(f"{case}: {k} max-abs {e:.3e}, bound {bound:.3e} (bound_l {ref['bound_l']:.3e}, floor32 "
              f"{ref['floor32']:.3e})")
        _record(case, k, e, bound, bound_l=ref["bound_l"], floor32=ref["floor32"])
    print(f"{case}: {int(exempt.sum())} of {M} positions exempt from the exact argmax")
    _record(case, "exempt", float(exempt.mean()), 0.05)
    top = top.reshape(-1)
    assert np.all(sc[~has, 0] == 0.0), f"{case}: a position without a target did not score 0.0"
    for k, e in errs.items():
        assert e <= bound, f"{case}: {k} max-abs {e} > {bound}"
    if built_ties:
        return
    assert exempt.mean() <= 0.05, f"{case}: {exempt.sum()} of {M} positions have a top-2 gap below 2 bound_l"
    ok = (top == rtop) | (exempt & (top == rsec))
    assert ok.all(), f"{case}: top_ids {top[~ok][:5]} != {rtop[~ok][:5]} at {np.flatnonzero(~ok)[:5]}, gaps {gap[~ok][:5]}"


def _targets(rng, B, S, V):
    t = rng.integers(0, V, (B, S)).astype(np.int32)
    t[rng.random((B, S)) < 0.2] = -1
    t[-1, -1] = -1
    return t


# (h, V, B, S): one K step under one tile; a ragged row tile; three K steps, 8 tiles + 48 rows, positions across a
# 128-row boundary; several vocabulary runs per block; the real vocabulary; and a K that ends in half a 64-deep step
SHAPES = [(64, 48, 1, 1), (64, 48, 3, 11), (192, 1072, 2, 65), (128, 4096, 7, 10), (1024, 250880, 2, 20),
          (96, 1072, 2, 9)]


@pytest.mark.parametrize("h,V,B,S", SHAPES)
def test_kernel_matches_float64_restatement(h, V, B, S):
    M = B * S
    st = _head_stage(h, V, M, S)
    rng = np.random.default_rng(1)
    hidden = (rng.standard_normal((B, S, h)) * 2).astype(np.float32)
    targets = _targets(rng, B, S, V)
    if M == 1:
        targets[:] = V - 1  # the single position scores a target (the last vocabulary row)
    ref = _reference(st, hidden, M, V, h)
    top, sc = _score_dev(st, hidden, targets, B, S)
    _check(f"A h={h} V={V} B={B} S={S}", ref, targets, top, sc, M, V)
    if M == 1:  # and without one
        top2, sc2 = _score_dev(st, hidden, np.full((1, 1), -1, np.int32), 1, 1)
        assert sc2[0, 0, 0] == 0.0 and np.array_equal(top2, top) and np.array_equal(sc2[..., 1:], sc[..., 1:])


# ---- B: dynamic range and ties (host weights, h 192, V 1072, M 130)
BH, BV_, BB, BS_ = 192, 1072, 2, 65


@functools.lru_cache(maxsize=None)
def _b_parts():
    emb = gen_np.tensor(7, -1, gen_np.GT_WEMB, (BV_, BH))
    g = gen_np.tensor(7, -1, gen_np.GT_LNF_G, (BH,))
    b = gen_np.tensor(7, -1, gen_np.GT_LNF_B, (BH,))
    hidden = (np.random.default_rng(1).standard_normal((BB, BS_, BH)) * 2).astype(np.float32)
    return emb, g, b, hidden


def _b_run(case, head, g, b, hidden, built_ties=False):
    M = BB * BS_
    st = _head_stage(BH, BV_, M, BS_, host_weights=np.concatenate([head.reshape(-1), g, b]).astype(np.float32))
    targets = _targets(np.random.default_rng(2), BB, BS_, BV_)
    ref = _reference(st, hidden, M, BV_, BH)
    top, sc = _score_dev(st, hidden, targets, BB, BS_)
    _check(case, ref, targets, top, sc, M, BV_, built_ties)
    return ref, top.reshape(-1), sc.reshape(M, 3)


def test_large_and_rising_logits():
    """Head x 32: logits reach about +-40, exp underflows and the running max is replaced many times; three positions
    see logits that rise with the vocabulary index (every tile brings a new maximum)."""
    emb, g, b, hidden = _b_parts()
    u = np.where(np.arange(BH) % 2 == 0, 1.0, -1.0).astype(np.float32)
    head = 32.0 * emb + (60.0 * np.arange(BV_, dtype=np.float32) / BV_ / BH)[:, None] * u[None, :]
    hidden = hidden.copy().reshape(-1, BH)
    for p in (3, 64, 129):
        hidden[p] = u
    ref, top, sc = _b_run("B(i) large and rising logits", head, g, b, hidden.reshape(BB, BS_, BH))
    assert np.abs(ref["L"]).max() > 30.0
    assert all(ref["L"][p].argmax() > BV_ * 3 // 4 for p in (3, 64, 129))


def test_all_equal_logits():
    """Every head row the same vector: every top_id is 0 and lse = l + log 1072."""
    emb, g, _, hidden = _b_parts()
    b = np.full(BH, 0.5, np.float32)
    head = np.repeat(emb[:1], BV_, axis=0)
    ref, top, sc = _b_run("B(ii) all-equal logits", head, g, b, hidden, built_ties=True)
    assert np.all(top == 0)
    bound = 2 * ref["bound_l"] + 8 * ref["floor32"]
    assert np.abs(sc[:, 2] - (ref["L"][:, 0] + np.log(BV_))).max() <= bound
    assert np.abs(sc[:, 1] + np.log(BV_)).max() <= bound


def test_ties_resolve_to_the_lowest_index():
    """Rows 5 and 1071 hold one winning vector (the first tile and the last, another split, another lane half):
    every top_id is 5."""
    emb, g, _, hidden = _b_parts()
    b = np.full(BH, 0.5, np.float32)
    head = np.repeat(emb[:1], BV_, axis=0)
    head[5] = head[1071] = 0.05
    ref, top, sc = _b_run("B(iii) ties", head, g, b, hidden, built_ties=True)
    assert np.all(ref["L"].argmax(axis=1) == 5) and np.all(ref["L"][:, 5] == ref["L"][:, 1071])
    assert np.all(top == 5), top


# ---- C: whole stage against the checker
CH, CNH, CL, CV, CB_, CS_ = 64, 4, 2, 512, 2, 12


def _c_stage(variant, **kw):
    return Stage(CH, CNH, CL, CV, 0, CL, dtype="bf16", max_batch=CB_, max_ctx=CS_ + 4, seed=11,
                 kv_int8=variant == "kv_int8", int8_weights=variant == "w_int8", **kw)


@functools.lru_cache(maxsize=None)
def _c_reference(int8):
    """The checker run teacher-forced, one position at a time with logits -> float64 log-probs."""
    o = OracleStage(CH, CNH, CL, CV, 0, CL, bf16=True, max_batch=CB_, max_ctx=CS_ + 4, seed=11, int8=int8)
    ids = gen_np.prompt_ids(5, CB_, CS_, CV).astype(np.int32)
    lg = np.empty((CB_, CS_, CV), np.float64)
    for t in range(CS_):
        _, l = o.forward(ids[:, t:t + 1], CB_, 1, past_len=t, want_logits=True)
        lg[:, t] = l
    mx = lg.max(axis=-1, keepdims=True)
    lse = (mx + np.log(np.exp(lg - mx).sum(axis=-1, keepdims=True)))[..., 0]
    targets = np.full((CB_, CS_), -1, np.int32)
    targets[:, :-1] = ids[:, 1:]
    return ids, targets, lg, lse


def _c_check(what, top, sc, ids, targets, lg, lse):
    tol = 2 * BF16_TOL  # a log-prob is a difference of two quantities each held to the logit tolerance
    M = CB_ * CS_
    flat, rows = lg.reshape(M, CV), np.arange(M)
    tg = targets.reshape(-1)
    want_t = np.where(tg >= 0, flat[rows, np.maximum(tg, 0)] - lse.reshape(-1), 0.0)
    got = sc.reshape(M, 3).astype(np.float64)
    errs = (np.abs(got[:, 0] - want_t).max(), np.abs(got[:, 1] - (flat.max(axis=1) - lse.reshape(-1))).max(),
            np.abs(got[:, 2] - lse.reshape(-1)).max())
    print(f"{what}: max-abs target {errs[0]:.3e} top {errs[1]:.3e} lse {errs[2]:.3e}, tolerance {tol}")
    for k, e in zip(("target", "top", "lse"), errs):
        _record("C " + what, k, e, tol)
    assert max(errs) <= tol, f"{what}: {errs} > {tol}"
    assert_ids_match(top.reshape(-1), flat.argmax(axis=1), flat, what)


@pytest.mark.parametrize("variant", ["bf16", "kv_int8", "w_int8"])
def test_stage_scores_match_teacher_forced_checker(variant):
    """One scoring call over the prompt against the checker, then: the KV cache equals a plain prefill's bit for bit
    and the greedy decode step after it returns the same token (device buffers: the scoring pass's last kernel left
    the rows' positions on the device)."""
    import torch
    ids, targets, lg, lse = _c_reference(variant == "w_int8")
    g, p = _c_stage(variant), _c_stage(variant)
    top, sc = _score_dev(g, ids, targets, CB_, CS_)
    _c_check(f"{variant} single call", top, sc, ids, targets, lg, lse)
    assert g.read_head_screen() is None  # a scoring pass never takes the screened tail
    idd = torch.from_numpy(ids).to(DEV)
    tok_p = torch.empty(CB_, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p.forward(idd, tok_p, CB_, CS_, past_len=0)
    torch.cuda.synchronize()
    assert g.past == p.past == [CS_] * CB_
    for layer in range(CL):
        for row in range(CB_):
            a, b = g.read_kv(layer, row, 0, CS_), p.read_kv(layer, row, 0, CS_)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"KV layer {layer} row {row}"
    nxt = torch.from_numpy(gen_np.prompt_ids(6, CB_, 1, CV).astype(np.int32)).to(DEV)
    tok_g = torch.empty(CB_, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g.forward(nxt, tok_g, CB_, 1)
    p.forward(nxt, tok_p, CB_, 1)
    torch.cuda.synchronize()
    assert np.array_equal(tok_g.cpu().numpy(), tok_p.cpu().numpy())


def test_chunked_scoring_equals_single_call():
    """S = 12 scored as 5 + 7 with past_len (bf16 KV: the second chunk attends the first through the cache)."""
    ids, targets, lg, lse = _c_reference(False)
    g = _c_stage("bf16")
    t1, s1 = _score_dev(g, ids[:, :5], targets[:, :5], CB_, 5, past_len=0)
    t2, s2 = _score_dev(g, ids[:, 5:], targets[:, 5:], CB_, 7, past_len=None)  # the host mirror: 5
    assert g.past == [CS_] * CB_
    _c_check("chunked 5 + 7", np.concatenate([t1, t2], axis=1), np.concatenate([s1, s2], axis=1), ids, targets, lg, lse)
    one_t, one_s = _score_dev(_c_stage("bf16"), ids, targets, CB_, CS_)
    d = np.abs(np.concatenate([s1, s2], axis=1).astype(np.float64) - one_s).max()
    print(f"chunked vs single call: max-abs {d:.3e}")
    assert d <= 2 * BF16_TOL


# ---- D: contract
def _raw_score(st, step, x, targets, top, scores):
    return bs.lib().bs_forward_score(st._h, ctypes.byref(step), bs._ptr(x), bs._ptr(targets), bs._ptr(top),
                                     bs._ptr(scores), None)


def test_abi_version_is_5():
    assert bs.lib().bs_abi_version() == 5


def test_statuses():
    x = np.zeros((1, 2, 64), np.float32)
    ids = np.zeros((1, 2), np.int32)
    top, sc = np.empty((1, 2), np.int32), np.empty((1, 2, 3), np.float32)
    host = Step(1, 2, 0, 0, bs.BS_STEP_HOST_IO, None)
    cls = Stage(64, 4, 2, 512, 1, 2, dtype="bf16", max_ctx=8, seed=1, n_labels=2)
    mid = Stage(64, 4, 2, 512, 0, 1, dtype="bf16", max_ctx=8, seed=1)
    slc = Stage(64, 4, 3, 512, 1, 2, dtype="bf16", max_ctx=8, seed=1, head_slice=(0, 256))
    f32 = Stage(64, 4, 2, 512, 0, 2, dtype="fp32", max_ctx=8, seed=1)
    assert _raw_score(cls, host, x, None, top, sc) == -4   # BS_ERR_STATE
    assert _raw_score(mid, host, ids, None, top, sc) == -4
    assert _raw_score(slc, host, x, None, top, sc) == -4
    assert _raw_score(f32, host, ids, None, top, sc) == -5  # BS_ERR_UNSUPPORTED
    ok = Stage(64, 4, 2, 512, 0, 2, dtype="bf16", max_ctx=8, max_tokens=4, seed=1)
    assert _raw_score(ok, Step(1, 2, 0, 0, bs.BS_STEP_HOST_IO | bs.BS_STEP_LOGITS, None), ids, None, top, sc) == -1
    assert _raw_score(ok, host, ids, None, None, None) == -1       # both outputs NULL
    assert _raw_score(ok, host, None, None, top, sc) == -1
    assert _raw_score(ok, Step(1, 5, 0, 0, bs.BS_STEP_HOST_IO, None), np.zeros((1, 5), np.int32), None,
                      np.empty((1, 5), np.int32), None) == -1      # batch * seq > max_tokens
    assert _raw_score(ok, Step(1, 2, 0, 7, bs.BS_STEP_HOST_IO, None), ids, None, top, sc) == -1  # past max_ctx
    with pytest.raises(BloomStageError, match="error -4"):
        cls.score_host(x, None, 1, 2)
    assert _raw_score(ok, host, ids, None, top, sc) == 0


def test_null_handling_host_io_and_bit_identity():
    h, nh, L, V, B, S = 64, 4, 2, 512, 2, 9
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_batch=B, max_ctx=S, seed=3)
    ids = gen_np.prompt_ids(8, B, S, V).astype(np.int32)
    tg = np.full((B, S), -1, np.int32)
    tg[:, :-1] = ids[:, 1:]
    tg[0, 2] = V  # outside [0, vocab): none
    top, sc = _score_dev(st, ids, tg, B, S)
    assert np.all((top >= 0) & (top < V)) and np.all(np.isfinite(sc))
    assert np.all(sc[:, -1, 0] == 0.0) and sc[0, 2, 0] == 0.0 and np.all(sc[1, :-1, 0] < 0.0)
    has = (tg >= 0) & (tg < V)
    assert np.all(sc[..., 1] <= 0.0) and np.all(sc[has, 0] <= sc[has, 1])
    top_b, sc_b = _score_dev(st, ids, tg, B, S)  # the same call again: bit-identical
    assert np.array_equal(top, top_b) and np.array_equal(sc.view(np.uint32), sc_b.view(np.uint32))
    top_h, sc_h = st.score_host(ids, tg, B, S, past_len=0)  # host I/O
    assert np.array_equal(top, top_h) and np.array_equal(sc.view(np.uint32), sc_h.view(np.uint32))
    top_n, sc_n = _score_dev(st, ids, None, B, S)  # NULL targets: none anywhere
    assert np.array_equal(top, top_n) and np.all(sc_n[..., 0] == 0.0)
    assert np.array_equal(sc[..., 1:].view(np.uint32), sc_n[..., 1:].view(np.uint32))
    top_o, none = _score_dev(st, ids, tg, B, S, want_scores=False)
    assert none is None and np.array_equal(top, top_o)
    none, sc_o = _score_dev(st, ids, tg, B, S, want_top=False)
    assert none is None and np.array_equal(sc.view(np.uint32), sc_o.view(np.uint32))


def test_workspace_grows_on_the_first_scoring_call_only():
    h, nh, L, V, B, S = 64, 4, 1, 2048, 2, 40
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_batch=B, max_ctx=S, max_tokens=B * S, seed=3)
    ids = gen_np.prompt_ids(9, B, S, V).astype(np.int32)
    before = st.info()["workspace_bytes"]
    st.forward_host(ids, B, S, past_len=0)
    assert st.info()["workspace_bytes"] == before
    st.score_host(ids, None, B, S, past_len=0)
    after = st.info()["workspace_bytes"]
    assert before < after < before + B * S * V, (before, after)
    st.score_host(ids, None, B, S, past_len=0)
    assert st.info()["workspace_bytes"] == after


def test_serve_score_task_on_gpu():
    """serve.run_rank with score=True on cuda:0 with the product stage (pipeline.score through StageExecutor on a
    torch stream): ragged prompts, 2 rows a pass, padded at the tail; every sample's log-likelihood against the checker
    scoring that sample alone, teacher-forced."""
    import torch
    from distributed_inference_demo_amd.config import BloomDims
    from distributed_inference_demo_amd.serve import RunConfig, run_rank
    m = BloomDims("tiny-score", 256, 3, 4, 1024)
    rng = np.random.default_rng(17)
    prompts = [rng.integers(0, m.vocab, size=n).tolist() for n in (9, 3, 17, 2, 9)]
    cfg = RunConfig(model=m, num_sample=len(prompts), core_pool_size=2, dtype="bf16", seed=23, score=True)
    res = run_rank(cfg, 0, 1, torch.device("cuda", 0), prompts=prompts)
    assert res["task"] == "score" and res["passes"] == 3 and len(res["samples"]) == len(prompts)
    for i, p in enumerate(prompts):
        n = len(p)
        o = OracleStage(256, 4, 3, 1024, 0, 3, bf16=True, max_ctx=n + 1, seed=23)
        ll = 0.0
        for t in range(n - 1):
            _, lg = o.forward(np.array(p[t:t + 1], np.int32).reshape(1, 1), 1, 1, past_len=t, want_logits=True)
            lg = lg[0].astype(np.float64)
            ll += lg[p[t + 1]] - (lg.max() + np.log(np.exp(lg - lg.max()).sum()))
        got = res["samples"][i]
        print(f"sample {i} ({n} tokens): loglik {got['loglik']:.6f}, checker {ll:.6f}")
        assert got["tokens"] == n - 1
        assert abs(got["loglik"] - ll) <= 2 * BF16_TOL * (n - 1), (i, got, ll)
        assert got["perplexity"] == pytest.approx(np.exp(-got["loglik"] / (n - 1)), rel=1e-6)
