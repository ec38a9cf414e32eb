"""GPU tests of the verify pass (bs_step.flags & BS_STEP_VERIFY: csrc/attn_verify.hip, the all-positions greedy tail,
graph replay of short passes).

A synthetic model echoes its last input token (the tied head's self-dot dominates), so a free-running generation has
identical K / V at every position and cannot see a mask or rollback error: the primitive is driven with random ids and
judged on logits.

A. the short-query attention element by element: method and bound of tests/test_gpu_attention_exact.py (0.5 ulp_bf16
   + 2^-14 max|V| against a float64 reference built from read_kv), with the flag set;
B. whole stages against the CPU checker, teacher-forced on random ids: plain prefill of 7 tokens, a flagged S = 8 pass
   whose last six inputs are junk, a flagged S = 2 pass at past = 9 with the true tokens (the rollback), an unflagged
   S = 1 step at past = 11; logits of every valid position within check_logits' tolerance, ids == first-index argmax
   of the returned logits exactly, the junk without any effect (bit for bit);
C. invariants: graph replay == eager bit for bit, run-to-run bit identity, K / V equal to the unflagged pass's,
   status codes, ABI version, workspace growth.
"""
import ctypes
import functools

import numpy as np
import pytest

from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.stage import BloomStageError, Stage, Step
from oracle import gen_np
from oracle.oracle import OracleStage

from test_gpu_attention_exact import AttnStage, bf16_ulp
from test_gpu_parity import assert_ids_match, check_close, check_logits, record_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fwd_dev(st, x, B, S, pasts, verify, want_logits=True, slot=0):
    """Stage.forward on device buffers (the graph-replayed path for S = 1 and flagged passes); numpy results."""
    import torch
    x = np.array(x, dtype=np.int32 if st.is_first else np.float32, order="C")  # a writable copy for torch
    xd = torch.from_numpy(x).to(DEV)
    rows = (B, S) if verify else (B,)
    if st.is_last:
        out = torch.full(rows, -7, dtype=torch.int32, device=DEV)
        lg = torch.full(rows + (st.vocab,), np.nan, dtype=torch.float32, device=DEV) if want_logits else None
    else:
        out = torch.full((B, S, st.hidden), np.nan, dtype=torch.float32, device=DEV)
        lg = None
    torch.cuda.synchronize()
    st.forward(xd, out, B, S, slot=slot, past_len=pasts, logits=lg, verify=verify)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if lg is None else lg.cpu().numpy())


# ---- A: attention, element by element
def _check_verify_attention(a, x, B, S, slot, pasts, what):
    """AttnStage.run_and_check with the flag set: every context element of a flagged pass."""
    out = a.st.forward_host(x, B, S, slot=slot, past_len=list(pasts), verify=True)
    ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(B, S, a.nh, a.hd)
    worst = 0.0
    for b in range(B):
        n = pasts[b] + S
        kv = a.st.read_kv(0, slot + b, 0, n).astype(np.float64)
        K, V = kv[0], kv[1]
        assert np.array_equal(V, np.roll(K, -1, axis=0)), f"{what}: V_j != K_(j+1) in row {b}"
        for j in range(a.nh):
            q = K[(j - 1) % a.nh, pasts[b]:n]
            s = a.inv_norm * (q @ K[j].T) + a.slopes[j] * np.arange(n)[None, :]
            s[np.arange(n)[None, :] > (pasts[b] + np.arange(S))[:, None]] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            ref = (p @ V[j]) / p.sum(axis=1, keepdims=True)
            got = ctx[b, :, j, :]
            slack = 2.0 ** -14 * np.abs(V[j]).max() + 1e-7
            over = (np.abs(got - ref) - 0.5 * bf16_ulp(ref)) / slack
            worst = max(worst, float(over.max()))
            bad = np.argwhere(over > 1.0)
            assert bad.size == 0, (f"{what}: row {b} head {j} query {bad[0][0]} dim {bad[0][1]}: "
                                   f"{got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    record_error(what + " [verify attention exact: worst (error - half ulp) / slack]", np.array([worst]),
                 np.array([0.0]), 1.0, "attention exact")
    print(f"{what}: worst (error - half ulp) / slack {worst:.3f}")
    return worst


def _x(rng, B, S, h):
    return (0.01 * rng.standard_normal((B, S, h))).astype(np.float32)


@pytest.mark.parametrize("nh,hd,B,slot,S,pasts,max_ctx", [
    (4, 64, 1, 0, 2, (0,), 64),              # the mask alone, one split
    (4, 64, 1, 0, 8, (61,), 128),            # the new positions straddle a 64-position chunk
    (4, 96, 3, 1, 5, (0, 130, 449), 512),    # two splits merged by ticket; row 0's second split holds no chunk
    (16, 128, 1, 0, 4, (1000,), 1024),       # four splits of 16 chunks
    (4, 80, 1, 0, 3, (70,), 128),            # head_dim 80: the lanes past it are masked
])
def test_verify_attention_exact(nh, hd, B, slot, S, pasts, max_ctx):
    h = nh * hd
    a = AttnStage(h, nh, slot + B, max_ctx, max(max(pasts), 32))
    rng = np.random.default_rng(100 + hd + S)
    for r, n in enumerate(pasts):
        if n:
            a.run_and_check(_x(rng, 1, n, h), 1, n, slot + r, [0], f"prompt {n}")
    _check_verify_attention(a, _x(rng, B, S, h), B, S, slot, list(pasts), f"verify {nh}x{hd} B={B} S={S} past={pasts}")


# ---- B: whole stages against the checker, teacher-forced on random ids
NTOK, NROW = 16, 2
SMALL, WIDE = (64, 4, 2, 512), (256, 4, 3, 1024)
MSEED = 3


@functools.lru_cache(maxsize=None)
def _reference(cfg, dtype, int8=False):
    """The checker run teacher-forced one position at a time: ids [2][16], logits [2][16][V]."""
    h, nh, L, V = cfg
    o = OracleStage(h, nh, L, V, 0, L, bf16=dtype == "bf16", max_batch=NROW, max_ctx=NTOK, seed=MSEED, int8=int8)
    ids = gen_np.prompt_ids(5, NROW, NTOK, V).astype(np.int32)
    lg = np.empty((NROW, NTOK, V), np.float32)
    for t in range(NTOK):
        _, l = o.forward(ids[:, t:t + 1], NROW, 1, past_len=t, want_logits=True)
        lg[:, t] = l
    o.close()
    lg.setflags(write=False)
    ids.setflags(write=False)
    return ids, lg


def _stage(cfg, dtype, **kw):
    h, nh, L, V = cfg
    return Stage(h, nh, L, V, 0, L, dtype=dtype, max_batch=NROW, max_ctx=NTOK + 8, max_tokens=32, seed=MSEED, **kw)


def _junk(seed, n, V):
    return np.random.default_rng(seed).integers(0, V, size=n).astype(np.int32)


def _check_ids(what, tok, lg, ref_lg, dtype):
    """ids == the first-index argmax of the returned logits exactly; against the checker with its tie exemption."""
    V = lg.shape[-1]
    assert np.array_equal(tok.reshape(-1), lg.reshape(-1, V).argmax(axis=1)), f"{what}: ids != argmax(logits)"
    if ref_lg is not None:
        flat = ref_lg.reshape(-1, V)
        assert_ids_match(tok.reshape(-1), flat.argmax(axis=1), flat, what,
                         **({} if dtype == "bf16" else {"tol": 1e-3 * float(np.abs(flat).max())}))


def _run_sequence(st, ids, junk_seed):
    """Row 0: prefill 7, flagged S = 8 (two true tokens + six junk), flagged S = 2 at 9, unflagged S = 1 at 11."""
    V = st.vocab
    row = ids[0]
    t1, l1 = _fwd_dev(st, row[None, :7], 1, 7, 0, False)
    t2, l2 = _fwd_dev(st, np.concatenate([row[7:9], _junk(junk_seed, 6, V)])[None], 1, 8, 7, True)
    assert st.past[0] == 15
    st.rollback(0, 9)
    t3, l3 = _fwd_dev(st, row[None, 9:11], 1, 2, None, True)  # the host mirror: 9
    t4, l4 = _fwd_dev(st, row[None, 11:12], 1, 1, 11, False)
    assert st.past[0] == 12
    return (t1, l1), (t2, l2), (t3, l3), (t4, l4)


@pytest.mark.parametrize("cfg,dtype,variant", [(SMALL, "bf16", ""), (SMALL, "fp32", ""), (WIDE, "bf16", ""),
                                               (SMALL, "bf16", "w_int8")])
def test_stage_matches_teacher_forced_checker(cfg, dtype, variant):
    ids, ref = _reference(cfg, dtype, variant == "w_int8")
    kw = {"int8_weights": True} if variant == "w_int8" else {}
    what = f"{cfg} {dtype} {variant}"
    (t1, l1), (t2, l2), (t3, l3), (t4, l4) = _run_sequence(_stage(cfg, dtype, **kw), ids, 1)
    check_logits(l1[0], ref[0, 6], dtype, f"{what} prefill")
    check_logits(l2[0, :2], ref[0, 7:9], dtype, f"{what} flagged S=8, positions 7-8")
    check_logits(l3[0], ref[0, 9:11], dtype, f"{what} flagged S=2 at 9 after the rollback")
    check_logits(l4[0], ref[0, 11], dtype, f"{what} S=1 at 11")
    assert np.all(np.isfinite(l2)) and t2.shape == (1, 8) and t3.shape == (1, 2)
    _check_ids(f"{what} S=8", t2, l2, None, dtype)           # the junk positions too
    _check_ids(f"{what} S=8 valid", t2[:, :2], l2[:, :2], ref[0, 7:9], dtype)
    _check_ids(f"{what} S=2", t3, l3, ref[0, 9:11], dtype)
    _check_ids(f"{what} S=1", t4, l4, ref[0, 11:12], dtype)
    # other junk at positions 9-14: nothing valid moves, bit for bit
    (_, _), (u2, m2), (u3, m3), (u4, m4) = _run_sequence(_stage(cfg, dtype, **kw), ids, 2)
    assert np.array_equal(_bits(l2[:, :2]), _bits(m2[:, :2])) and np.array_equal(t2[:, :2], u2[:, :2])
    assert not np.array_equal(_bits(l2[:, 2:]), _bits(m2[:, 2:]))  # the junk positions did differ
    assert np.array_equal(_bits(l3), _bits(m3)) and np.array_equal(t3, u3), "stale junk at 11-14 reached S=2"
    assert np.array_equal(_bits(l4), _bits(m4)) and np.array_equal(t4, u4), "stale junk at 12-14 reached S=1"


def test_two_rows_with_different_rollbacks():
    """B = 2: both rows verified at 7 with junk tails of different lengths, then past_lens = [9, 12]."""
    cfg, dtype = SMALL, "bf16"
    ids, ref = _reference(cfg, dtype)
    V = cfg[3]
    st = _stage(cfg, dtype)
    _fwd_dev(st, ids[:, :7], 2, 7, 0, False)
    x2 = np.stack([np.concatenate([ids[0, 7:9], _junk(3, 6, V)]), np.concatenate([ids[1, 7:12], _junk(4, 3, V)])])
    t2, l2 = _fwd_dev(st, x2, 2, 8, [7, 7], True)
    check_logits(l2[0, :2], ref[0, 7:9], dtype, "B=2 S=8 row 0")
    check_logits(l2[1, :5], ref[1, 7:12], dtype, "B=2 S=8 row 1")
    _check_ids("B=2 S=8", t2, l2, None, dtype)
    x3 = np.stack([ids[0, 9:11], ids[1, 12:14]])
    t3, l3 = _fwd_dev(st, x3, 2, 2, [9, 12], True)
    assert st.past == [11, 14]
    check_logits(l3[0], ref[0, 9:11], dtype, "B=2 S=2 row 0 at 9")
    check_logits(l3[1], ref[1, 12:14], dtype, "B=2 S=2 row 1 at 12")
    _check_ids("B=2 S=2 row 0", t3[0], l3[0], ref[0, 9:11], dtype)
    _check_ids("B=2 S=2 row 1", t3[1], l3[1], ref[1, 12:14], dtype)
    x4 = np.stack([ids[0, 11:12], ids[1, 14:15]])
    t4, l4 = _fwd_dev(st, x4, 2, 1, [11, 14], False)
    check_logits(l4[0], ref[0, 11], dtype, "B=2 S=1 row 0 at 11")
    check_logits(l4[1], ref[1, 14], dtype, "B=2 S=1 row 1 at 14")


def test_three_stage_chain_with_the_flag_on_all_stages():
    """first / middle / last stages of the wide config, host I/O: the middle stage's hidden states and the logits."""
    h, nh, L, V = WIDE
    dtype = "bf16"
    ids, ref = _reference(WIDE, dtype)
    kw = dict(max_batch=1, max_ctx=NTOK + 8, seed=MSEED)
    dev = [Stage(h, nh, L, V, i, i + 1, dtype=dtype, max_tokens=32, **kw) for i in range(L)]
    chk = [OracleStage(h, nh, L, V, i, i + 1, bf16=True, **kw) for i in range(2)]
    row = ids[0]
    mid_ref = np.empty((NTOK, h), np.float32)  # the checker's middle-stage output, one position at a time
    for t in range(11):
        x = row[None, t:t + 1]
        for o in chk:
            x = o.forward(x, 1, 1, past_len=t)
        mid_ref[t] = x[0, 0]

    def chain(x, S, past, verify):
        mids = None
        for i, st in enumerate(dev):
            if i == L - 1:
                tok, lg = st.forward_host(x, 1, S, past_len=past, want_logits=True, verify=verify)
                return mids, tok, lg
            x = st.forward_host(x, 1, S, past_len=past, verify=verify)
            if i == 1:
                mids = x
    chain(row[None, :7], 7, 0, False)
    m2, t2, l2 = chain(np.concatenate([row[7:9], _junk(5, 6, V)])[None], 8, 7, True)
    m3, t3, l3 = chain(row[None, 9:11], 2, 9, True)
    check_close(m2[0, :2], mid_ref[7:9], dtype, "chain middle hidden, flagged S=8 positions 7-8")
    check_close(m3[0], mid_ref[9:11], dtype, "chain middle hidden, flagged S=2 at 9")
    check_logits(l2[0, :2], ref[0, 7:9], dtype, "chain logits, flagged S=8 positions 7-8")
    check_logits(l3[0], ref[0, 9:11], dtype, "chain logits, flagged S=2 at 9")
    _check_ids("chain S=8", t2, l2, None, dtype)
    _check_ids("chain S=2", t3, l3, ref[0, 9:11], dtype)


def test_mxfp4_stage_against_the_bf16_stage_of_its_weights():
    cfg, dtype = WIDE, "bf16"
    ids, _ = _reference(cfg, dtype)
    g = _stage(cfg, dtype, mxfp4_weights=True)
    r = _stage(cfg, dtype, host_weights=g.read_weights())
    got, want = _run_sequence(g, ids, 1), _run_sequence(r, ids, 1)
    for (tg, lg), (tr, lr), what, valid in zip(got, want, ("prefill", "S=8", "S=2", "S=1"), (1, 2, 2, 1)):
        lg, lr = lg.reshape(-1, cfg[3])[:valid], lr.reshape(-1, cfg[3])[:valid]
        check_logits(lg, lr, dtype, f"mxfp4 {what}")
        _check_ids(f"mxfp4 {what}", tg.reshape(-1)[:valid], lg, lr, dtype)


# ---- C: invariants
def test_graph_replay_equals_eager_and_runs_are_bit_identical():
    """Device buffers (captured and replayed) against a set_graphs(False) twin: ids, logits and a middle stage's hidden
    states bit for bit, including a second replay of one captured shape at other positions; two identical runs agree
    bit for bit; host I/O returns the same bits."""
    import torch
    h, nh, L, V = SMALL
    ids, _ = _reference(SMALL, "bf16")
    row = ids[0]

    def run(graphs, split):
        if split:  # first + middle stage (hidden out) feeding a last stage
            sts = [Stage(h, nh, L, V, 0, 1, dtype="bf16", max_ctx=NTOK + 8, max_tokens=32, seed=MSEED),
                   Stage(h, nh, L, V, 1, 2, dtype="bf16", max_ctx=NTOK + 8, max_tokens=32, seed=MSEED)]
        else:
            sts = [Stage(h, nh, L, V, 0, L, dtype="bf16", max_ctx=NTOK + 8, max_tokens=32, seed=MSEED)]
        for st in sts:
            st.set_graphs(graphs)
        # fixed buffers: the second pass of a shape replays the first one's graph
        xd = torch.empty(4, dtype=torch.int32, device=DEV)
        hid = torch.empty((4, h), dtype=torch.float32, device=DEV)
        out = torch.empty(4, dtype=torch.int32, device=DEV)
        lg = torch.empty((4, V), dtype=torch.float32, device=DEV)
        pre = torch.from_numpy(np.array(row[:5])).to(DEV)
        hp = torch.empty((5, h), dtype=torch.float32, device=DEV)
        tp = torch.empty(1, dtype=torch.int32, device=DEV)
        stream = torch.cuda.Stream()
        res = []
        with torch.cuda.stream(stream):
            sh = stream.cuda_stream
            if split:
                sts[0].forward(pre, hp, 1, 5, past_len=0, stream=sh)
                sts[1].forward(hp, tp, 1, 5, past_len=0, stream=sh)
            else:
                sts[0].forward(pre, tp, 1, 5, past_len=0, stream=sh)
            for past, toks in ((5, row[5:9]), (9, row[9:13]), (7, row[3:7])):  # the last one after a rollback
                xd.copy_(torch.from_numpy(np.array(toks)))
                if split:
                    sts[0].forward(xd, hid, 1, 4, past_len=past, stream=sh, verify=True)
                    sts[1].forward(hid, out, 1, 4, past_len=past, logits=lg, stream=sh, verify=True)
                else:
                    sts[0].forward(xd, out, 1, 4, past_len=past, logits=lg, stream=sh, verify=True)
                stream.synchronize()
                res.append((out.cpu().numpy().copy(), lg.cpu().numpy().copy(), hid.cpu().numpy().copy()))
        return res

    whole = None
    for split in (False, True):
        a, b, c = run(True, split), run(False, split), run(True, split)
        whole = a if whole is None else whole
        for i, ((ta, la, ha), (tb, lb, hb), (tc, lc, hc)) in enumerate(zip(a, b, c)):
            assert np.array_equal(ta, tb) and np.array_equal(_bits(la), _bits(lb)), f"graph != eager, pass {i}"
            assert np.array_equal(ta, tc) and np.array_equal(_bits(la), _bits(lc)), f"two runs differ, pass {i}"
            if split:
                assert np.array_equal(_bits(ha), _bits(hb)) and np.array_equal(_bits(ha), _bits(hc)), f"hidden {i}"
            assert np.array_equal(ta, la.argmax(axis=1))
    # host I/O: the same bits as the device-buffer pass
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_ctx=NTOK + 8, max_tokens=32, seed=MSEED)
    st.forward_host(row[None, :5], 1, 5, past_len=0)
    th, lh = st.forward_host(row[None, 5:9], 1, 4, past_len=5, want_logits=True, verify=True)
    assert th.shape == (1, 4) and lh.shape == (1, 4, V)
    assert np.array_equal(th[0], whole[0][0]) and np.array_equal(_bits(lh[0]), _bits(whole[0][1]))
    assert st.read_head_screen() is None  # the verify tail is never screened


@pytest.mark.parametrize("variant", ["bf16", "fp32", "w_int8", "mxfp4"])
def test_kv_equals_the_unflagged_pass_bit_for_bit(variant):
    """The linears of a flagged pass are the unflagged pass's, so the K / V rows they write are the same bits.  Layer 0
    sees identical inputs in both passes.  A deeper layer sees the attention's context, which the two passes compute
    with different kernels: a bf16 stage rounds it to bf16 and both round to the same values here, so every layer
    must agree bit for bit; an fp32 stage keeps the summation-order difference (a few fp32 ulp), so its deeper layers
    are held to the fp32 tolerance of check_close (1e-3 relative) instead."""
    h, nh, L, V = SMALL
    dtype = "fp32" if variant == "fp32" else "bf16"
    kw = {"w_int8": {"int8_weights": True}, "mxfp4": {"mxfp4_weights": True}}.get(variant, {})
    ids, _ = _reference(SMALL, "bf16")
    for B, S in ((1, 2), (2, 5), (1, 8)):
        g = Stage(h, nh, L, V, 0, L, dtype=dtype, max_batch=2, max_ctx=NTOK + 8, max_tokens=32, seed=MSEED, **kw)
        p = Stage(h, nh, L, V, 0, L, dtype=dtype, max_batch=2, max_ctx=NTOK + 8, max_tokens=32, seed=MSEED, **kw)
        for st in (g, p):
            st.forward_host(ids[:B, :6], B, 6, past_len=0)
        tg = g.forward_host(ids[:B, 6:6 + S], B, S, past_len=6, verify=True)
        tp = p.forward_host(ids[:B, 6:6 + S], B, S, past_len=6)
        assert g.past[:B] == p.past[:B] == [6 + S] * B
        assert np.array_equal(tg[:, -1], tp)  # the unflagged pass picks each row's last position
        for layer in range(L):
            for row in range(B):
                a, b = g.read_kv(layer, row, 0, 6 + S), p.read_kv(layer, row, 0, 6 + S)
                what = f"{variant} B={B} S={S} KV layer {layer} row {row}"
                if variant == "fp32" and layer > 0:
                    check_close(a, b, "fp32", what)
                else:
                    assert np.array_equal(_bits(a), _bits(b)), what


def _raw(st, step, x, out, logits=None):
    return bs.lib().bs_forward(st._h, ctypes.byref(step), bs._ptr(x), bs._ptr(out), bs._ptr(logits), None)


def test_statuses_and_abi_version():
    assert bs.lib().bs_abi_version() == 5
    VF = bs.BS_STEP_VERIFY | bs.BS_STEP_HOST_IO
    ids = np.zeros((1, 2), np.int32)
    x = np.zeros((1, 2, 64), np.float32)
    out, hid = np.empty((4, 8), np.int32), np.empty((1, 8, 64), np.float32)
    ok = Stage(64, 4, 2, 512, 0, 2, dtype="bf16", max_batch=8, max_ctx=16, max_tokens=64, seed=1)
    assert _raw(ok, Step(1, 2, 0, 0, VF, None), ids, out) == 0
    assert _raw(ok, Step(1, 1, 0, 0, VF, None), ids, out) == -1                               # seq < 2
    assert _raw(ok, Step(1, 9, 0, 0, VF, None), np.zeros((1, 9), np.int32), out) == -1        # seq > 8
    assert _raw(ok, Step(5, 7, 0, 0, VF, None), np.zeros((5, 7), np.int32), np.empty((5, 7), np.int32)) == -1  # > 32
    assert _raw(ok, Step(4, 8, 0, 0, VF, None), np.zeros((4, 8), np.int32), out) == 0         # 32 positions
    assert _raw(ok, Step(1, 2, 0, 15, VF, None), ids, out) == -1                              # past max_ctx
    kv8 = Stage(64, 4, 2, 512, 0, 2, dtype="bf16", max_ctx=16, seed=1, kv_int8=True)
    assert _raw(kv8, Step(1, 2, 0, 0, VF, None), ids, out) == -5                              # BS_ERR_UNSUPPORTED
    cls = Stage(64, 4, 2, 512, 1, 2, dtype="bf16", max_ctx=16, seed=1, n_labels=2)
    assert _raw(cls, Step(1, 2, 0, 0, VF, None), x, out) == -4                                # BS_ERR_STATE
    smp = Stage(64, 4, 2, 512, 0, 2, dtype="bf16", max_ctx=16, seed=1)
    smp.set_sampling(4, 1.0, 7)
    assert _raw(smp, Step(1, 2, 0, 0, VF, None), ids, out) == -4
    smp.set_sampling(1)
    assert _raw(smp, Step(1, 2, 0, 0, VF, None), ids, out) == 0
    slc = Stage(64, 4, 3, 512, 2, 3, dtype="bf16", max_ctx=16, seed=1, head_slice=(0, 256))
    assert _raw(slc, Step(1, 2, 0, 0, VF, None), x, out) == -4                                # not the whole head
    mid = Stage(64, 4, 3, 512, 1, 2, dtype="bf16", max_ctx=16, seed=1)
    assert _raw(mid, Step(1, 2, 0, 0, VF, None), x, hid) == 0                                 # any stage of the model
    # the scoring pass rejects the flag
    top = np.empty((1, 2), np.int32)
    assert bs.lib().bs_forward_score(ok._h, ctypes.byref(Step(1, 2, 0, 0, VF, None)), bs._ptr(ids), None,
                                     bs._ptr(top), None, None) == -1
    with pytest.raises(BloomStageError, match="error -5"):
        kv8.forward_host(ids, 1, 2, past_len=0, verify=True)


def test_workspace_grows_at_the_first_verify_call_only():
    h, nh, L, V = 64, 4, 1, 2048
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_batch=2, max_ctx=600, max_tokens=64, seed=3)
    ids = gen_np.prompt_ids(9, 2, 8, V).astype(np.int32)
    before = st.info()["workspace_bytes"]
    st.forward_host(ids, 2, 8, past_len=0)
    st.forward_host(ids[:, :1], 2, 1, past_len=8)
    assert st.info()["workspace_bytes"] == before
    st.forward_host(ids[:, :4], 2, 4, past_len=9, verify=True)
    after = st.info()["workspace_bytes"]
    assert after > before
    st.forward_host(ids, 2, 8, past_len=13, verify=True)
    st.forward_host(ids[:1, :2], 1, 2, past_len=21, verify=True, want_logits=True)
    assert st.info()["workspace_bytes"] == after
