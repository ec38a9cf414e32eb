"""BS_STEP_VERIFY_DRAW on the GPU: a verify pass whose last stage returns the row sampler's draw at every position.

Model: bf16, hidden 64, 4 heads, 2 layers, vocab 6160 -- the row sampler runs ceil(6160 / 2048) = 4 blocks per
selection, the last one on 16 logits, and the pick scans two 4096-logit tiles, the second ragged: the cross-block
histogram merge and the ragged tile are exercised (at vocab 512 one block does everything).

  exactness   every draw of a pass equals bs_sample_logits on that position's logits, EXACTLY (the sampler's integer
              arithmetic makes a draw a function of (state, position, logits) alone), and its read-out passes the
              float64 checker of tests/row_sampling_ref.py;
  hygiene     the pass advances the device position once a row, leaves the per-row scratch alone, replays as it
              launches eagerly, and follows a state change without a recapture;
  statuses    the table of include/bloomstage.h;
  agreement   a twin stage fed the plain sampled decode's tokens in verify-draw passes of S = 5 draws those tokens
              wherever u lies further inside the token's CDF interval than the measured logit difference can move it.

The agreement fixture: the generator's ln_f gives logits within about +-1.2 (the echoed token leads by 0.6), a softmax
over 6160 tokens that is flat (largest probability below 1e-3) at every temperature for which the bound
2 (exp(2 * 2e-2 / T) - 1) stays below 1/2 -- no position could clear it.  The fixture therefore scales ln_f's weight
and bias by 16, an exact power of two: every logit is exactly 16 times the generator's, and the distribution is as
peaked as a trained model's (the echoed token holds about 0.99 at T = 1.5).  The sampler seeds below were chosen on the
CPU from the checker's logits (times 16) of the plain sampled decode.
"""
import ctypes

import numpy as np
import pytest
import torch

import row_sampling_ref as ref
from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.speculative import SpeculativeDecoder, StageChain, StageDrafter
from distributed_inference_demo_amd.stage import BloomStageError, Stage
from oracle import gen_np

from test_gpu_parity import canonical_weights

pytestmark = pytest.mark.gpu

H, NH, L, V = 64, 4, 2, 6160
TOPK, TOPP, BOTH, FULL = (50, 1.0, 2.0), (0, 0.9, 3.0), (40, 0.8, 2.5), (0, 1.0, 1.5)  # (top_k, top_p, temperature)


def tiny(max_batch=1, max_ctx=64, seed=31, **kw):
    return Stage(H, NH, L, V, 0, L, dtype="bf16", max_batch=max_batch, max_ctx=max_ctx, max_tokens=32, seed=seed, **kw)


def warm(g, slot, pasts, seed=200):
    """Prefill row slot + b with pasts[b] tokens, one row a call."""
    for b, n in enumerate(pasts):
        g.forward_host(gen_np.prompt_ids(seed + b, 1, n, V).astype(np.int32), 1, n, slot=slot + b, past_len=0)


def set_states(g, slot, states, stream=None):
    for b, st in enumerate(states):
        if st is None:
            g.clear_row_sampler(slot + b, stream=stream)
        else:
            g.set_row_sampler(slot + b, top_k=st[0], top_p=st[1], temperature=st[2], seed=st[3], stream=stream)


def expected(g, slot, pasts, logits):
    """bs_sample_logits on every position's logits [B][S][V] with the rows' current states: [B][S]."""
    B, S = logits.shape[:2]
    return np.stack([g.sample_logits(np.ascontiguousarray(logits[:, t]), [pasts[b] + t + 1 for b in range(B)],
                                     slot=slot) for t in range(S)], axis=1)


# ---- 1. exactness
@pytest.mark.parametrize("B,S,pasts,kinds", [
    (1, 2, [5], [TOPP]),
    (1, 8, [11], [BOTH]),
    (4, 8, [3, 17, 9, 1], [TOPK, TOPP, None, BOTH]),
    (3, 5, [7, 2, 13], [FULL, None, TOPK]),
])
def test_every_draw_equals_the_row_sampler_on_its_logits(B, S, pasts, kinds):
    slot = 1
    g = tiny(max_batch=5)
    warm(g, slot, pasts)
    states = [None if k is None else k + (1000 + 17 * b,) for b, k in enumerate(kinds)]
    set_states(g, slot, states)
    ids = gen_np.prompt_ids(77, B, S, V).astype(np.int32)
    toks, lg = g.forward_host(ids, B, S, slot=slot, past_len=pasts, want_logits=True, verify=True, draw=True)
    assert toks.shape == (B, S) and lg.shape == (B, S, V)
    want = expected(g, slot, pasts, lg)
    stateful = differ = 0
    for b in range(B):
        for t in range(S):
            what = f"B={B} S={S} row {b} position {t}"
            pos = pasts[b] + t + 1
            d = g.read_verify_draw(slot + b, t)
            assert d["token"] == int(toks[b, t]) and d["position"] == pos, (what, d)
            if states[b] is None:
                assert int(toks[b, t]) == ref.first_argmax(lg[b, t]), what
                continue
            assert int(toks[b, t]) == int(want[b, t]), f"{what}: pass drew {toks[b, t]}, bs_sample_logits {want[b, t]}"
            ref.check_readout(lg[b, t], states[b], pos, d, what)
            stateful += 1
            differ += int(toks[b, t]) != ref.first_argmax(lg[b, t])
    print(f"B={B} S={S}: {differ} of {stateful} stateful draws differ from the argmax")
    assert 4 * differ >= stateful, "the fixture degenerated to greedy"
    with pytest.raises(BloomStageError, match="error -1"):
        g.read_verify_draw(slot + B, 0)
    with pytest.raises(BloomStageError, match="error -1"):
        g.read_verify_draw(slot, S)
    with pytest.raises(BloomStageError, match="error -1"):
        g.read_verify_draw(slot - 1, 0)


# ---- 2. positions and scratch hygiene
def test_positions_scratch_replay_and_state_changes():
    B, S, pasts = 2, 4, [6, 9]
    g = tiny(max_batch=B)
    warm(g, 0, pasts)
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    states = [BOTH + (5,), TOPP + (6,)]
    with torch.cuda.stream(cs):
        sh = cs.cuda_stream
        set_states(g, 0, states, stream=sh)
        ids = torch.from_numpy(gen_np.prompt_ids(78, B, S, V).astype(np.int32)).to(dev)
        tok = torch.empty((B, S), dtype=torch.int32, device=dev)
        lg = torch.empty((B, S, V), dtype=torch.float32, device=dev)
        tok1 = torch.empty(B, dtype=torch.int32, device=dev)
        lg1 = torch.empty((B, V), dtype=torch.float32, device=dev)

        def run(logits=lg):
            tok.fill_(-1)
            g.forward(ids, tok, B, S, slot=0, past_len=pasts, logits=logits, stream=sh, verify=True, draw=True)
            torch.cuda.synchronize()
            return tok.cpu().numpy().copy()

        ws0 = g.info()["workspace_bytes"]
        t0 = run(logits=None)  # the first verify-draw pass: scratch and the pass's own logits buffer
        ws1 = g.info()["workspace_bytes"]
        assert ws1 >= ws0 + 32 * (9 * 2048 * 4) + 32 * V * 4, (ws0, ws1)
        t1 = run()
        l1 = lg.cpu().numpy().copy()
        assert np.array_equal(t0, t1), "the pass's own logits buffer and the caller's give different draws"
        assert np.array_equal(t1, expected(g, 0, pasts, l1))
        assert 4 * int((t1 != l1.argmax(-1)).sum()) >= B * S
        for i in range(2):  # rolled back by passing the same positions: three passes in a row agree
            assert np.array_equal(run(), t1), f"pass {i + 2} of the same shape differs"
        # a graph-replayed sampled step that finds the rows' positions on the device: the pass advanced them by S once
        after = [p + S for p in pasts]
        tok1.copy_(torch.from_numpy(t1[:, -1].copy()))
        g.forward(tok1, tok1, B, 1, slot=0, past_len=after, logits=lg1, stream=sh)
        torch.cuda.synchronize()
        s1, sl = tok1.cpu().numpy(), lg1.cpu().numpy()
        for r in range(B):
            d = g.read_row_draw(r)
            assert d["position"] == after[r] + 1, f"row {r}: drew at {d['position']}, the row held {after[r]} positions"
            assert d["token"] == int(s1[r])
        assert np.array_equal(s1, g.sample_logits(sl, [p + 1 for p in after], slot=0)), "the plain step between passes"
        assert np.array_equal(run(), t1), "a pass after a plain sampled step differs"
        assert g.info()["workspace_bytes"] == ws1, "only the first verify-draw pass allocates"
        # another seed for row 0 between two replays of the same graph
        states[0] = BOTH + (999,)
        set_states(g, 0, states[:1], stream=sh)
        t2 = run()
        assert np.array_equal(lg.cpu().numpy(), l1)
        assert np.array_equal(t2, expected(g, 0, pasts, l1)), "the replay did not follow the new state"
        assert np.array_equal(t2[1], t1[1]) and not np.array_equal(t2[0], t1[0])
        assert g.read_verify_draw(0, 2)["u24"] == ref.draw_u24(999, pasts[0] + 3)
        g.set_graphs(False)
        t3 = run()
        assert np.array_equal(t3, t2) and np.array_equal(lg.cpu().numpy(), l1), "eager launch and replay differ"
        assert g.info()["workspace_bytes"] == ws1


# ---- 3. statuses
def raw_forward(g, flags, x, batch, seq, slot, past, score=False):
    """bs_forward / bs_forward_score with any flags (the binding refuses draw without verify itself)."""
    st = bs.Step(batch, seq, slot, past, flags | bs.BS_STEP_HOST_IO, None)
    x = np.ascontiguousarray(x, np.int32)
    out = np.empty((batch, seq), np.int32)
    if score:
        return bs.lib().bs_forward_score(g._h, ctypes.byref(st), x.ctypes.data, None, out.ctypes.data, None, None)
    return bs.lib().bs_forward(g._h, ctypes.byref(st), x.ctypes.data, out.ctypes.data, None, None)


def test_statuses():
    g = tiny(max_batch=2, max_ctx=24)
    x = gen_np.prompt_ids(2, 2, 4, V).astype(np.int32)
    g.forward_host(x, 2, 4, slot=0, past_len=0)
    ws0 = g.info()["workspace_bytes"]
    with pytest.raises(BloomStageError, match="error -4"):
        g.read_verify_draw(0, 0)
    with pytest.raises(ValueError):
        g.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, draw=True)
    assert raw_forward(g, bs.BS_STEP_VERIFY_DRAW, x[:1, :3], 1, 3, 0, 4) == -1  # the flag alone
    assert raw_forward(g, bs.BS_STEP_VERIFY_DRAW, x[:1, :3], 1, 3, 0, 4, score=True) == -1
    assert raw_forward(g, bs.BS_STEP_VERIFY | bs.BS_STEP_VERIFY_DRAW, x[:1, :3], 1, 3, 0, 4, score=True) == -1
    # no row holds state: the unflagged verify pass, bit for bit, and nothing is allocated for the sampler
    a, la = g.forward_host(x[:, :3], 2, 3, slot=0, past_len=4, want_logits=True, verify=True)
    ws1 = g.info()["workspace_bytes"]
    b, lb = g.forward_host(x[:, :3], 2, 3, slot=0, past_len=4, want_logits=True, verify=True, draw=True)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and np.array_equal(a, la.argmax(-1))
    assert g.info()["workspace_bytes"] == ws1 and ws1 > ws0
    with pytest.raises(BloomStageError, match="error -4"):
        g.read_verify_draw(0, 0)
    # bs_set_sampling top_k > 1: BS_ERR_STATE, with or without the flag
    g.set_sampling(4, 1.0, 1)
    for draw in (False, True):
        with pytest.raises(BloomStageError, match="error -4"):
            g.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True, draw=draw)
    g.set_sampling(1)
    g.set_row_sampler(0, top_p=0.9, temperature=2.0, seed=3)
    with pytest.raises(BloomStageError, match="error -4"):  # BS_STEP_VERIFY alone on a stateful row, as before
        g.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True)
    with pytest.raises(BloomStageError, match="error -1"):  # the shape limits are the verify pass's
        g.forward_host(x[:1, :1], 1, 1, slot=0, past_len=4, verify=True, draw=True)
    t = g.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True, draw=True)
    assert t.shape == (1, 3) and g.read_verify_draw(0, 1)["token"] == int(t[0, 1])
    with pytest.raises(BloomStageError, match="error -1"):
        g.read_verify_draw(1, 0)  # row 1 was not part of that pass
    # a non-last stage takes the flag and ignores it
    first = Stage(H, NH, L, V, 0, 1, dtype="bf16", max_ctx=24, max_tokens=32, seed=31)
    first.forward_host(x[:1], 1, 4, slot=0, past_len=0)
    h0 = first.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True)
    h1 = first.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True, draw=True)
    assert np.array_equal(h0, h1)
    k8 = tiny(kv_int8=True)
    k8.forward_host(x[:1], 1, 4, slot=0, past_len=0)
    with pytest.raises(BloomStageError, match="error -5"):  # an int8 KV cache has no verify pass
        k8.forward_host(x[:1, :3], 1, 3, slot=0, past_len=4, verify=True, draw=True)


# ---- 4. agreement with plain sampled decoding
EP, EN, MSEED, SCALE = 12, 32, 1, 16.0
TOL = 2e-2  # the project's logits tolerance (tests/test_gpu_parity.py BF16_TOL)
FIX_A = dict(top_k=0, top_p=1.0, temperature=1.5, seed=5)   # three draws off the argmax; smallest margin 5.8e-6
FIX_B = dict(top_k=0, top_p=1.0, temperature=1.25, seed=3)  # every margin >= 0.028: no draw near an interval's end


def peaked_weights():
    w = canonical_weights(MSEED, H, L, V)
    w[-2 * H:] *= np.float32(SCALE)  # ln_f weight and bias: every logit exactly SCALE times the generator's
    return w


def peaked(**kw):
    return Stage(H, NH, L, V, 0, L, dtype="bf16", max_batch=1, max_ctx=EP + EN + 8, max_tokens=32,
                 host_weights=peaked_weights(), **kw)


def bound(delta, T):
    """What a logit perturbation of at most delta moves a partial or total mass by, twice (both sides of u * mass),
    plus the sampler's own arithmetic (row_sampling_ref.EPS)."""
    return 2.0 * (np.exp(2.0 * delta / T) - 1.0) + 2.0 ** -16


_PLAIN = {}


def plain_sampled(fix):
    """The plain sampled decode of the peaked stage with state `fix`, once: (prompt, tokens x [EN], logits L [EN][V],
    margins [EN]).  margin_i: the distance from u * mass to the nearer end of x_i's CDF interval over the mass."""
    key = fix["seed"]
    if key not in _PLAIN:
        g = peaked()
        g.set_row_sampler(0, **fix)
        prompt = gen_np.prompt_ids(5, 1, EP, V).astype(np.int32)
        x, past, toks, L, margins = prompt, 0, [], [], []
        for i in range(EN):
            S = x.shape[1]
            tk, lg = g.forward_host(x, 1, S, slot=0, past_len=past, want_logits=True)
            past += S
            l = lg[0].astype(np.float64)
            w = np.exp((l - l.max()) / float(np.float32(fix["temperature"])))
            cum = np.cumsum(w)
            t = int(tk[0])
            target = ref.draw_u24(fix["seed"], past) / 2.0 ** 24 * cum[-1]
            margins.append(min(target - (cum[t] - w[t]), cum[t] - target) / cum[-1])
            toks.append(t)
            L.append(lg[0].copy())
            x = tk.reshape(1, 1)
        _PLAIN[key] = (prompt.reshape(-1).tolist(), toks, np.stack(L), np.array(margins))
    return _PLAIN[key]


def test_teacher_forced_passes_draw_the_plain_decodes_tokens():
    """Fixture: model seed 1 with ln_f x 16, top_k = 0, top_p = 1, T = 1.5, sampler seed 5 (chosen on the CPU from the
    checker's logits: 29 of the 32 positions clear the bound at 2e-2, three draws are off the argmax, the smallest
    margin is 5.8e-6 -- a draw the assertion rightly leaves out).  Measured on the MI355X: the largest delta_i is
    1.9e-6, 30 positions clear their own bound and all 32 draws agree."""
    fix = FIX_A
    T = fix["temperature"]
    prompt, x, L, margins = plain_sampled(fix)
    clear = margins > bound(TOL, T)
    print(f"margins: min {margins.min():.3e}, {int(clear.sum())} of {EN} clear {bound(TOL, T):.4f}; "
          f"{sum(int(t) != int(l.argmax()) for t, l in zip(x, L))} draws off the argmax")
    assert 4 * int(clear.sum()) >= 3 * EN, "the fixture leaves the assertion vacuous"
    twin = peaked()
    twin.set_row_sampler(0, **fix)
    t0, p0 = twin.forward_host(np.array([prompt], np.int32), 1, EP, slot=0, past_len=0, want_logits=True)
    assert int(t0[0]) == x[0] and np.array_equal(p0[0], L[0])  # the same prefill
    D, P = {0: x[0]}, {0: p0[0]}
    for i in range(0, EN - 1, 5):  # x_i .. x_(i+4) fed at EP + i draw D_(i+1) .. D_(i+5)
        lo = min(i, EN - 1 - 2)    # the last chunk holds one token: start it one earlier (a rollback by one)
        chunk = x[lo:min(i + 5, EN - 1)]
        d, p = twin.forward_host(np.array([chunk], np.int32), 1, len(chunk), slot=0, past_len=EP + lo,
                                 want_logits=True, verify=True, draw=True)
        for j in range(len(chunk)):
            D[lo + j + 1], P[lo + j + 1] = int(d[0, j]), p[0, j]
    delta = np.array([np.abs(P[i] - L[i]).max() for i in range(EN)])
    need = np.array([bound(delta[i], T) for i in range(EN)])
    print("delta_i = max|P_i - L_i|:", " ".join(f"{v:.2e}" for v in delta))
    print(f"largest delta {delta.max():.3e}; {int((margins > need).sum())} of {EN} positions clear their own bound; "
          f"{sum(D[i] == x[i] for i in range(EN))} of {EN} draws agree")
    for i in range(EN):
        if margins[i] > need[i]:
            assert D[i] == x[i], f"position {i}: pass drew {D[i]}, plain decode {x[i]} (margin {margins[i]:.3e}, " \
                                 f"delta {delta[i]:.3e}, bound {need[i]:.3e})"


# ---- 5. decoder and serve
class Replay:
    def __init__(self, truth, n0, wrong=False):
        self.truth, self.n0, self.wrong = truth, n0, wrong

    def propose(self, history, k):
        done = len(history) - self.n0
        return [(t + 1) % V if self.wrong else t for t in self.truth[done:done + k]]


class Recording:
    """Records every proposal of a drafter with the history length it was made at."""

    def __init__(self, inner):
        self.inner, self.rounds = inner, []

    def propose(self, history, k):
        d = list(self.inner.propose(history, k))
        self.rounds.append((len(history), d))
        return d


def test_sampled_decoder_with_replay_wrong_twin_and_int8_drafters():
    """Fixture: as above with T = 1.25, sampler seed 3 (on the CPU 30 of the 32 positions clear the bound at 2e-2 and
    the smallest margin is 0.028: no draw sits near an end of its interval, so the three runs, which reach a position
    through passes of different alignment, see the same contexts)."""
    fix, k = FIX_B, 4
    T = fix["temperature"]
    prompt, truth, L, margins = plain_sampled(fix)
    print(f"margins: min {margins.min():.3e}; {int((margins > bound(TOL, T)).sum())} of {EN} clear {bound(TOL, T):.4f}")
    clear = margins > bound(TOL, T)
    assert 4 * int(clear.sum()) >= 3 * EN, "the fixture leaves the assertions vacuous"
    tgt = peaked()
    toks, stats = SpeculativeDecoder([tgt], Replay(truth, EP), k, sampler=fix).generate(prompt, EN)
    print(f"replay drafter: {stats}")
    assert stats["accepted"] == stats["drafted"], "a pass of the target's own continuation emits k + 1 tokens"
    assert stats["passes"] + stats["plain_steps"] == -(-(EN - 1) // (k + 1)) and stats["plain_steps"] <= 1
    d = tgt.read_verify_draw(0, 0)  # the sampler ran, keyed by this seed and the row's position
    assert d["u24"] == ref.draw_u24(fix["seed"], d["position"]) and d["position"] > EP
    wrong, wstats = SpeculativeDecoder([peaked()], Replay(truth, EP, wrong=True), k, sampler=fix).generate(prompt, EN)
    print(f"wrong drafter: {wstats}")
    assert wstats["accepted"] == 0 and wstats["passes"] == EN - 2
    rec = Recording(StageDrafter([peaked()], k, sampler=fix))
    twin, tstats = SpeculativeDecoder([peaked()], rec, k, sampler=fix).generate(prompt, EN)
    print(f"bf16 twin drafter: {tstats}")
    assert toks == wrong == twin, "the three runs emit different tokens"
    same = int(np.argmin(clear)) if not clear.all() else EN  # the contexts are the plain decode's up to there
    print(f"the plain sampled decode's tokens: {sum(a == b for a, b in zip(toks, truth))} of {EN} equal")
    assert toks[:same] == truth[:same], "the decoder left plain sampled decoding at a position clearing the margin"
    for n, draft in rec.rounds:  # draft[j] proposes token n - EP + j of the generation
        for j, t in enumerate(draft):
            i = n - EP + j
            if clear[n - EP:i + 1].all():
                assert t == twin[i], f"twin draft of token {i} refused at a position clearing the margin"
    q8 = StageDrafter([peaked(int8_weights=True)], k, sampler=fix)
    qt, qstats = SpeculativeDecoder([peaked()], q8, k, sampler=fix).generate(prompt, EN)
    print(f"int8 coupled drafter: {qstats}")
    assert qstats["accepted"] > 0 and qt == toks


def test_serve_sample_speculate_equals_the_decoder_run_directly():
    from distributed_inference_demo_amd.config import BloomDims
    from distributed_inference_demo_amd.serve import RunConfig, request_seed, run_rank
    from distributed_inference_demo_amd.speculative import NgramDrafter
    m = BloomDims("tiny-sample-spec", H, L, NH, vocab=V)
    state = dict(top_k=30, top_p=0.9, temperature=1.5)
    n, ml, pl = 3, 16, 9
    cfg = RunConfig(model=m, num_sample=n, max_length=ml, prompt_len=pl, sample=True, sample_speculate=4,
                    sample_seed=5, seed=13, **state)
    res = run_rank(cfg, 0, 1, torch.device("cuda", 0))
    print({k: v for k, v in res.items() if k != "samples"})
    assert res["sample"] is True and res["sample_speculate"] == 4 and res["sample_seed"] == 5
    assert {k: res[k] for k in state} == state
    assert res["passes"] + res["plain_steps"] + res["accepted"] == n * (ml - 1)
    g = Stage(H, NH, L, V, 0, L, dtype="bf16", max_batch=1, max_ctx=pl + ml + 1, max_tokens=pl + 32, seed=13)
    chain = StageChain([g])
    drafter = NgramDrafter(4)
    for i in range(n):
        prompt = bs.prompt_ids(1234 + i, 1, pl, V).reshape(-1).tolist()
        sampler = dict(state, seed=request_seed(5, i))
        toks, _ = SpeculativeDecoder(chain, drafter, 4, sampler=sampler).generate(prompt, ml)
        assert res["samples"][i] == toks, f"sample {i}"
    assert len({tuple(s) for s in res["samples"]}) == n
