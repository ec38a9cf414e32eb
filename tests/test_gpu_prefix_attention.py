"""Shared-prefix decode attention (bs_set_row_prefix, csrc/attn_prefix.hip): the prefix of a template row streamed
once per head for all rows of a decode step, each row's own positions and the merge in a second launch.

  exact      every context element of the shared route against float64 attention on the device's own cache, with
             tests/test_gpu_attention_exact.py's one-layer identity stage and its bound, unchanged: half a bf16 ulp of
             the reference + 2^-14 max|V|.  head_dim 64 / 80 / 96 / 128; 2, 16, 17 and 32 rows (one query tile, a full
             one, a second with one live row, two full ones); prefixes of 1, 63, 64 and 700 positions (under a chunk,
             the chunk edge, several splits and waves, with max_ctx = 1024: 4 splits, the trailing ones empty for the
             short prefixes); tails of 0 positions and one whose suffix crosses 64 positions during the steps.
  not read   the rows' own first P positions overwritten with another template's: the same bits out.
  agreement  a tiny full model: the greedy ids of the plain route, logits within the bf16 bound of
             tests/test_gpu_parity.py, graph replay == eager launches and run == run bit for bit.
  fallbacks  differing declarations, one row, seq > 1: the plain route's bits; the statuses; the workspace; reset.
"""
import numpy as np
import pytest
import torch

from distributed_inference_demo_amd.stage import BloomStageError, Stage, lib
from oracle.oracle import alibi_slopes

from test_gpu_attention_exact import _x, bf16_ulp, identity_attention_weights
from test_gpu_parity import BF16_TOL, record_error

pytestmark = pytest.mark.gpu

NH, CTX = 4, 1024


def shared_steps(hd, B, P, tails, overwrite=False, check=None):
    """Template row B prefilled with P tokens and forked into rows [0, B), row b's own tail of tails[b] tokens, the
    declaration, 3 decode steps.  overwrite: before the steps, another template's P positions land in the rows' own
    first P positions.  Returns the steps' outputs; check: every context element against float64 attention."""
    h = NH * hd
    st = Stage(h, NH, 1, 512, 0, 1, dtype="bf16", max_batch=B + 2, max_ctx=CTX, max_tokens=max(P, B, max(tails)),
               host_weights=identity_attention_weights(h, NH), is_first=False, is_last=False)
    rng = np.random.default_rng(100 * hd + 10 * B + P)
    st.forward_host(_x(rng, 1, P, h), 1, P, slot=B, past_len=[0])
    st.fork_kv(B, 0, npos=P, count=B)
    for b, t in enumerate(tails):
        if t:
            st.forward_host(_x(rng, 1, t, h), 1, t, slot=b, past_len=[P])
    if overwrite:
        st.forward_host(_x(np.random.default_rng(7), 1, P, h), 1, P, slot=B + 1, past_len=[0])  # rng: the steps' inputs stay
        st.fork_kv(B + 1, 0, npos=P, count=B)
    st.set_row_prefix(0, B, P, count=B)
    slopes, inv_norm = alibi_slopes(NH).astype(np.float64), float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    outs, worst = [], 0.0
    for step in range(3):
        pasts = [P + t + step for t in tails]
        x = _x(rng, B, 1, h)
        out = st.forward_host(x, B, 1, slot=0, past_len=pasts)
        outs.append(out)
        if check is None:
            continue
        ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(B, NH, hd)
        for b in range(B):
            n = pasts[b] + 1
            K, V = st.read_kv(0, b, 0, n).astype(np.float64)  # [nh][n][hd] each
            for j in range(NH):
                s = inv_norm * (K[j] @ K[(j - 1) % NH, n - 1]) + slopes[j] * np.arange(n)
                p = np.exp(s - s.max())
                ref = (p @ V[j]) / p.sum()
                slack = 2.0 ** -14 * np.abs(V[j]).max() + 1e-7
                over = (np.abs(ctx[b, j] - ref) - 0.5 * bf16_ulp(ref)) / slack
                worst = max(worst, float(over.max()))
                assert over.max() <= 1.0, f"{check}: step {step} row {b} head {j} dim {int(over.argmax())}"
    st.close()
    if check is not None:
        print(f"{check}: worst (error - half ulp) / slack {worst:.3f}")
        record_error(check + " [prefix attention exact: worst (error - half ulp) / slack]", np.array([worst]),
                     np.array([0.0]), 1.0, "attention exact")
    return outs


def ragged(B):
    return [(7 * b) % 13 for b in range(B)]  # row 0: the new token alone


@pytest.mark.parametrize("hd,B,P,tails", [(64, 2, 65, [0, 5]), (80, 2, 65, [0, 5]), (96, 2, 65, [0, 5]), (128, 2, 65, [0, 5]),
                                          (64, 16, 65, ragged(16)), (64, 17, 65, ragged(17)), (64, 32, 65, ragged(32)),
                                          (64, 3, 1, [0, 62, 9]), (64, 3, 63, [0, 62, 9]), (64, 3, 64, [0, 62, 9]),
                                          (128, 3, 700, [0, 62, 9])])
def test_context_element_by_element(hd, B, P, tails):
    shared_steps(hd, B, P, tails, check=f"hd={hd} B={B} P={P}")


def test_own_prefix_is_not_read():
    a = shared_steps(96, 17, 130, ragged(17))
    b = shared_steps(96, 17, 130, ragged(17), overwrite=True)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


DEV = torch.device("cuda", 0)
B3, P3, V3 = 3, 70, 512


def tiny(**kw):
    kw.setdefault("dtype", "bf16")
    return Stage(256, 4, 2, V3, 0, 2, max_batch=B3 + 1, max_ctx=CTX, max_tokens=128, seed=9, **kw)


def warm(st, declare):
    """Template row B3 with P3 tokens forked into rows [0, B3), tails of 1, 2 and 3 tokens; returns the rows' lengths."""
    rng = np.random.default_rng(3)
    st.forward_host(rng.integers(0, V3, (1, P3)), 1, P3, slot=B3, past_len=[0])
    st.fork_kv(B3, 0, npos=P3, count=B3)
    for b in range(B3):
        st.forward_host(rng.integers(0, V3, (1, b + 1)), 1, b + 1, slot=b, past_len=[P3])
    if declare:
        st.set_row_prefix(0, B3, P3, count=B3)
    return [P3 + b + 1 for b in range(B3)]


def greedy(declare, graphs=True, steps=16):
    st = tiny()
    st.set_graphs(graphs)
    pasts = warm(st, declare)
    ids = torch.tensor([[5], [6], [7]], dtype=torch.int32, device=DEV)
    out = torch.empty(B3, dtype=torch.int32, device=DEV)
    lg = torch.empty(B3, V3, dtype=torch.float32, device=DEV)
    all_ids, all_lg = [], []
    for t in range(steps):
        st.forward(ids, out, B3, 1, slot=0, past_len=[p + t for p in pasts], logits=lg)
        torch.cuda.synchronize()
        all_ids.append(out.cpu().numpy().copy())
        all_lg.append(lg.cpu().numpy().copy())
        ids.copy_(out.view(B3, 1))
    st.close()
    return np.stack(all_ids), np.stack(all_lg)


def test_agrees_with_the_plain_route_and_is_deterministic():
    ids0, lg0 = greedy(False)
    ids1, lg1 = greedy(True)
    assert np.array_equal(ids0, ids1)
    assert not np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32)), "the shared route did not run"
    record_error("shared vs plain route [logits, 16 greedy steps]", lg1, lg0, BF16_TOL, "prefix attention")
    assert np.abs(lg1 - lg0).max() <= BF16_TOL
    for what, (ids2, lg2) in (("eager", greedy(True, graphs=False)), ("second run", greedy(True))):
        assert np.array_equal(ids1, ids2) and np.array_equal(lg1.view(np.uint32), lg2.view(np.uint32)), what


def test_fallbacks_and_statuses():
    plain, st = tiny(), tiny()
    pasts = warm(plain, False)
    ws0 = st.info()["workspace_bytes"]
    warm(st, True)
    ws1 = st.info()["workspace_bytes"]
    st.set_row_prefix(2, B3, P3 - 8)  # row 2 now differs from rows 0 and 1
    assert ws1 > ws0 and st.info()["workspace_bytes"] == ws1
    rng = np.random.default_rng(4)
    for B, S in ((B3, 1), (1, 1), (B3, 2)):  # differing declarations, one row, seq > 1
        x = rng.integers(0, V3, (B, S))
        want = plain.forward_host(x, B, S, slot=0, past_len=pasts[:B], want_logits=True)[1]
        got = st.forward_host(x, B, S, slot=0, past_len=pasts[:B], want_logits=True)[1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, S)
        pasts = [p + S if b < B else p for b, p in enumerate(pasts)]
    with pytest.raises(BloomStageError, match="error -1"):
        st.forward_host(np.zeros((B3, 1)), B3, 1, slot=0, past_len=[P3 - 9] * B3)
    for slot in (-1, B3 + 1):
        assert lib().bs_set_row_prefix(st._h, slot, 1, 0, 4, None) == -1
    assert lib().bs_set_row_prefix(st._h, 0, 1, B3 + 1, 4, None) == -1
    assert lib().bs_set_row_prefix(st._h, 0, 1, 0, CTX + 1, None) == -1
    st.reset(0)
    st.reset(1)
    st.forward_host(np.zeros((2, 1)), 2, 1, slot=0, past_len=[0, 0])  # below the old npos: the declaration is gone
    for kw in ({"dtype": "fp32"}, {"kv_int8": True}):
        other = tiny(**kw)
        assert lib().bs_set_row_prefix(other._h, 0, 2, 0, 4, None) == -5
        other.close()
    plain.close()
    st.close()
