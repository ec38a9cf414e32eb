"""The tree verify attention (bs_forward_tree, csrc/attn_tree.hip) element by element.

Method and bound of tests/test_gpu_attention_exact.py (identity-weight stage, float64 reference on the device's own
cache, half a bf16 ulp + 2^-14 max|V| + 1e-7) with the ancestor-or-self mask and the ALiBi position past + depth of a
node key.  Nothing at or beyond past + N is written, two runs agree bit for bit, and junk a rolled-back row holds
beyond past + N does not move a bit."""
import numpy as np
import pytest

from test_gpu_attention_exact import AttnStage, bf16_ulp
from test_gpu_parity import record_error

pytestmark = pytest.mark.gpu


def _x(rng, B, S, h):
    return (0.01 * rng.standard_normal((B, S, h))).astype(np.float32)


def _trees(kind, B, N, rng):
    one = {"star": [-1] + [0] * (N - 1), "chain": list(range(-1, N - 1)), "binary": [-1] + [(i - 1) // 2 for i in range(1, N)]}
    if kind in one:
        return np.array([one[kind]] * B, np.int32)
    return np.array([[-1] + [int(rng.integers(0, i)) for i in range(1, N)] for _ in range(B)], np.int32)


def _reference(a, K, V, past, par):
    """float64 context [N][nh][hd] of one row from its cache K, V [nh][past + N][hd]."""
    N, n = len(par), past + len(par)
    vis = np.zeros((N, N), bool)
    depth = np.zeros(N, np.int64)
    for i in range(N):
        vis[i, i] = True
        if i:
            vis[i] |= vis[par[i]]
            depth[i] = depth[par[i]] + 1
    live = np.concatenate([np.ones((N, past), bool), vis], axis=1)
    apos = np.concatenate([np.arange(past), past + depth]).astype(np.float64)
    ref = np.empty((N, a.nh, a.hd))
    for j in range(a.nh):
        q = K[(j - 1) % a.nh, past:n]
        s = np.where(live, a.inv_norm * (q @ K[j].T) + a.slopes[j] * apos[None, :], -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        ref[:, j] = (p @ V[j]) / p.sum(axis=1, keepdims=True)
    return ref


def _run(nh, hd, B, N, pasts, max_ctx, kind, poison):
    h = nh * hd
    a = AttnStage(h, nh, B, max_ctx, max(max(pasts), 32))
    rng = np.random.default_rng(200 + hd + N)
    for r, n in enumerate(pasts):
        if n:
            a.st.forward_host(_x(rng, 1, n, h), 1, n, slot=r, past_len=[0])
    par = _trees(kind, B, N, rng)
    x = _x(rng, B, N, h)
    if poison:  # a longer earlier pass leaves NaN K / V at past + N .. (0 * NaN would show), then the row is rolled back
        junk = min(40, max_ctx - pasts[0])
        a.st.forward_host(np.full((1, junk, h), np.nan, np.float32), 1, junk, slot=0, past_len=[pasts[0]])
        a.st.rollback(0, pasts[0])
    tails = [a.st.read_kv(0, b, pasts[b] + N, max_ctx - pasts[b] - N) for b in range(B) if pasts[b] + N < max_ctx]
    assert not poison or np.isnan(tails[0][:, :, 0]).all(), "the poison did not land at past + N"
    out = a.st.forward_tree_host(x, par, slot=0, past_len=list(pasts))
    again = a.st.forward_tree_host(x, par, slot=0, past_len=list(pasts))
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)), "two runs differ"
    after = [a.st.read_kv(0, b, pasts[b] + N, max_ctx - pasts[b] - N) for b in range(B) if pasts[b] + N < max_ctx]
    assert all(np.array_equal(t.view(np.uint32), u.view(np.uint32)) for t, u in zip(tails, after)), "wrote beyond past + N"
    return a, x, par, out


@pytest.mark.parametrize("nh,hd,B,N,pasts,max_ctx,kind", [
    (4, 64, 1, 2, (0,), 64, "chain"),                  # root + one child: the smallest pass
    (4, 64, 1, 16, (0,), 64, "star"),                  # every node sees only itself and the root
    (4, 64, 1, 16, (0,), 64, "chain"),                 # the causal limit
    (4, 64, 1, 16, (57,), 128, "binary"),              # the nodes straddle a chunk edge; siblings must not see each other
    (4, 96, 3, 5, (0, 130, 449), 512, "random"),       # ticket merge; a split with no chunk
    (16, 128, 1, 16, (1000,), 1024, "random"),         # many splits
    (4, 80, 1, 3, (70,), 128, "star"),                 # head_dim padding
    # 192 (row, head) pairs: one split, a wave walks up to 4 chunks with the nodes in its last one (prefetch, both
    # ring stages, the rescale of a finite state); then 128 pairs over 48 chunks: 4 splits, up to 3 chunks per wave
    (12, 64, 16, 2, (1000, 997, 960, 900, 833, 770, 705, 641, 640, 639, 577, 500, 400, 257, 130, 0), 1024, "chain"),
    (8, 64, 16, 2, (3060, 2500, 1100, 130) + (0,) * 12, 3072, "chain"),
])
def test_tree_attention_exact(nh, hd, B, N, pasts, max_ctx, kind):
    what = f"tree {kind} {nh}x{hd} B={B} N={N} past={pasts}"
    a, x, par, out = _run(nh, hd, B, N, pasts, max_ctx, kind, False)
    ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(B, N, nh, hd)
    worst = 0.0
    for b in range(B):
        kv = a.st.read_kv(0, b, 0, pasts[b] + N).astype(np.float64)
        K, V = kv[0], kv[1]
        assert np.array_equal(V, np.roll(K, -1, axis=0)), f"{what}: V_j != K_(j+1) in row {b}"
        ref = _reference(a, K, V, pasts[b], par[b])
        slack = 2.0 ** -14 * np.abs(V).max(axis=(1, 2))[None, :, None] + 1e-7
        over = (np.abs(ctx[b] - ref) - 0.5 * bf16_ulp(ref)) / slack
        worst = max(worst, float(over.max()))
        bad = np.argwhere(over > 1.0)
        assert bad.size == 0, (f"{what}: row {b} node {bad[0][0]} head {bad[0][1]} dim {bad[0][2]}: "
                               f"{ctx[b][tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    record_error(what + " [tree attention exact: worst (error - half ulp) / slack]", np.array([worst]), np.array([0.0]),
                 1.0, "attention exact")
    print(f"{what}: worst (error - half ulp) / slack {worst:.3f}")
    if kind == "binary":  # the same pass over a row whose positions past + N .. hold a rolled-back pass's junk
        poisoned = _run(nh, hd, B, N, pasts, max_ctx, kind, True)[3]
        assert np.array_equal(out.view(np.uint32), poisoned.view(np.uint32)), f"{what}: junk beyond past + N reached a result"
