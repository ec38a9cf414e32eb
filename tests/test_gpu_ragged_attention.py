"""The ragged prefill attention (bs_forward_ragged, csrc/attn_ragged.hip) element by element.

Method and bound of tests/test_gpu_attention_exact.py: on the identity-weight one-layer stage out - x is the context,
q_j = K_(j-1) and V_j = K_(j+1) bit for bit, so the attention's exact inputs are read back from the cache the pass
itself wrote (the in-launch copy from staging) and every context element is held to half a bf16 ulp of a float64
reference plus 2^-14 max|V| + 1e-7.  The rows' pasts are laid down by ordinary bs_forward passes.
"""
import numpy as np
import pytest

from test_gpu_attention_exact import AttnStage, _x, bf16_ulp
from test_gpu_parity import record_error

pytestmark = pytest.mark.gpu

CASES = [
    (4, 64, [(0, 1, 0), (1, 5, 0)], 64),                     # the mask alone; a one-token row from an empty cache
    (4, 96, [(2, 70, 0), (0, 3, 61), (1, 64, 64)], 256),     # a second query tile; new positions across a key-tile
                                                             # edge; a past that is a whole tile; slots out of order
    (16, 128, [(0, 130, 449), (1, 17, 0)], 1024),            # many past tiles next to a short fresh row
    (4, 80, [(0, 33, 70)], 128),                             # head_dim padding
    (4, 64, [(i, 2, i) for i in range(32)], 64),             # a long work list of tiny tiles
]


@pytest.mark.parametrize("nh,hd,rows,max_ctx", CASES)
def test_ragged_attention_exact(nh, hd, rows, max_ctx):
    h = nh * hd
    T = sum(S for _, S, _ in rows)
    nslot = max(r for r, _, _ in rows) + 2  # one more row than used: it must stay untouched
    a = AttnStage(h, nh, nslot, max_ctx, max(T, max(p for _, _, p in rows), 32))
    rng = np.random.default_rng(200 + hd + len(rows))
    for slot, _, past in rows:
        if past:
            a.run_and_check(_x(rng, 1, past, h), 1, past, slot, [0], f"prompt {past}")
    x = _x(rng, 1, T, h)[0]
    slots, lens, pasts = zip(*rows)
    out = a.st.forward_ragged_host(x, slots, lens, pasts)
    again = a.st.forward_ragged_host(x, slots, lens, pasts)  # rewrites the same cache positions with the same bits
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)), "two runs differ"
    ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(T, nh, hd)
    what = f"ragged {nh}x{hd} rows={rows if len(rows) < 5 else len(rows)}"
    worst, t0 = 0.0, 0
    for slot, S, past in rows:
        n = past + S
        kv = a.st.read_kv(0, slot, 0, max_ctx).astype(np.float64)
        assert not kv[:, :, n:].any(), f"{what}: row {slot} written at or beyond {n}"
        K, V = kv[0, :, :n], kv[1, :, :n]
        assert np.array_equal(V, np.roll(K, -1, axis=0)), f"{what}: V_j != K_(j+1) in row {slot}"
        for j in range(nh):
            q = K[(j - 1) % nh, past:n]  # the new tokens' q, as the cache write reproduced it
            s = a.inv_norm * (q @ K[j].T) + a.slopes[j] * np.arange(n)[None, :]
            s[np.arange(n)[None, :] > (past + np.arange(S))[:, None]] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            ref = (p @ V[j]) / p.sum(axis=1, keepdims=True)
            got = ctx[t0:t0 + S, j, :]
            slack = 2.0 ** -14 * np.abs(V[j]).max() + 1e-7
            over = (np.abs(got - ref) - 0.5 * bf16_ulp(ref)) / slack
            worst = max(worst, float(over.max()))
            bad = np.argwhere(over > 1.0)
            assert bad.size == 0, (f"{what}: row {slot} head {j} query {bad[0][0]} dim {bad[0][1]}: "
                                   f"{got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
        t0 += S
    for slot in set(range(nslot)) - set(slots):
        assert not a.st.read_kv(0, slot, 0, max_ctx).any(), f"{what}: unused row {slot} was written"
    record_error(what + " [ragged attention exact: worst (error - half ulp) / slack]", np.array([worst]),
                 np.array([0.0]), 1.0, "attention exact")
    print(f"{what}: worst (error - half ulp) / slack {worst:.3f}")
