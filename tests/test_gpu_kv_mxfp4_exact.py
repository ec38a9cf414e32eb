"""The MXFP4 KV cache (BS_FLAG_MXFP4_KV) pinned element by element, by the method of test_gpu_kv_int8_exact.py: a
bf16-KV twin and the MXFP4 stage (one layer, identity weights) run the same inputs call for call.  After every call:
  (a) read_kv of the MXFP4 stage over the written positions == mxfp4_np.roundtrip(twin read_kv) along head_dim
      (np.array_equal: the sign of a zero code is unspecified); nothing at or beyond them is non-zero;
  (b) every context element against float64 attention over the dequantised cache (positions < past_b) and the twin's
      bf16 values (the call's own positions), for seq == 1 and seq > 1 alike: a dequantised value is exact in bf16.
      Bound, unchanged: half a bf16 ulp of the reference + 2^-14 max|V| + 1e-7.
Shapes: the smallest that reach each decode grid with 16 heads.  The kernel takes the new token from the staging row
and walks chunks of cached positions only (64 under the 8-wave split grid, else 128), so a step opens a new chunk when
past_b reaches 64k + 1 / 128k + 1.  In a cache of past + 1 positions that step is also the one that fills the last
position, which prompt 700 in 705 positions cannot be (704 = 64 * 11): that case stays, beside ones that do both.
"""
import numpy as np
import pytest

import mxfp4_np
from distributed_inference_demo_amd.stage import Stage
from oracle.oracle import alibi_slopes

from test_gpu_attention_exact import _x, bf16_ulp, identity_attention_weights
from test_gpu_parity import record_error

pytestmark = pytest.mark.gpu

NH = 16


class TwinPair:
    def __init__(self, hd, max_batch, max_ctx, max_tokens):
        self.h, self.hd, self.max_ctx = NH * hd, hd, max_ctx
        kw = dict(dtype="bf16", max_batch=max_batch, max_ctx=max_ctx, max_tokens=max_tokens,
                  host_weights=identity_attention_weights(self.h, NH), is_first=False, is_last=False)
        self.twin = Stage(self.h, NH, 1, 512, 0, 1, **kw)
        self.fp4 = Stage(self.h, NH, 1, 512, 0, 1, kv_mxfp4=True, **kw)
        self.slopes = alibi_slopes(NH).astype(np.float64)
        self.inv_norm = float(np.float32(1.0) / np.sqrt(np.float32(hd)))

    def close(self):
        self.twin.close()
        self.fp4.close()

    def run_and_check(self, x, B, S, slot, pasts, what):
        self.twin.forward_host(x, B, S, slot=slot, past_len=list(pasts))
        out = self.fp4.forward_host(x, B, S, slot=slot, past_len=list(pasts))
        assert np.isfinite(out).all(), f"{what}: non-finite output"
        ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(B, S, NH, self.hd)
        worst = 0.0
        for b in range(B):
            past, n = pasts[b], pasts[b] + S
            kv_t = self.twin.read_kv(0, slot + b, 0, n)  # [2][nh][n][hd], the exact bf16 K / V
            kv_q = self.fp4.read_kv(0, slot + b, 0, self.max_ctx)
            assert np.array_equal(kv_q[:, :, :n], mxfp4_np.roundtrip(kv_t)), f"{what}: row {b}: cache != MXFP4(twin)"
            assert not kv_q[:, :, n:].any(), f"{what}: row {b}: something written at or beyond position {n}"
            eff = np.concatenate([kv_q[:, :, :past], kv_t[:, :, past:]], axis=2).astype(np.float64)
            K, V = eff[0], eff[1]
            Kt = kv_t[0].astype(np.float64)
            for j in range(NH):
                q = Kt[(j - 1) % NH, past:n]  # [S][hd]: q_j = K_(j-1) at the query's position
                s = self.inv_norm * (q @ K[j].T) + self.slopes[j] * np.arange(n)[None, :]
                s[np.arange(n)[None, :] > (past + np.arange(S))[:, None]] = -np.inf
                p = np.exp(s - s.max(axis=1, keepdims=True))
                r = (p @ V[j]) / p.sum(axis=1, keepdims=True)
                got = ctx[b, :, j, :]
                slack = 2.0 ** -14 * np.abs(V[j]).max() + 1e-7
                over = (np.abs(got - r) - 0.5 * bf16_ulp(r)) / slack
                worst = max(worst, float(over.max()))
                bad = np.argwhere(over > 1.0)
                assert bad.size == 0, (f"{what}: row {b} head {j} query {bad[0][0]} dim {bad[0][1]}: "
                                       f"{got[tuple(bad[0])]} vs {r[tuple(bad[0])]} (over / slack {over.max():.2f})")
        record_error(what + " [MXFP4 KV exact: worst (error - half ulp) / slack]", np.array([worst]), np.array([0.0]),
                     1.0, "attention exact")


# (name, hd, prompts per row (one prefill call each when they differ), decode steps, max_ctx)
DECODE = [
    ("deferred merge, last cache position", 96, [700], 5, 705),
    ("deferred merge, chunk 11 opened at past 705, last cache position", 96, [701], 5, 706),
    ("ticket merge", 96, [700, 663, 626], 5, 705),
    ("ticket merge, chunks opened at past 769 / 641, last cache position", 96, [765, 640, 637], 5, 770),
    ("unsplit 8-wave hd 64, chunk 1 opened at past 129", 64, [126, 126], 4, 130),
    ("unsplit 8-wave hd 64", 64, [62, 62], 4, 66),
    ("unsplit 8-wave hd 96", 96, [62, 62], 4, 66),
    ("unsplit 8-wave hd 128", 128, [62, 62], 4, 66),
    ("4-wave blocks", 64, [40] * 17, 2, 42),
]


@pytest.mark.parametrize("what,hd,pasts,steps,max_ctx", DECODE, ids=[c[0] for c in DECODE])
def test_decode_grids(what, hd, pasts, steps, max_ctx):
    B = len(pasts)
    a = TwinPair(hd, B, max_ctx, max(B * min(pasts), max(pasts)))
    rng = np.random.default_rng(31 + hd + B)
    if len(set(pasts)) == 1:
        a.run_and_check(_x(rng, B, pasts[0], a.h), B, pasts[0], 0, [0] * B, f"{what}: prompt")
    else:
        for r, n in enumerate(pasts):
            a.run_and_check(_x(rng, 1, n, a.h), 1, n, r, [0], f"{what}: row {r} prompt {n}")
    for step in range(steps):
        a.run_and_check(_x(rng, B, 1, a.h), B, 1, 0, [p + step for p in pasts], f"{what}: decode step {step}")
    a.close()


def test_continuation_prefill_and_decode_see_the_same_past():
    """70 new tokens on rows holding 130 / 450 positions (bf16 staging copy), then a decode step (codes): one past."""
    a = TwinPair(96, 3, 600, 2 * 520)  # staging: both rows laid out at the longer one's 450 + 70 positions
    rng = np.random.default_rng(35)
    for r, n in enumerate((130, 450)):
        a.run_and_check(_x(rng, 1, n, a.h), 1, n, 1 + r, [0], f"prompt {n}")
    a.run_and_check(_x(rng, 2, 70, a.h), 2, 70, 1, [130, 450], "continuation 70 after 130 / 450")
    a.run_and_check(_x(rng, 2, 1, a.h), 2, 1, 1, [200, 520], "decode after the continuation")
    a.close()
