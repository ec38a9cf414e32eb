"""The int8 KV cache (BS_FLAG_INT8_KV) pinned element by element, on the identity-weight scheme of
test_gpu_attention_exact.py.

Two one-layer middle stages get the same host weights and the same inputs, call for call: a bf16-KV twin and an
int8-KV stage.  Both run the same deterministic LN + QKV kernels, so the twin's cache holds the exact bf16 K / V the
int8 stage's epilogue produced (and q_j = K_(j-1) at the query's position).  After every call:

  (a) cache bits: read_kv of the int8 stage over the positions written so far == quantise -> dequantise
      (tests/kv_int8_ref.py) of the twin's read_kv, bit for bit;
  (b) context: every element of out - x against float64 attention whose K / V are the int8 stage's dequantised cache
      for positions < past_b and the twin's bf16 values for the call's own positions.  A call with seq > 1 reads its
      past through the bf16 staging copy (bloomstage.h), so there the past is bf16(dequantised); seq == 1 applies the
      fp32 scales to the codes, so there it is the fp32 dequantised value.  Bound: the bf16 file's, unchanged -- half
      a bf16 ulp of the reference + 2^-14 max|V| + 1e-7 (codes times an fp32 scale add only fp32 rounding).

Shapes are the smallest that reach each decode grid (attention_decode_splits) with 16 heads: split context with the
deferred merge (B = 1) and the ticket merge (B = 3), unsplit 8-wave (B = 2, every head_dim) and 4-wave (B = 17) blocks,
a new 64-position chunk opened by a decode step, the last cache position, and prefill continuations.
"""
import numpy as np
import pytest

import kv_int8_ref as ref
from distributed_inference_demo_amd.stage import BS_FLAG_INT8_KV, BloomStageError, Stage
from oracle.oracle import alibi_slopes

from test_gpu_attention_exact import _x, bf16_ulp, identity_attention_weights
from test_gpu_parity import record_error

pytestmark = pytest.mark.gpu


class TwinPair:
    def __init__(self, h, nh, max_batch, max_ctx, max_tokens, weights=None):
        self.h, self.nh, self.hd = h, nh, h // nh
        w = identity_attention_weights(h, nh) if weights is None else weights
        kw = dict(dtype="bf16", max_batch=max_batch, max_ctx=max_ctx, max_tokens=max_tokens, host_weights=w,
                  is_first=False, is_last=False)
        self.twin = Stage(h, nh, 1, 512, 0, 1, **kw)
        self.q8 = Stage(h, nh, 1, 512, 0, 1, kv_int8=True, **kw)
        self.slopes = alibi_slopes(nh).astype(np.float64)
        self.inv_norm = float(np.float32(1.0) / np.sqrt(np.float32(self.hd)))

    def close(self):
        self.twin.close()
        self.q8.close()

    def run_and_check(self, x, B, S, slot, pasts, what):
        self.twin.forward_host(x, B, S, slot=slot, past_len=list(pasts))
        out = self.q8.forward_host(x, B, S, slot=slot, past_len=list(pasts))
        assert np.isfinite(out).all(), f"{what}: non-finite output"
        ctx = (out.astype(np.float64) - x.astype(np.float64)).reshape(B, S, self.nh, self.hd)
        worst = 0.0
        for b in range(B):
            past, n = pasts[b], pasts[b] + S
            kv_t = self.twin.read_kv(0, slot + b, 0, n)   # [2][nh][n][hd], the exact bf16 K / V
            kv_q = self.q8.read_kv(0, slot + b, 0, n)
            want = ref.roundtrip(kv_t)
            assert np.array_equal(kv_q, want), \
                f"{what}: row {b}: int8 cache != quantise(twin cache) at {np.argwhere(kv_q != want)[0]}"
            seen = kv_q[:, :, :past] if S == 1 else ref.to_bf16(kv_q[:, :, :past])  # how this call read its past
            eff = np.concatenate([seen, kv_t[:, :, past:]], axis=2).astype(np.float64)
            K, V = eff[0], eff[1]
            Kt = kv_t[0].astype(np.float64)
            for j in range(self.nh):
                q = Kt[(j - 1) % self.nh, past:n]                          # [S][hd]
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
        record_error(what + " [int8 KV exact: worst (error - half ulp) / slack]", np.array([worst]), np.array([0.0]),
                     1.0, "attention exact")
        print(f"{what}: worst (error - half ulp) / slack {worst:.3f}")
        return out


def _prompts_then_steps(a, rng, pasts, steps, what):
    B = len(pasts)
    for r in range(B):
        a.run_and_check(_x(rng, 1, pasts[r], a.h), 1, pasts[r], r, [0], f"{what} row {r} prompt {pasts[r]}")
    for step in range(steps):
        a.run_and_check(_x(rng, B, 1, a.h), B, 1, 0, [p + step for p in pasts], f"{what} decode step {step}")


def test_decode_split_context_deferred_merge_fills_the_cache():
    """B = 1, hd 96, 700-token prompt, 5 steps in a 705-position cache: the context splits over blocks and the dense
    GEMV merges; step 4 opens a new 64-position chunk at 704 and fills the last cache position."""
    nh, hd, P = 16, 96, 700
    a = TwinPair(nh * hd, nh, 1, P + 5, P)
    _prompts_then_steps(a, np.random.default_rng(21), [P], 5, "deferred merge")
    a.close()


def test_decode_split_context_ticket_merge():
    """B = 3 (above the deferral limit) at 700 / 663 / 626 cached positions: the last split block merges by ticket."""
    nh, hd = 16, 96
    pasts = [700, 663, 626]
    a = TwinPair(nh * hd, nh, 3, 705, 700)
    _prompts_then_steps(a, np.random.default_rng(22), pasts, 5, "ticket merge")
    a.close()


@pytest.mark.parametrize("hd", [64, 80, 96, 128])
def test_decode_unsplit_8_wave_across_the_chunk_boundary(hd):
    """B = 2, prompt 62, 4 steps (contexts 63..66, across the 64-position chunk), max_ctx = 66: one 8-wave block per
    (row, head); hd 64 / 80 / 96 mask the lanes past head_dim."""
    nh, B, P = 16, 2, 62
    a = TwinPair(nh * hd, nh, B, P + 4, B * P)
    rng = np.random.default_rng(23 + hd)
    a.run_and_check(_x(rng, B, P, a.h), B, P, 0, [0] * B, f"hd={hd} prompt")
    for step in range(4):
        a.run_and_check(_x(rng, B, 1, a.h), B, 1, 0, [P + step] * B, f"hd={hd} decode step {step}")
    a.close()


def test_decode_unsplit_4_wave_many_pairs():
    """B = 17, hd 64: 272 (row, head) pairs > 256 -> 4-wave blocks."""
    nh, hd, B, P = 16, 64, 17, 40
    a = TwinPair(nh * hd, nh, B, P + 2, B * P)
    rng = np.random.default_rng(24)
    a.run_and_check(_x(rng, B, P, a.h), B, P, 0, [0] * B, "B=17 prompt")
    for step in range(2):
        a.run_and_check(_x(rng, B, 1, a.h), B, 1, 0, [P + step] * B, f"B=17 decode step {step}")
    a.close()


def test_prefill_continuations_dequantise_the_past():
    """Rows at slots 1 and 2 hold 130 and 450 positions, then 200 new tokens each (hd 96): the past goes through the
    bf16 staging copy, the new positions are quantised into the cache."""
    nh, hd = 16, 96
    h = nh * hd
    a = TwinPair(h, nh, 3, 1024, 2 * 650)  # staging: both rows laid out at the longer one's 450 + 200 positions
    rng = np.random.default_rng(25)
    for r, n in enumerate((130, 450)):
        a.run_and_check(_x(rng, 1, n, h), 1, n, 1 + r, [0], f"prompt {n}")
    a.run_and_check(_x(rng, 2, 200, h), 2, 200, 1, [130, 450], "continuation 200 after 130 / 450")
    a.close()


def test_prefill_one_row_continuation_after_700():
    nh, hd = 16, 128
    h = nh * hd
    a = TwinPair(h, nh, 1, 708, 700)
    rng = np.random.default_rng(26)
    a.run_and_check(_x(rng, 1, 700, h), 1, 700, 0, [0], "prompt 700")
    a.run_and_check(_x(rng, 1, 8, h), 1, 8, 0, [700], "continuation 8 after 700")
    a.close()


def test_prefill_over_staging_capacity_is_an_error_not_a_fault():
    """cap = max(max_tokens, max_ctx) = 128 positions; 2 rows x (100 cached + 10 new) = 220 > 128: refused on the
    host, before any launch, and the stage keeps working."""
    nh, hd = 16, 64
    h = nh * hd
    st = Stage(h, nh, 1, 512, 0, 1, dtype="bf16", max_batch=2, max_ctx=128, max_tokens=100, kv_int8=True,
               host_weights=identity_attention_weights(h, nh), is_first=False, is_last=False)
    rng = np.random.default_rng(27)
    for r in range(2):
        st.forward_host(_x(rng, 1, 100, h), 1, 100, slot=r, past_len=0)
    with pytest.raises(BloomStageError) as ei:
        st.forward_host(_x(rng, 2, 10, h), 2, 10, slot=0, past_len=[100, 100])
    assert "-5" in str(ei.value) and "220" in str(ei.value) and "128" in str(ei.value)
    out = st.forward_host(_x(rng, 1, 10, h), 1, 10, slot=0, past_len=[100])  # one row always fits
    assert np.isfinite(out).all()
    st.close()


def test_all_zero_vectors():
    """QKV weight and bias zero: every K / V vector is zero (scale 1, codes 0), the context is exactly 0."""
    nh, hd, B, P = 16, 64, 2, 20
    h = nh * hd
    w = identity_attention_weights(h, nh)
    w[2 * h:2 * h + 3 * h * h] = 0.0  # the fused QKV weight (after ln1 gamma, beta); its bias is already zero
    st = Stage(h, nh, 1, 512, 0, 1, dtype="bf16", max_batch=B, max_ctx=P + 3, max_tokens=B * P, kv_int8=True,
               host_weights=w, is_first=False, is_last=False)
    rng = np.random.default_rng(28)
    x = _x(rng, B, P, h)
    assert np.array_equal(st.forward_host(x, B, P, past_len=0), x)
    for step in range(3):
        x = _x(rng, B, 1, h)
        out = st.forward_host(x, B, 1, past_len=P + step)
        assert np.isfinite(out).all() and np.array_equal(out, x)
    for b in range(B):
        kv = st.read_kv(0, b, 0, P + 3)
        assert np.isfinite(kv).all() and not kv.any()
    st.close()


def test_slot_reuse_after_reset_gives_the_same_bits():
    nh, hd, P = 16, 64, 70
    h = nh * hd
    st = Stage(h, nh, 1, 512, 0, 1, dtype="bf16", max_batch=2, max_ctx=P + 3, max_tokens=P, kv_int8=True,
               host_weights=identity_attention_weights(h, nh), is_first=False, is_last=False)
    rng = np.random.default_rng(29)
    st.forward_host(_x(rng, 1, P, h), 1, P, slot=0, past_len=0)   # use row 0, up to its last positions
    for step in range(3):
        st.forward_host(_x(rng, 1, 1, h), 1, 1, slot=0, past_len=P + step)
    st.reset(0)
    assert not st.read_kv(0, 0, 0, P + 3).any()
    xs = [_x(rng, 1, 33, h)] + [_x(rng, 1, 1, h) for _ in range(3)]
    outs = []
    for slot in (0, 1):  # the reused row, then a never-used one
        o = [st.forward_host(xs[0], 1, 33, slot=slot, past_len=0)]
        o += [st.forward_host(xs[1 + i], 1, 1, slot=slot, past_len=33 + i) for i in range(3)]
        outs.append(o)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.array_equal(st.read_kv(0, 0, 0, P + 3), st.read_kv(0, 1, 0, P + 3))
    st.close()


def test_stage_info_sizes():
    nh, hd, B, C = 16, 80, 3, 77
    st = Stage(nh * hd, nh, 2, 512, 0, 2, dtype="bf16", max_batch=B, max_ctx=C, max_tokens=40, kv_int8=True,
               is_first=False, is_last=False)
    tw = Stage(nh * hd, nh, 2, 512, 0, 2, dtype="bf16", max_batch=B, max_ctx=C, max_tokens=40, is_first=False,
               is_last=False)
    assert st.kv_int8 and not tw.kv_int8 and st.desc.flags & BS_FLAG_INT8_KV
    assert st.info()["kv_bytes"] == ref.kv_bytes(2, B, nh, C, hd) == 2 * 2 * B * nh * C * (hd + 4)
    # the two bf16 staging buffers (cap = max(max_tokens, max_ctx) positions) count as workspace
    assert st.info()["workspace_bytes"] - tw.info()["workspace_bytes"] == 2 * max(40, C) * nh * hd * 2
    st.close()
    tw.close()


def test_int8_kv_with_a_head_slice_builds():
    """A middle stage that also owns a vocabulary slice: the slice owns no cache beyond the stage's layers."""
    nh, hd = 4, 16
    st = Stage(nh * hd, nh, 4, 512, 1, 3, dtype="bf16", max_batch=2, max_ctx=16, kv_int8=True, head_slice=(128, 256))
    assert st.info()["kv_bytes"] == ref.kv_bytes(2, 2, nh, 16, hd)
    st.close()


def test_fp32_stage_rejects_the_flag():
    with pytest.raises(BloomStageError) as ei:
        Stage(64, 4, 1, 512, 0, 1, dtype="fp32", kv_int8=True)
    assert "bloomstage error -1" in str(ei.value) and "BS_FLAG_INT8_KV" in str(ei.value)
