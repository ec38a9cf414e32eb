"""Whole decoder blocks with the MXFP4 KV cache (BS_FLAG_MXFP4_KV), by the method of test_gpu_kv_int8_model.py, and
the flag's statuses.  Blocks: h = 64, 2 heads (hd = 32), 4 layers, V = 512; prefill P = 24 for B = 2, then 6 decode
steps fed the reference's tokens, logits held to the existing bf16 decode bound (test_gpu_parity.check_logits).
  * bf16 weights: the reference is the CPU checker, handed the device's cache before every step.
  * mxfp4_weights=True: the checker holds no 4-bit weights, so the reference is a second device stage over the
    dequantised weights (exact in bf16), also with kv_mxfp4 and its own cache: it shows that the two flags compose
    (the decode GEMVs differ), not that the attention is right -- both sides run the same attention and cache kernels.
"""
import re

import numpy as np
import pytest

import mxfp4_np
from distributed_inference_demo_amd.stage import BS_FLAG_MXFP4_KV, BloomStageError, Stage
from oracle import gen_np
from oracle.oracle import OracleStage

from test_gpu_parity import assert_ids_match, check_logits

pytestmark = pytest.mark.gpu

H, NH, L, V = 64, 2, 4, 512
B, P, STEPS = 2, 24, 6
KW = dict(dtype="bf16", max_batch=B, max_ctx=P + STEPS, max_tokens=B * P)


@pytest.mark.parametrize("mxfp4_weights", [False, True])
def test_blocks_match_the_reference_step_for_step(mxfp4_weights):
    gs = Stage(H, NH, L, V, 0, L, seed=11, kv_mxfp4=True, mxfp4_weights=mxfp4_weights, **KW)
    if mxfp4_weights:
        ref = Stage(H, NH, L, V, 0, L, host_weights=gs.read_weights(), kv_mxfp4=True, **KW)
        ref_forward = lambda x, S, past: ref.forward_host(x, B, S, past_len=past, want_logits=True)
    else:
        ref = OracleStage(H, NH, L, V, 0, L, bf16=True, max_batch=B, max_ctx=P + STEPS, seed=11)
        ref_forward = lambda x, S, past: ref.forward(x, B, S, past_len=past, want_logits=True)
    ids = gen_np.prompt_ids(16, B, P, V).astype(np.int32)
    tg, lg = gs.forward_host(ids, B, P, past_len=0, want_logits=True)
    to, lo = ref_forward(ids, P, 0)
    check_logits(lg, lo, "bf16", "prefill (attends bf16)")
    assert_ids_match(tg, to, lo, "prefill")
    for step in range(STEPS):
        past = P + step
        for layer in range(L if not mxfp4_weights else 0):  # the checker is handed the device's cache
            for r in range(B):
                ref.write_kv(layer, r, 0, gs.read_kv(layer, r, 0, past))
        t_in = np.ascontiguousarray(to, np.int32).reshape(B, 1)
        tg, lg = gs.forward_host(t_in, B, 1, past_len=past, want_logits=True)
        to, lo = ref_forward(t_in, 1, past)
        check_logits(lg, lo, "bf16", f"decode step {step} (ctx {past + 1})")
        assert_ids_match(tg, to, lo, f"decode step {step}")
    gs.close()
    ref.close()


def _code(fn):
    with pytest.raises(BloomStageError) as ei:
        fn()
    return int(re.search(r"error (-\d+)", str(ei.value)).group(1))


@pytest.mark.parametrize("kw,code", [
    (dict(dtype="fp32", kv_mxfp4=True), -1),                              # BS_ERR_INVALID
    (dict(dtype="bf16", kv_mxfp4=True, kv_int8=True), -1),
    (dict(dtype="bf16", kv_mxfp4=True, hidden=4 * 80), -5),               # hd = 80: BS_ERR_UNSUPPORTED
], ids=["fp32", "both KV flags", "hd 80"])
def test_init_errors(kw, code):
    hidden = kw.pop("hidden", 128)
    assert _code(lambda: Stage(hidden, 4, 1, 512, 0, 1, **kw)) == code


def test_orthogonal_flags_build_and_report_kv_bytes():
    nh, hd, mb, C = 4, 96, 3, 77
    for kw in (dict(int8_weights=True), dict(mxfp4_weights=True), dict(n_labels=3)):
        st = Stage(nh * hd, nh, 2, 512, 0, 2, dtype="bf16", max_batch=mb, max_ctx=C, max_tokens=40, kv_mxfp4=True, **kw)
        assert st.kv_mxfp4 and st.desc.flags & BS_FLAG_MXFP4_KV
        assert st.info()["kv_bytes"] == 2 * 2 * mb * nh * C * (hd // 2 + hd // 32)
        st.close()


def test_refused_paths_return_the_int8_cache_codes():
    h, nh = 128, 4
    kw = dict(dtype="bf16", max_batch=4, max_ctx=40, max_tokens=64, is_first=False)
    codes = []
    for fmt in (dict(kv_int8=True), dict(kv_mxfp4=True)):
        st = Stage(h, nh, 1, 512, 0, 1, **fmt, **kw)
        x = np.zeros((2, 4, h), np.float32)
        st.forward_host(x, 2, 4, past_len=0)
        codes.append([
            _code(lambda: st.forward_host(x, 2, 4, past_len=4, verify=True)),
            _code(lambda: st.forward_host(x, 2, 4, past_len=4, verify=True, draw=True)),
            _code(lambda: st.forward_tree_host(x, [[-1, 0, 0, 1]] * 2, past_len=4)),
            _code(lambda: st.compact_kv(0, 2, [1])),
            _code(lambda: st.forward_ragged_host(x.reshape(8, h), [0, 1], [4, 4], [4, 4])),
            _code(lambda: st.set_row_prefix(1, 0, 4)),
        ])
        st.close()
    assert codes[0] == codes[1] and all(c < 0 for c in codes[1])


def test_fork_and_copy_reproduce_a_row_bit_for_bit():
    """hd = 96 and an odd max_ctx: 3 scale bytes per position, segments that start on odd addresses."""
    h, nh, C, n = 4 * 96, 4, 37, 21
    st = Stage(h, nh, 2, 512, 0, 2, dtype="bf16", max_batch=5, max_ctx=C, max_tokens=n, kv_mxfp4=True, is_first=False)
    st.forward_host(np.random.default_rng(3).standard_normal((1, n, h)).astype(np.float32), 1, n, slot=1, past_len=0)
    st.fork_kv(1, 2, npos=n - 2, count=2)
    st.copy_kv([(1, 0), (1, 4)], n)
    for layer in range(2):
        src = st.read_kv(layer, 1, 0, C)
        assert src[:, :, :n].any() and np.array_equal(src, mxfp4_np.roundtrip(src))
        for dst, npos in ((2, n - 2), (3, n - 2), (0, n), (4, n)):
            got = st.read_kv(layer, dst, 0, C)
            assert np.array_equal(got[:, :, :npos].view(np.uint32), src[:, :, :npos].view(np.uint32))
            assert not got[:, :, npos:].any()
    st.close()
