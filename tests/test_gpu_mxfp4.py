"""Weight-only MXFP4 stages (BS_FLAG_MXFP4_WEIGHTS) on the GPU.

Every dequantised MXFP4 weight is exact in bf16, so an MXFP4 stage is the same model as a plain bf16 stage whose host
weights are the dequantised values W' = read_weights() of the MXFP4 stage: that bf16 stage is the reference of every
test below.  Where both run the same kernels on the same bf16 operands (prefill, M > 32: the codes are dequantised
to scratch and the bf16 GEMM runs) the outputs are bit-identical; the fp4 GEMV (decode of a few rows) is a second fp32-accumulating
evaluation of the same bf16 model in another summation order, held to the project's bf16 bounds
(tests/test_gpu_parity.py check_close / check_logits / BF16_TOL).

Measured on MI355X (max-abs against the reference, the largest over the calls of each test):
  family widths, hidden states (bound 2e-2 + 2^-9 max|ref|): 560m 3.0e-3, 1b1 3.6e-3, 3b 7.1e-3, 7b1 2.0e-2
  whole model, logits (bound 2e-2): B=1 0, B=2 2.4e-3, B=4 3.0e-3, B=8 2.8e-3, B=9..32 0 (the dequant route)
  graph decode after a 1000-token prompt, logits (bound 2e-2): 1.8e-4
"""
import functools

import numpy as np
import pytest

import mxfp4_np
from distributed_inference_demo_amd.stage import (BS_FLAG_MXFP4_WEIGHTS, BloomStageError, Stage, StageDesc, lib)
from golden_io import load_parts
from oracle import gen_np

from test_gpu_parity import BF16_TOL, assert_ids_match, canonical_weights, check_close, check_logits

pytestmark = pytest.mark.gpu


def mx_pair(h, nh, L, V, lb, le, seed, **kw):
    """An MXFP4 stage (synthetic weights) and the bf16 stage on its dequantised weights W'."""
    g = Stage(h, nh, L, V, lb, le, dtype="bf16", seed=seed, mxfp4_weights=True, **kw)
    r = Stage(h, nh, L, V, lb, le, dtype="bf16", host_weights=g.read_weights(), **kw)
    return g, r


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0.0)).view(np.uint32)  # + 0.0: the sign of a zero code is free


# ---- 1. quantisation bits
def test_device_quantization_is_bit_exact():
    h, nh, L, V = 128, 4, 2, 512
    w = gen_np.bf16_round(canonical_weights(4, h, L, V))
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_ctx=8, seed=4, mxfp4_weights=True)
    got = st.read_weights()
    want = w.copy()
    off = V * h + 2 * h
    sizes = [h, h, 3 * h * h, 3 * h, h * h, h, h, h, 4 * h * h, 4 * h, 4 * h * h, h]
    kdim = {2: h, 4: h, 8: h, 10: 4 * h}
    matrix = np.zeros(w.size, bool)
    for _ in range(L):
        for t, n in enumerate(sizes):
            if t in kdim:
                want[off:off + n] = mxfp4_np.roundtrip(w[off:off + n].reshape(-1, kdim[t])).reshape(-1)
                matrix[off:off + n] = True
            off += n
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (bad[:10], got[bad[:5]], want[bad[:5]], w[bad[:5]])
    assert np.array_equal(got[~matrix].view(np.uint32), w[~matrix].view(np.uint32))  # the rest stays the bf16 weight
    assert (got[matrix] != w[matrix]).mean() > 0.5  # and the matrices really are quantised
    # a piece that starts and ends inside blocks reads the same values
    lo = V * h + 2 * h + 2 * h + 5 * h + 13
    assert np.array_equal(_bits(st.read_weights(lo, 3 * h + 40)), _bits(got[lo:lo + 3 * h + 40]))
    hw = Stage(h, nh, L, V, 0, L, dtype="bf16", max_ctx=8, host_weights=canonical_weights(4, h, L, V), mxfp4_weights=True)
    assert np.array_equal(_bits(hw.read_weights()), _bits(got))


# ---- 2. prefill: the same kernels on the same bf16 operands
@pytest.mark.parametrize("last", [False, True])
def test_prefill_is_bit_identical_to_bf16_stage(last):
    h, nh, L, V = 256, 4, 2, 1024
    g, r = mx_pair(h, nh, L, V, 0, L, 3, max_ctx=136, max_tokens=96, is_last=last)
    ids = gen_np.prompt_ids(2, 1, 136, V).astype(np.int32)
    for past, S in ((0, 96), (96, 40)):
        x = ids[:, past:past + S]
        a = g.forward_host(x, 1, S, past_len=past, want_logits=last)
        b = r.forward_host(x, 1, S, past_len=past, want_logits=last)
        if last:
            assert np.array_equal(a[0], b[0]), f"S={S} past={past}: tokens"
            a, b = a[1], b[1]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            f"S={S} past={past}: {np.abs(a - b).max()} max-abs apart"


# ---- 3. the family's widths: every row count and prologue of the fp4 GEMV, the 48- and 80-block row tails
@pytest.mark.parametrize("fam", ["560m", "1b1", "3b", "7b1"])
def test_family_width_block_decode_chunks(fam):
    f = load_parts("family_blocks")
    h, nh = (int(v) for v in f[fam + "_config"][:2])
    V = 1024
    g, r = mx_pair(h, nh, 1, V, 0, 1, 5, max_ctx=40, max_tokens=16, is_last=False)
    ids = gen_np.prompt_ids(7, 1, 38, V).astype(np.int32)
    past, worst = 0, 0.0
    for S in (15, 1, 2, 3, 4, 5, 8):
        x = ids[:, past:past + S]
        worst = max(worst, check_close(g.forward_host(x, 1, S, past_len=past), r.forward_host(x, 1, S, past_len=past),
                                       "bf16", f"{fam} mxfp4 S={S} past={past}"))
        past += S
    print(f"{fam} (h {h}): hidden max-abs {worst:.3e}")


# ---- 4. whole model, batched
@functools.lru_cache(maxsize=None)
def _model_weights():
    """W' of the h = 512 model (the same for every batch size)."""
    st = Stage(512, 8, 3, 2048, 0, 3, dtype="bf16", max_ctx=8, seed=7, mxfp4_weights=True)
    w = st.read_weights()
    st.close()
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("B", [1, 2, 4, 8, 9, 20, 32])
def test_whole_model_batched_greedy_decode(B):
    h, nh, L, V = 512, 8, 3, 2048
    kw = dict(dtype="bf16", max_batch=B + 1, max_ctx=40, max_tokens=B * 8)
    g = Stage(h, nh, L, V, 0, L, seed=7, mxfp4_weights=True, **kw)
    r = Stage(h, nh, L, V, 0, L, host_weights=_model_weights(), **kw)
    ids = gen_np.prompt_ids(9, B, 8, V).astype(np.int32)
    tg, lg = g.forward_host(ids, B, 8, slot=1, past_len=0, want_logits=True)
    tr, lr = r.forward_host(ids, B, 8, slot=1, past_len=0, want_logits=True)
    worst = check_logits(lg, lr, "bf16", f"B={B} mxfp4 prefill")
    assert_ids_match(tg, tr, lr, f"B={B} mxfp4 prefill")
    for step in range(6):
        x = tr.reshape(B, 1)  # teacher-forced with the reference's ids
        tg, lg = g.forward_host(x, B, 1, slot=1, past_len=8 + step, want_logits=True)
        tr, lr = r.forward_host(x, B, 1, slot=1, past_len=8 + step, want_logits=True)
        worst = max(worst, check_logits(lg, lr, "bf16", f"B={B} mxfp4 decode step {step}"))
        assert_ids_match(tg, tr, lr, f"B={B} mxfp4 decode step {step}")
    print(f"B={B}: logits max-abs {worst:.3e}")


# ---- 5. graph-replayed decode over a split-attention context
def test_long_context_graph_decode_and_eager_twin():
    import torch
    h, nh, L, V, P, STEPS = 1536, 16, 2, 1024, 1000, 24
    kw = dict(dtype="bf16", max_ctx=P + STEPS, max_tokens=P)  # 16 chunks of 64: 4 context splits, merged by the dense GEMV
    g = Stage(h, nh, L, V, 0, L, seed=5, mxfp4_weights=True, **kw)
    e = Stage(h, nh, L, V, 0, L, seed=5, mxfp4_weights=True, **kw)
    e.set_graphs(False)
    r = Stage(h, nh, L, V, 0, L, host_weights=g.read_weights(), **kw)
    ids = gen_np.prompt_ids(3, 1, P, V).astype(np.int32)
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    worst = 0.0
    with torch.cuda.stream(cs):
        tin = torch.from_numpy(ids).to(dev)
        tok, tok_e = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
        lg, lg_e = (torch.empty((1, V), dtype=torch.float32, device=dev) for _ in range(2))
        g.forward(tin, tok, 1, P, slot=0, past_len=0, logits=lg, stream=cs.cuda_stream)
        e.forward(tin, tok_e, 1, P, slot=0, past_len=0, logits=lg_e, stream=cs.cuda_stream)
        tr, lr = r.forward_host(ids, 1, P, want_logits=True)
        torch.cuda.synchronize()
        assert np.array_equal(lg.cpu().numpy(), lr), "prefill logits are the bf16 stage's, bit for bit"
        for step in range(STEPS):
            tok.copy_(torch.from_numpy(tr))
            tok_e.copy_(torch.from_numpy(tr))
            g.forward(tok, tok, 1, 1, slot=0, past_len=P + step, logits=lg, stream=cs.cuda_stream)
            e.forward(tok_e, tok_e, 1, 1, slot=0, past_len=P + step, logits=lg_e, stream=cs.cuda_stream)
            tr, lr = r.forward_host(tr.reshape(1, 1), 1, 1, past_len=P + step, want_logits=True)
            torch.cuda.synchronize()
            a, b = lg.cpu().numpy(), lg_e.cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"step {step}: replayed != eager logits"
            assert np.array_equal(tok.cpu().numpy(), tok_e.cpu().numpy()), f"step {step}: replayed != eager token"
            if step % 5 == 0 or step == STEPS - 1:
                worst = max(worst, check_logits(a, lr, "bf16", f"mxfp4 graph decode step {step}"))
                assert_ids_match(tok.cpu().numpy(), tr, lr, f"mxfp4 graph decode step {step}")
    print(f"graph decode: logits max-abs {worst:.3e}")


def test_split_attention_merge_two_rows():
    """Two rows over a context long enough to split (max_ctx 320: 2 splits): the M = 2 merge prologue."""
    h, nh, L, V, B, P = 256, 4, 2, 1024, 2, 300
    g, r = mx_pair(h, nh, L, V, 0, L, 17, max_batch=B, max_ctx=320, max_tokens=B * P)
    ids = gen_np.prompt_ids(8, B, P, V).astype(np.int32)
    tg, lg = g.forward_host(ids, B, P, want_logits=True)
    tr, lr = r.forward_host(ids, B, P, want_logits=True)
    assert np.array_equal(lg, lr)
    for step in range(4):
        x = tr.reshape(B, 1)
        tg, lg = g.forward_host(x, B, 1, past_len=P + step, want_logits=True)
        tr, lr = r.forward_host(x, B, 1, past_len=P + step, want_logits=True)
        check_logits(lg, lr, "bf16", f"mxfp4 2-row split decode step {step}")
        assert_ids_match(tg, tr, lr, f"mxfp4 2-row split decode step {step}")


# ---- 6. combinations
def test_with_int8_kv_cache():
    h, nh, L, V, B, P = 256, 4, 2, 1024, 2, 24
    g, r = mx_pair(h, nh, L, V, 0, L, 11, max_batch=B, max_ctx=P + 8, max_tokens=B * P, kv_int8=True)
    ids = gen_np.prompt_ids(16, B, P, V).astype(np.int32)
    tg, lg = g.forward_host(ids, B, P, want_logits=True)
    tr, lr = r.forward_host(ids, B, P, want_logits=True)
    assert np.array_equal(lg, lr)  # M = 48: the same kernels, and the same cache codes for the steps below
    for step in range(6):
        x = tr.reshape(B, 1)
        tg, lg = g.forward_host(x, B, 1, past_len=P + step, want_logits=True)
        tr, lr = r.forward_host(x, B, 1, past_len=P + step, want_logits=True)
        check_logits(lg, lr, "bf16", f"mxfp4 + int8 KV decode step {step}")
        assert_ids_match(tg, tr, lr, f"mxfp4 + int8 KV decode step {step}")


def test_with_classifier_tail():
    h, nh, L, V, B, nl = 256, 4, 4, 1024, 3, 3
    g, r = mx_pair(h, nh, L, V, 2, L, 21, max_batch=B, max_ctx=40, n_labels=nl)
    rng = np.random.default_rng(5)
    past = 0
    for S in (12, 1, 1, 2):
        hid = rng.standard_normal((B, S, h)).astype(np.float32)
        cg, lg = g.forward_host(hid, B, S, past_len=past, want_logits=True)
        cr, lr = r.forward_host(hid, B, S, past_len=past, want_logits=True)
        assert lg.shape == (B, nl)
        check_logits(lg, lr, "bf16", f"mxfp4 classifier S={S}")
        assert_ids_match(cg, cr, lr, f"mxfp4 classifier S={S}")
        past += S


def test_forward_score_on_mxfp4_last_stage():
    h, nh, L, V, B, S = 256, 4, 2, 1024, 2, 12
    g, r = mx_pair(h, nh, L, V, 0, L, 13, max_batch=B, max_ctx=S + 2, max_tokens=B * S)
    ids = gen_np.prompt_ids(4, B, S, V).astype(np.int32)
    targets = np.full((B, S), -1, np.int32)
    targets[:, :-1] = ids[:, 1:]
    top_g, sc_g = g.score_host(ids, targets, B, S)
    top_r, sc_r = r.score_host(ids, targets, B, S)
    assert np.isfinite(sc_g).all() and (sc_g[:, :-1, 0] < 0).all() and (sc_g[:, -1, 0] == 0).all()
    assert np.abs(sc_g - sc_r).max() <= 2 * BF16_TOL  # a log-prob is a difference of two logit-tolerance quantities
    # where the greedy ids differ, the reference itself ranks the two within the logit tolerance (a near-tie)
    r.reset()
    _, sc_x = r.score_host(ids, top_g, B, S)
    gap = sc_x[..., 1] - sc_x[..., 0]  # reference log p(its top id) - reference log p(the MXFP4 stage's top id)
    differ = top_g != top_r
    assert (gap[differ] < BF16_TOL).all(), (np.argwhere(differ)[:5], gap[differ][:5])
    assert (gap[~differ] == 0).all()


# ---- 7. storage and errors
def test_weight_bytes_of_a_middle_stage():
    h, nh, L, V = 512, 8, 4, 2048
    kw = dict(dtype="bf16", max_ctx=8, seed=1, is_first=False, is_last=False)
    mx = Stage(h, nh, L, V, 1, 3, mxfp4_weights=True, **kw).info()["weight_bytes"]
    bf = Stage(h, nh, L, V, 1, 3, **kw).info()["weight_bytes"]
    i8 = Stage(h, nh, L, V, 1, 3, int8_weights=True, **kw).info()["weight_bytes"]
    assert mx < 0.30 * bf and mx < 0.6 * i8, (mx, i8, bf)
    assert mx >= 2 * 12 * h * h * mxfp4_np.BYTES_PER_WEIGHT  # codes and scales are all there


def _init_rc(**kw):
    d = StageDesc()
    d.hidden, d.n_head, d.n_layer, d.vocab, d.ln_eps = 64, 4, 1, 256, 1e-5
    d.layer_begin, d.layer_end, d.is_first, d.is_last = 0, 1, 1, 1
    d.dtype, d.max_batch, d.max_ctx, d.flags = 16, 1, 4, BS_FLAG_MXFP4_WEIGHTS
    for k, v in kw.items():
        setattr(d, k, v)
    import ctypes
    out = ctypes.c_void_p()
    rc = lib().bs_init_stage(ctypes.byref(d), ctypes.byref(out))
    msg = lib().bs_last_error().decode() if rc else ""
    if out.value:
        lib().bs_release(out)
    assert (rc == 0) == bool(out.value)
    return rc, msg


def test_error_codes():
    rc, msg = _init_rc(dtype=1)
    assert rc == -5 and "BFLOAT16" in msg, (rc, msg)                      # BS_ERR_UNSUPPORTED: fp32 stage
    rc, msg = _init_rc(flags=BS_FLAG_MXFP4_WEIGHTS | 1)
    assert rc == -1 and "INT8_WEIGHTS" in msg, (rc, msg)                  # BS_ERR_INVALID: with int8 weights
    rc, msg = _init_rc(hidden=48)
    assert rc == -5 and "multiple of 32" in msg, (rc, msg)                # BS_ERR_UNSUPPORTED: hidden % 32
    with pytest.raises(BloomStageError, match="multiple of 32"):
        Stage(48, 4, 1, 256, 0, 1, dtype="bf16", max_ctx=4, mxfp4_weights=True)
    rc, msg = _init_rc()                                                  # and the plain case is accepted
    assert rc == 0, (rc, msg)
