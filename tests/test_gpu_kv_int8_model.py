"""Whole decoder blocks with the int8 KV cache (BS_FLAG_INT8_KV) against the CPU checker, the checker handed the
device's cache (the read_kv -> write_kv pattern of test_gpu_7b1_width.py).

The tiny configuration of the parity tests (h = 64, 4 heads, 4 layers, V = 512; hd = 16), bf16, first and last stage
in one: prefill P = 24 for B = 2 (both sides attend the prompt at bf16), every layer's device cache copied into a
bf16-mode OracleStage, then 6 decode steps fed the checker's tokens; after each step the position the device just
cached is copied across.  The checker attends its own new position unquantised, like the device, so step for step the
two see the same cache and the error sources are those of bf16 decode:
  * logits: test_gpu_parity.check_logits (flat 2e-2 in bf16), ids by assert_ids_match;
  * the vector a step caches vs the checker's own bf16 K / V at that position: one quantisation half-step plus one
    bf16 rounding, scale / 2 + 2^-8 |ref| with scale = max|ref vector| / 127, on top of what check_bf16_stored allows
    two correct bf16 paths (2e-2 + 2^-9 max|ref| + one bf16 ulp of max|ref|).
The same run with set_graphs(False) returns bit-identical tokens and logits.
"""
import numpy as np
import pytest

from distributed_inference_demo_amd.stage import Stage
from oracle import gen_np
from oracle.oracle import OracleStage

from test_gpu_7b1_width import _kv_rows
from test_gpu_parity import BF16_TOL, assert_ids_match, check_logits, record_error

pytestmark = pytest.mark.gpu

H, NH, L, V = 64, 4, 4, 512
HD = H // NH
B, P, STEPS = 2, 24, 6


def check_new_kv(got, ref, what):
    """got / ref [2][nh][1][hd]: the device's dequantised new vectors against the checker's bf16 ones."""
    mx = float(np.abs(ref).max())
    ulp = 2.0 ** (np.floor(np.log2(mx)) - 7) if mx > 0 else 0.0
    scale = np.abs(ref).max(axis=-1, keepdims=True) / 127.0
    tol = scale / 2 + 2.0 ** -8 * np.abs(ref) + (BF16_TOL + 2.0 ** -9 * mx + ulp)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    record_error(what, got, ref, float(tol.max()), "kv int8")
    assert (err <= tol).all(), f"{what}: max-abs {err.max()} (bound {tol.flat[err.argmax()]} there)"


def _device_run(int8_weights, seed, graphs, feed=None, checker=None):
    """Prefill + STEPS decode steps on device buffers (decode replays captured graphs unless graphs is False).
    checker: the OracleStage that is fed the same tokens and handed the device's cache; its tokens drive both.
    feed: the tokens of an earlier run (prefill ids, then one [B] array per step).  Returns (fed, tokens, logits)."""
    import torch
    gs = Stage(H, NH, L, V, 0, L, dtype="bf16", max_batch=B, max_ctx=P + STEPS, max_tokens=B * P, seed=seed,
               int8_weights=int8_weights, kv_int8=True)
    gs.set_graphs(graphs)
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    ids = gen_np.prompt_ids(seed + 5, B, P, V).astype(np.int32)
    fed, toks, lgs = [ids], [], []
    with torch.cuda.stream(cs):
        tin = torch.from_numpy(ids).to(dev)
        tok = torch.empty(B, dtype=torch.int32, device=dev)
        lg = torch.empty((B, V), dtype=torch.float32, device=dev)
        gs.forward(tin, tok, B, P, slot=0, past_len=0, logits=lg, stream=cs.cuda_stream)
        cs.synchronize()
        toks.append(tok.cpu().numpy().copy())
        lgs.append(lg.cpu().numpy().copy())
        nxt = feed[1] if feed is not None else toks[0]
        if checker is not None:
            to, lo = checker.forward(ids, B, P, want_logits=True)
            check_logits(lgs[0], lo, "bf16", "prefill (attends bf16)")
            assert_ids_match(toks[0], to, lo, "prefill")
            for layer in range(L):  # the device's prompt cache (quantised by the prefill) replaces the checker's
                for r in range(B):
                    checker.write_kv(layer, r, 0, gs.read_kv(layer, r, 0, P))
            nxt = to
        for step in range(STEPS):
            past = P + step
            t_in = np.ascontiguousarray(nxt, np.int32)
            fed.append(t_in.copy())
            tok.copy_(torch.from_numpy(t_in))
            gs.forward(tok, tok, B, 1, slot=0, past_len=past, logits=lg, stream=cs.cuda_stream)
            cs.synchronize()
            toks.append(tok.cpu().numpy().copy())
            lgs.append(lg.cpu().numpy().copy())
            nxt = feed[2 + step] if feed is not None and step + 2 < len(feed) else toks[-1]
            if checker is not None:
                to, lo = checker.forward(t_in.reshape(B, 1), B, 1, past_len=past, want_logits=True)
                err = check_logits(lgs[-1], lo, "bf16", f"decode step {step} (ctx {past + 1})")
                print(f"int8_weights={int8_weights} seed {seed} step {step}: logits max-abs {err:.3e}")
                assert_ids_match(toks[-1], to, lo, f"decode step {step}")
                for layer in range(L):
                    for r in range(B):
                        new = gs.read_kv(layer, r, past, 1)
                        check_new_kv(new, _kv_rows(checker, layer, r, past, NH, HD),
                                     f"step {step} new KV layer {layer} row {r}")
                        checker.write_kv(layer, r, past, new)  # the next step reads what the device cached
                nxt = to
    gs.close()
    return fed, toks, lgs


@pytest.mark.parametrize("int8_weights", [False, True])
def test_int8_kv_blocks_match_checker_and_graphs_match_eager(int8_weights):
    seed = 11
    os_ = OracleStage(H, NH, L, V, 0, L, bf16=True, max_batch=B, max_ctx=P + STEPS, seed=seed, int8=int8_weights)
    fed, toks, lgs = _device_run(int8_weights, seed, True, checker=os_)
    os_.close()
    _, toks_e, lgs_e = _device_run(int8_weights, seed, False, feed=fed)
    for i, (a, b) in enumerate(zip(toks, toks_e)):
        assert np.array_equal(a, b), f"call {i}: graph-replayed tokens != eager tokens"
    for i, (a, b) in enumerate(zip(lgs, lgs_e)):
        assert np.array_equal(a, b), f"call {i}: graph-replayed logits != eager logits"
