"""Batched decode on MXFP4 weights: the fp4 tile GEMV (gemv_mx4_tiles, 5..32 rows, K % 128 == 0).

The reference is the one of tests/test_gpu_mxfp4.py: a plain bf16 stage on W' = read_weights() of the MXFP4 stage
(exact in bf16), held to the project's bf16 bounds (check_close: 2e-2 + 2^-9 max|ref|; logits: BF16_TOL).
"""
import numpy as np
import pytest

from distributed_inference_demo_amd.stage import Stage
from golden_io import load_parts
from oracle import gen_np

from test_gpu_mxfp4 import mx_pair
from test_gpu_parity import assert_ids_match, check_close, check_logits

pytestmark = pytest.mark.gpu


def test_batched_rows_are_counted_as_weight_gemvs():
    h, nh, L, V, M = 1024, 16, 2, 1024, 16
    g = Stage(h, nh, L + 2, V, 1, L + 1, dtype="bf16", seed=3, mxfp4_weights=True, max_batch=M, max_ctx=40, max_tokens=40,
              is_first=False, is_last=False)
    rng = np.random.default_rng(1)
    g.profile_enable(1)
    g.forward_host(rng.standard_normal((M, 1, h)).astype(np.float32), M, 1, past_len=0)
    _, launches, units = g.profile_read()
    want = L * sum(0.53125 * N * K + 2 * N + 2 * M * K + M * N * ob
                   for N, K, ob in ((3 * h, h, 4), (h, h, 4), (4 * h, h, 2), (h, 4 * h, 4)))
    assert launches == 4 * L, launches
    assert abs(units - want) <= 1e-6 * want, (units, want)
    g.reset()
    g.profile_enable(1)
    g.forward_host(rng.standard_normal((1, 33, h)).astype(np.float32), 1, 33, past_len=0)
    assert g.profile_read()[1] == 0  # 33 rows: the dequant pass and the GEMM


@pytest.mark.parametrize("fam", ["560m", "1b1", "3b", "7b1"])
def test_family_width_block_row_counts(fam):
    f = load_parts("family_blocks")
    h, nh = (int(v) for v in f[fam + "_config"][:2])
    V = 1024
    g, r = mx_pair(h, nh, 1, V, 0, 1, 5, max_ctx=104, max_tokens=32, is_last=False)
    ids = gen_np.prompt_ids(7, 1, 102, V).astype(np.int32)
    past, worst = 0, 0.0
    for S in (15, 5, 8, 9, 16, 17, 32):
        x = ids[:, past:past + S]
        worst = max(worst, check_close(g.forward_host(x, 1, S, past_len=past), r.forward_host(x, 1, S, past_len=past),
                                       "bf16", f"{fam} mxfp4 tiles S={S} past={past}"))
        past += S
    print(f"{fam} (h {h}): hidden max-abs {worst:.3e}")


@pytest.mark.parametrize("B", [5, 32])
def test_edges_fallback_k_and_partial_tiles(B):
    """h = 320: K = 320 keeps the dequant route (not a multiple of 128), K = 1280 is 10 groups for 8 waves."""
    h, nh, L, V = 320, 4, 2, 1024
    g, r = mx_pair(h, nh, L, V, 0, L, 9, max_batch=B, max_ctx=16, max_tokens=B * 8)
    ids = gen_np.prompt_ids(11, B, 8, V).astype(np.int32)
    tg, lg = g.forward_host(ids, B, 8, want_logits=True)
    tr, lr = r.forward_host(ids, B, 8, want_logits=True)
    worst = check_logits(lg, lr, "bf16", f"B={B} edges prefill")
    for step in range(4):
        x = tr.reshape(B, 1)  # teacher-forced with the reference's ids
        tg, lg = g.forward_host(x, B, 1, past_len=8 + step, want_logits=True)
        tr, lr = r.forward_host(x, B, 1, past_len=8 + step, want_logits=True)
        worst = max(worst, check_logits(lg, lr, "bf16", f"B={B} edges decode step {step}"))
        assert_ids_match(tg, tr, lr, f"B={B} edges decode step {step}")
    print(f"B={B}: logits max-abs {worst:.3e}")


def test_graph_replay_eager_twin_and_rerun_are_bit_identical():
    import torch
    h, nh, L, V, B, P, STEPS = 1024, 16, 2, 1024, 16, 8, 8
    kw = dict(dtype="bf16", max_batch=B, max_ctx=P + STEPS, max_tokens=B * P)
    runs = [Stage(h, nh, L, V, 0, L, seed=5, mxfp4_weights=True, **kw) for _ in range(3)]  # replayed, eager, fresh
    runs[1].set_graphs(False)
    r = Stage(h, nh, L, V, 0, L, host_weights=runs[0].read_weights(), **kw)
    ids = gen_np.prompt_ids(3, B, P, V).astype(np.int32)
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    worst = 0.0
    with torch.cuda.stream(cs):
        tin = torch.from_numpy(ids).to(dev)
        tok = [torch.empty(B, dtype=torch.int32, device=dev) for _ in runs]
        lg = [torch.empty((B, V), dtype=torch.float32, device=dev) for _ in runs]
        for s, t, l in zip(runs, tok, lg):
            s.forward(tin, t, B, P, slot=0, past_len=0, logits=l, stream=cs.cuda_stream)
        tr, lr = r.forward_host(ids, B, P, want_logits=True)
        for step in range(STEPS):
            for s, t, l in zip(runs, tok, lg):
                t.copy_(torch.from_numpy(tr))
                s.forward(t, t, B, 1, slot=0, past_len=P + step, logits=l, stream=cs.cuda_stream)
            tr, lr = r.forward_host(tr.reshape(B, 1), B, 1, past_len=P + step, want_logits=True)
            torch.cuda.synchronize()
            a = lg[0].cpu().numpy()
            for i, what in ((1, "eager twin"), (2, "fresh stage")):
                assert np.array_equal(a.view(np.uint32), lg[i].cpu().numpy().view(np.uint32)), f"step {step}: {what} logits"
                assert np.array_equal(tok[0].cpu().numpy(), tok[i].cpu().numpy()), f"step {step}: {what} tokens"
            worst = max(worst, check_logits(a, lr, "bf16", f"mxfp4 tiles graph decode step {step}"))
            assert_ids_match(tok[0].cpu().numpy(), tr, lr, f"mxfp4 tiles graph decode step {step}")
    print(f"graph decode B={B}: logits max-abs {worst:.3e}")
