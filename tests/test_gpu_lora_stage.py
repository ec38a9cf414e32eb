"""Per-row LoRA adapters through the model: a tiny bf16 stage (h = 256, 4 heads, 2 layers, V = 512, 3 KV rows) with two
synthetic adapters on query_key_value, dense and dense_4h_to_h, rows [a0, none, a1], against stages built from the
merged weights W + scale * B A (lora.merged_weights) run with the same batch shape, and against a stage that never
loaded an adapter.  One run = a 20-token prefill from empty, a 7-token continuation and 8 graph-replayed decode steps of
fixed tokens, logits at every pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from distributed_inference_demo_amd import lora
from distributed_inference_demo_amd.stage import AdapterDesc, BloomStageError, RaggedStep, Stage, lib
from oracle import gen_np
from test_gpu_parity import BF16_TOL, assert_ids_match, canonical_weights, check_bf16_stored, record_error

pytestmark = pytest.mark.gpu
H, NH, L, V, SEED, ROWS = 256, 4, 2, 512, 7, 3
NPRE, NCONT, NDEC = 20, 7, 8
ADAPTERS = [lora.synthetic(31 + k, (16, 40)[k], lora.TARGETS, H, L, 0.5) for k in range(2)]
IDS = gen_np.prompt_ids(5, ROWS, NPRE + NCONT + NDEC, V).astype(np.int32)
LONG_PRE = 150  # the small-batch case: a context of three 64-position chunks, split two ways at max_ctx 320
LONG_IDS = gen_np.prompt_ids(6, 2, LONG_PRE + NCONT + NDEC, V).astype(np.int32)


def make_stage(kv="bf16", weights=None, dtype="bf16", rows=ROWS, max_ctx=64, **kw):
    return Stage(H, NH, L, V, 0, L, dtype=dtype, max_batch=rows, max_ctx=max_ctx, max_tokens=512, seed=SEED,
                 host_weights=weights, kv_int8=kv == "int8", **kw)


def decode_buffers(rows=ROWS):
    """The stream and the device buffers of a run's decode steps: a captured step's graph is keyed by them."""
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        return (stream, torch.empty(rows, dtype=torch.int32, device="cuda"),
                torch.empty(rows, dtype=torch.int32, device="cuda"),
                torch.empty(rows, V, dtype=torch.float32, device="cuda"))


def run(st, bufs=None, rows=ROWS, npre=NPRE):
    """The passes of one run on `st` from empty rows: (logits fp32 [10][rows][V], ids int32 [10][rows])."""
    tok = IDS[:rows] if npre == NPRE else LONG_IDS[:rows]
    ids1, lg1 = st.forward_host(tok[:, :npre], rows, npre, past_len=0, want_logits=True)
    ids2, lg2 = st.forward_host(tok[:, npre:npre + NCONT], rows, NCONT, past_len=npre, want_logits=True)
    logits, ids = [lg1, lg2], [ids1, ids2]
    stream, inp, out, lg = bufs or decode_buffers(rows)
    with torch.cuda.stream(stream):
        for t in range(NDEC):
            inp.copy_(torch.from_numpy(tok[:, npre + NCONT + t].copy()))
            st.forward(inp, out, rows, 1, past_len=npre + NCONT + t, logits=lg, stream=stream.cuda_stream)
            stream.synchronize()
            logits.append(lg.cpu().numpy())
            ids.append(out.cpu().numpy())
    return np.stack(logits), np.stack(ids)


def kv_rows(st, row):
    return np.stack([st.read_kv(l, row, 0, NPRE + NCONT + NDEC) for l in range(L)])


@functools.lru_cache(maxsize=None)
def adapted(kv, assign=(0, -1, 1), graphs=True, **kw):
    """A stage with both adapters loaded and rows named by `assign`, after one run: (stage, logits, ids)."""
    st = make_stage(kv, **dict(kw))
    loaded = [st.load_adapter(a) for a in ADAPTERS]
    st.set_graphs(graphs)
    for r, k in enumerate(assign):
        st.set_row_adapter(r, loaded[k] if k >= 0 else -1)
    return (st,) + run(st)


@functools.lru_cache(maxsize=None)
def plain(kv, merged=-1, **kw):
    """A stage that never loaded an adapter, on the base weights or on adapter `merged`'s merged weights."""
    w = canonical_weights(SEED, H, L, V)
    st = make_stage(kv, lora.merged_weights(w, ADAPTERS[merged], H, V) if merged >= 0 else w, **dict(kw))
    return (st,) + run(st)


@pytest.mark.parametrize("kv", ["bf16", "int8"])
def test_adapted_rows_match_merged_weights(kv):
    st, lg, ids = adapted(kv)
    _, lg_base, _ = plain(kv)
    for k, row in ((0, 0), (1, 2)):
        ref, lg_ref, ids_ref = plain(kv, k)
        apart = float(np.abs(lg_ref[:, row] - lg_base[:, row]).max())
        assert apart >= 10 * BF16_TOL, f"adapter {k} moves the logits by {apart} only: the check would pass without it"
        err = record_error(f"lora {kv} adapter {k} logits vs merged", lg[:, row], lg_ref[:, row], BF16_TOL, "logits bf16")
        print(f"adapter {k} kv {kv}: logits max-abs {err:.5f} (bound {BF16_TOL}), base is {apart:.3f} away")
        assert err <= BF16_TOL, f"adapter {k}: logits max-abs {err} > {BF16_TOL} against the merged-weights stage"
        assert_ids_match(ids[:, row], ids_ref[:, row], lg_ref[:, row], f"adapter {k} ids")
        if kv == "bf16":
            check_bf16_stored(kv_rows(st, row), kv_rows(ref, row), f"lora adapter {k} K/V vs merged")


@pytest.mark.parametrize("kv", ["bf16", "int8"])
def test_row_without_adapter_keeps_the_base_bits(kv):
    st, lg, _ = adapted(kv)
    base, lg_base, _ = plain(kv)
    assert np.array_equal(lg[:, 1].view(np.uint32), lg_base[:, 1].view(np.uint32))
    assert np.array_equal(kv_rows(st, 1).view(np.uint32), kv_rows(base, 1).view(np.uint32))


def test_eager_graph_and_second_run_agree_bitwise_and_a_replay_follows_a_swap():
    """A stage of its own, ONE stream and one set of decode buffers throughout: the graph key of a decode step (shape,
    slot, flags, tail, stream, in / out / logits pointers, the adapter bit) is the same in every run below, so the
    steps after the first run replay the graphs captured with rows [a0, none, a1]."""
    _, lg, ids = adapted("bf16")
    _, lg_eager, ids_eager = adapted("bf16", graphs=False)
    assert np.array_equal(lg.view(np.uint32), lg_eager.view(np.uint32)) and np.array_equal(ids, ids_eager)
    st = make_stage()
    a0, a1 = [st.load_adapter(a) for a in ADAPTERS]
    bufs = decode_buffers()
    for assign in ((a0, -1, a1), (a0, -1, a1)):  # the first run captures, the second replays
        st.reset()
        assert [st.read_row_adapter(r) for r in range(ROWS)] == [-1] * ROWS  # bs_reset_kv cleared the rows
        for r, a in enumerate(assign):
            st.set_row_adapter(r, a)
        lg2, ids2 = run(st, bufs)
        assert np.array_equal(lg.view(np.uint32), lg2.view(np.uint32)) and np.array_equal(ids, ids2)
    # rows 0 and 2 swap adapters on the same handles: the captured steps must read the new ids on the device
    st.reset()
    for r, a in enumerate((a1, -1, a0)):
        st.set_row_adapter(r, a)
    lg3, ids3 = run(st, bufs)
    _, lg_sw, ids_sw = adapted("bf16", assign=(1, -1, 0))
    assert np.array_equal(lg3.view(np.uint32), lg_sw.view(np.uint32)) and np.array_equal(ids3, ids_sw)
    assert not np.array_equal(lg3[:, 0], lg[:, 0])


@pytest.mark.parametrize("rows", [1, 2])
def test_small_batch_decode_matches_merged_weights(rows):
    """B = 1 / 2 on a first stage at max_ctx 320 (5 chunks: the decode attention splits two ways and the dense GEMV
    merges the partials in its prologue; layer 0 fuses the embedding into its QKV GEMV): the dense adapter reads the
    ctx a kernel of lora.hip merges, the QKV adapter the LayerNorm of the residual the fused kernel stored.  Every row
    on adapter 1, against the merged-weights stage of the same shape."""
    st = make_stage(rows=rows, max_ctx=320)
    aid = st.load_adapter(ADAPTERS[1])
    st.set_row_adapter(0, aid, count=rows)
    lg, ids = run(st, rows=rows, npre=LONG_PRE)
    w = canonical_weights(SEED, H, L, V)
    lg_base, _ = run(make_stage(weights=w, rows=rows, max_ctx=320), rows=rows, npre=LONG_PRE)
    ref = make_stage(weights=lora.merged_weights(w, ADAPTERS[1], H, V), rows=rows, max_ctx=320)
    lg_ref, ids_ref = run(ref, rows=rows, npre=LONG_PRE)
    apart = float(np.abs(lg_ref[2:] - lg_base[2:]).max())
    assert apart >= 10 * BF16_TOL, f"the adapter moves the decode logits by {apart} only"
    err = record_error(f"lora B={rows} decode logits vs merged", lg, lg_ref, BF16_TOL, "logits bf16")
    print(f"B={rows}: logits max-abs {err:.5f} (bound {BF16_TOL}), base is {apart:.3f} away")
    assert err <= BF16_TOL, f"logits max-abs {err} > {BF16_TOL} against the merged-weights stage"
    assert_ids_match(ids.reshape(-1), ids_ref.reshape(-1), lg_ref.reshape(-1, V), f"B={rows} ids")
    n = LONG_PRE + NCONT + NDEC
    for row in range(rows):
        got = np.stack([st.read_kv(l, row, 0, n) for l in range(L)])
        want = np.stack([ref.read_kv(l, row, 0, n) for l in range(L)])
        check_bf16_stored(got, want, f"lora B={rows} row {row} K/V vs merged")


def test_adapter_over_int8_weights():
    _, lg, _ = adapted("bf16", assign=(0, -1, -1), int8_weights=True)
    _, lg_base, _ = plain("bf16", int8_weights=True)
    assert np.array_equal(lg[:, 1].view(np.uint32), lg_base[:, 1].view(np.uint32))
    assert np.abs(lg[:, 0] - lg_base[:, 0]).max() >= 10 * BF16_TOL


def test_statuses_and_workspace():
    L_ = lib()
    assert L_.bs_abi_version() == 5
    st = make_stage()
    ad = ADAPTERS[0]
    arrs = [np.ascontiguousarray(ad.a["qkv"]), np.ascontiguousarray(ad.b["qkv"])]

    def load(stage, rank, targets):
        d = AdapterDesc(rank, 1.0, targets)
        d.a[0], d.b[0] = arrs[0].ctypes.data, arrs[1].ctypes.data
        return L_.bs_load_adapter(stage._h, ctypes.byref(d), ctypes.byref(ctypes.c_int32()))

    assert load(make_stage(dtype="fp32"), 16, 1) == -5
    assert [load(st, 0, 1), load(st, 65, 1), load(st, 16, 0)] == [-1, -1, -1]
    ws0 = st.info()["workspace_bytes"]
    aid = st.load_adapter(ad)
    ws1 = st.info()["workspace_bytes"]
    assert ws1 > ws0
    assert L_.bs_set_row_adapter(st._h, 0, 1, 5, None) == -1       # an id that is not loaded
    assert L_.bs_set_row_adapter(st._h, 2, 2, aid, None) == -1     # rows [2, 4) of 3
    st.set_row_adapter(1, aid)
    assert st.info()["workspace_bytes"] == ws1
    assert st.read_row_adapter(1) == aid and st.read_row_adapter(0) == -1
    assert L_.bs_unload_adapter(st._h, aid) == -4
    ids = np.zeros(4, np.int32)
    out = np.zeros(1, np.int32)
    one = lambda v: (ctypes.c_int32 * 1)(v)
    rs = RaggedStep(1, 1, one(1), one(4), one(0))
    assert L_.bs_forward_ragged(st._h, ctypes.byref(rs), ids.ctypes.data, out.ctypes.data, None, None) == -4
    st.reset(1)
    assert st.read_row_adapter(1) == -1
    st.unload_adapter(aid)
    assert st.info()["workspace_bytes"] < ws1
    with pytest.raises(BloomStageError):
        st.set_row_adapter(0, aid)
