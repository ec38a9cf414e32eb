"""Whole stages through bs_forward_ragged against the CPU checker run per row, the decode steps that follow a ragged
pass (the cache contents and the device positions it leaves), the status codes and the workspace growth."""
import ctypes
import functools

import numpy as np
import pytest

from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.stage import RaggedStep, Stage
from oracle import gen_np
from oracle.oracle import OracleStage

from test_gpu_parity import check_logits
from test_gpu_verify import MSEED, SMALL, WIDE, _check_ids

pytestmark = pytest.mark.gpu

# (slot, new tokens, past): lengths 5 and 19 from empty, 4 new tokens after a 7-token past laid down by bs_forward
ROWS = [(1, 5, 0), (2, 19, 0), (0, 4, 7)]
NDEC = 2  # ordinary decode steps after the ragged pass


@functools.lru_cache(maxsize=None)
def _reference(cfg, int8=False):
    """Per row the checker alone: ids [3][24]; logits [3][1 + NDEC][V] of the row's last ragged token and of the
    NDEC teacher-forced decode steps after it."""
    h, nh, L, V = cfg
    ids = gen_np.prompt_ids(5, len(ROWS), 24, V).astype(np.int32)
    lg = np.empty((len(ROWS), 1 + NDEC, V), np.float32)
    for r, (_, S, past) in enumerate(ROWS):
        o = OracleStage(h, nh, L, V, 0, L, bf16=True, max_batch=1, max_ctx=32, seed=MSEED, int8=int8)
        n = past + S
        _, lg[r, 0] = o.forward(ids[r, :n], 1, n, want_logits=True)
        for i in range(NDEC):
            _, lg[r, 1 + i] = o.forward(ids[r, n + i:n + i + 1], 1, 1, past_len=n + i, want_logits=True)
        o.close()
    lg.setflags(write=False)
    ids.setflags(write=False)
    return ids, lg


@pytest.mark.parametrize("cfg,split,variant", [(SMALL, False, ""), (SMALL, True, ""), (WIDE, False, ""),
                                               (WIDE, True, "w_int8")])
def test_ragged_pass_and_the_decode_after_it_match_the_checker(cfg, split, variant):
    h, nh, L, V = cfg
    ids, ref = _reference(cfg, variant == "w_int8")
    kw = dict(dtype="bf16", max_batch=3, max_ctx=32, max_tokens=32, seed=MSEED,
              **({"int8_weights": True} if variant else {}))
    sts = [Stage(h, nh, L, V, 0, 1, **kw), Stage(h, nh, L, V, 1, L, **kw)] if split else [Stage(h, nh, L, V, 0, L, **kw)]
    what = f"{cfg} split={split} {variant}"

    def chain(fn):
        x = None
        for st in sts:
            x = fn(st, x)
        return x
    slot0, S0, past0 = ROWS[2]
    chain(lambda st, x: st.forward_host(ids[2, :past0] if x is None else x, 1, past0, slot=slot0, past_len=0))
    slots, lens, pasts = zip(*ROWS)
    packed = np.concatenate([ids[r, p:p + S] for r, (_, S, p) in enumerate(ROWS)])
    tok, lg = chain(lambda st, x: st.forward_ragged_host(packed if x is None else x, slots, lens, pasts,
                                                         **({"want_logits": True} if st.is_last else {})))
    for r in range(len(ROWS)):
        check_logits(lg[r], ref[r, 0], "bf16", f"{what} ragged row {r}")
    _check_ids(f"{what} ragged", tok, lg, ref[:, 0], "bf16")
    assert sts[-1].read_head_screen() is None  # the ragged tail is never screened
    # two ordinary decode steps of KV rows 0..2 at per-row positions: the cache and the device positions hold
    order = np.argsort(slots)  # call row b = KV row b
    at = [pasts[r] + lens[r] for r in order]
    for i in range(NDEC):
        x = np.array([ids[r, at[b] + i] for b, r in enumerate(order)], np.int32)
        pl = [a + i for a in at]
        tok, lg = chain(lambda st, y: st.forward_host(x if y is None else y, 3, 1, past_len=pl,
                                                      **({"want_logits": True} if st.is_last else {})))
        for b, r in enumerate(order):
            check_logits(lg[b], ref[r, 1 + i], "bf16", f"{what} decode {i} row {r}")
        _check_ids(f"{what} decode {i}", tok, lg, ref[order, 1 + i], "bf16")


def _raw(st, slots, lens, pasts, x, out, flags=bs.BS_STEP_HOST_IO):
    step = bs.Stage._ragged_step(slots, lens, pasts, flags)
    return bs.lib().bs_forward_ragged(st._h, ctypes.byref(step), bs._ptr(x), bs._ptr(out), None, None)


def test_statuses():
    assert bs.lib().bs_abi_version() == 5
    ids, x = np.zeros(64, np.int32), np.zeros((64, 64), np.float32)
    out = np.empty(8, np.int32)
    kw = dict(max_batch=4, max_ctx=16, max_tokens=16, seed=1)
    ok = Stage(64, 4, 2, 512, 0, 2, dtype="bf16", **kw)
    assert _raw(ok, [0, 2], [3, 5], [0, 0], ids, out) == 0
    assert _raw(ok, [0, 2], [8, 9], [0, 0], ids, out) == -1              # T > max_tokens
    assert _raw(ok, [1, 1], [2, 2], [0, 0], ids, out) == -1              # a slot named twice
    assert _raw(ok, [0, 4], [2, 2], [0, 0], ids, out) == -1              # a slot outside max_batch
    assert _raw(ok, [0, 1], [2, 3], [0, 14], ids, out) == -1             # past + S > max_ctx
    assert _raw(ok, [0], [2], [0], ids, out, bs.BS_STEP_HOST_IO | bs.BS_STEP_VERIFY) == -1
    null = RaggedStep(1, bs.BS_STEP_HOST_IO, None, None, None)
    assert bs.lib().bs_forward_ragged(ok._h, ctypes.byref(null), bs._ptr(ids), bs._ptr(out), None, None) == -1
    assert _raw(Stage(64, 4, 2, 512, 0, 2, dtype="fp32", **kw), [0], [2], [0], ids, out) == -5
    assert _raw(Stage(64, 4, 2, 512, 0, 2, dtype="bf16", kv_int8=True, **kw), [0], [2], [0], ids, out) == -5
    assert _raw(Stage(64, 4, 2, 512, 1, 2, dtype="bf16", n_labels=2, **kw), [0], [2], [0], x, out) == -4
    ok.set_sampling(4, 1.0, 7)
    assert _raw(ok, [0], [2], [0], ids, out) == -4                       # bs_set_sampling top_k > 1
    ok.set_sampling(1)
    ok.set_row_sampler(2, top_k=4, seed=3)
    assert _raw(ok, [2], [2], [0], ids, out) == -4                       # a row with sampler state
    assert _raw(ok, [3, 0], [2, 1], [0, 3], ids, out) == 0               # other rows: the stage still works
    assert ok.forward_host(ids[:4], 4, 1, past_len=[4, 0, 0, 2]).shape == (4,)


def test_workspace_grows_at_the_first_ragged_call_only():
    h, nh, L, V, T, mb = 64, 4, 1, 2048, 200, 3
    st = Stage(h, nh, L, V, 0, L, dtype="bf16", max_batch=mb, max_ctx=256, max_tokens=T, seed=3)
    ids = gen_np.prompt_ids(9, 1, T, V).astype(np.int32)[0]
    before = st.info()["workspace_bytes"]
    st.forward_host(ids[:8], 1, 8, past_len=0)
    assert st.info()["workspace_bytes"] == before
    st.forward_ragged_host(ids[:12], [2, 0], [3, 9], [0, 8])
    a256 = lambda n: (n + 255) // 256 * 256
    grown = st.info()["workspace_bytes"] - before
    # K and V staging [n_head][max_tokens][hd] bf16, the rows (16 B each) and the work list (8 B an item)
    assert grown == 2 * a256(T * h * 2) + a256(mb * 16) + a256((mb + T // 64 + 1) * 8)
    st.forward_ragged_host(ids, [1], [T], [0])
    st.forward_ragged_host(ids[:3], [0, 1, 2], [1, 1, 1], [17, 200, 3])
    assert st.info()["workspace_bytes"] == before + grown
