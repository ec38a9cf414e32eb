"""bs_fork_kv (Stage.fork_kv): positions [0, npos) of one KV row copied to other rows on the device -- an exact copy
that writes nothing else, on bf16, fp32 and int8 caches; rows forked from a prefilled row decode bit for bit like
rows that prefilled the prompt themselves, under graph replay and with no host synchronisation in between."""
import numpy as np
import pytest
import torch

from distributed_inference_demo_amd.stage import Stage, lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
H, NH, L, V, MB, CTX = 64, 4, 2, 512, 5, 21  # max_ctx odd: the int8 cache's scale segments start misaligned
KINDS = ["bf16", "fp32", "int8"]
RNG = np.random.default_rng(77)
PROMPT = RNG.integers(0, V, size=9).astype(np.int32)
SENTINELS = [RNG.integers(0, V, size=13).astype(np.int32) for _ in range(MB)]
OTHER = RNG.integers(0, V, size=6).astype(np.int32)


def make(kind, hidden=H, n_head=NH, n_layer=L, max_batch=MB, max_ctx=CTX, seed=21, **kw):
    return Stage(hidden, n_head, n_layer, V, 0, n_layer, dtype="fp32" if kind == "fp32" else "bf16",
                 max_batch=max_batch, max_ctx=max_ctx, seed=seed, kv_int8=kind == "int8", **kw)


def snapshot(st, n_layer=L, max_batch=MB, max_ctx=CTX):
    """Every row, every layer, positions [0, max_ctx): uint32 bits of [layer][row][K|V][head][pos][hd]."""
    return np.stack([np.stack([st.read_kv(l, r, 0, max_ctx) for r in range(max_batch)])
                     for l in range(n_layer)]).view(np.uint32)


def check_fork(before, after, src, dst, count, npos, max_batch):
    for r in range(max_batch):
        if dst <= r < dst + count:
            assert not np.array_equal(before[:, r, :, :, :npos], before[:, src, :, :, :npos]), "the case has no teeth"
            assert np.array_equal(after[:, r, :, :, :npos], before[:, src, :, :, :npos]), f"row {r}: copied positions"
            assert np.array_equal(after[:, r, :, :, npos:], before[:, r, :, :, npos:]), f"row {r}: positions >= npos"
        else:
            assert np.array_equal(after[:, r], before[:, r]), f"row {r} was written"


@pytest.fixture(scope="module", params=KINDS)
def stage(request):
    st = make(request.param)
    yield st
    st.close()


def fill(st, src):
    """The 9-token prompt in row `src`, a different 13-token prompt in every other row."""
    for r in range(MB):
        p = PROMPT if r == src else SENTINELS[r]
        st.forward_host(p.reshape(1, -1), 1, len(p), slot=r, past_len=0)


@pytest.mark.parametrize("src,dst,count,npos", [(3, 0, 3, 7), (3, 0, 3, 1), (3, 0, 3, 5), (3, 0, 3, 9), (3, 0, 3, 21),
                                                (0, 2, 2, 5), (3, 1, 1, 7), (0, 4, 1, 13)])
def test_fork_is_an_exact_copy_and_writes_nothing_else(stage, src, dst, count, npos):
    fill(stage, src)
    before = snapshot(stage)
    stage.fork_kv(src, dst, npos=npos, count=count)
    after = snapshot(stage)
    check_fork(before, after, src, dst, count, npos, MB)
    assert stage.past[dst:dst + count] == [npos] * count


@pytest.mark.parametrize("kind", KINDS)
def test_a_prefill_leaves_the_same_bits_in_any_slot(kind):
    """The premise of the decode test: the slot only offsets addresses."""
    a, b = make(kind), make(kind)
    a.forward_host(PROMPT.reshape(1, -1), 1, len(PROMPT), slot=0, past_len=0)
    b.forward_host(PROMPT.reshape(1, -1), 1, len(PROMPT), slot=2, past_len=0)
    for l in range(L):
        assert np.array_equal(a.read_kv(l, 0, 0, CTX).view(np.uint32), b.read_kv(l, 2, 0, CTX).view(np.uint32))
    a.close()
    b.close()


def _decode_run(st, forked, sh):
    """Prefill + three B = 4 graph-replayed decode steps + a row reuse + one more step; nothing synchronises until
    the end.  forked: rows 1..3 (then 1..2) come from fork_kv; else from their own prefills."""
    n = len(PROMPT)
    pd = torch.from_numpy(PROMPT.reshape(1, -1)).to(DEV)
    od = torch.from_numpy(OTHER.reshape(1, -1)).to(DEV)
    junk = torch.empty(1, dtype=torch.int32, device=DEV)
    xs = [torch.from_numpy(RNG_STEPS[i]).to(DEV) for i in range(4)]
    outs = [torch.full((4,), -7, dtype=torch.int32, device=DEV) for _ in range(4)]
    lgs = [torch.full((4, V), np.nan, dtype=torch.float32, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    st.forward(pd, junk, 1, n, slot=0, past_len=0, stream=sh)
    if forked:
        st.fork_kv(0, 1, count=3, stream=sh)
    else:
        for r in (1, 2, 3):
            st.forward(pd, junk, 1, n, slot=r, past_len=0, stream=sh)
    for i in range(3):
        st.forward(xs[i], outs[i], 4, 1, slot=0, past_len=n + i, logits=lgs[i], stream=sh)
    # rows 1..2 are taken by another prompt (5 of its 6 positions) while rows 0 and 3 keep decoding
    if forked:
        st.forward(od, junk, 1, len(OTHER), slot=4, past_len=0, stream=sh)
        st.fork_kv(4, 1, npos=5, count=2, stream=sh)
    else:
        for r in (1, 2):
            st.forward(od, junk, 1, len(OTHER), slot=r, past_len=0, stream=sh)
    st.forward(xs[3], outs[3], 4, 1, slot=0, past_len=[n + 3, 5, 5, n + 3], logits=lgs[3], stream=sh)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], [g.cpu().numpy().view(np.uint32) for g in lgs]


RNG_STEPS = [np.random.default_rng(5 + i).integers(0, V, size=4).astype(np.int32) for i in range(4)]


@pytest.mark.parametrize("kind", KINDS)
def test_forked_rows_decode_like_prefilled_rows_under_graph_replay(kind):
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a, b = make(kind), make(kind)
        ids_a, lg_a = _decode_run(a, True, stream.cuda_stream)
        ids_b, lg_b = _decode_run(b, False, stream.cuda_stream)
    for i in range(4):
        assert np.all((ids_b[i] >= 0) & (ids_b[i] < V))
        for r in range(4):
            assert ids_a[i][r] == ids_b[i][r], f"step {i} row {r}: ids"
            assert np.array_equal(lg_a[i][r], lg_b[i][r]), f"step {i} row {r}: logits"
    a.close()
    b.close()


@pytest.mark.parametrize("kind,hidden,n_head", [("bf16", 1024, 16), ("int8", 1024, 16), ("bf16", 320, 4)])
def test_fork_at_real_width(kind, hidden, n_head):
    """hd 64 (and hd 80): 130 of 200 positions, two destinations, one layer."""
    mb, ctx, npos = 4, 200, 130
    st = make(kind, hidden=hidden, n_head=n_head, n_layer=1, max_batch=mb, max_ctx=ctx, max_tokens=160)
    rng = np.random.default_rng(3)
    for r, n in enumerate((150, 140, 150, 150)):  # row 1 is the source
        st.forward_host(rng.integers(0, V, size=(1, n)).astype(np.int32), 1, n, slot=r, past_len=0)
    before = snapshot(st, 1, mb, ctx)
    st.fork_kv(1, 2, npos=npos, count=2)
    check_fork(before, snapshot(st, 1, mb, ctx), 1, 2, 2, npos, mb)
    st.close()


def test_statuses(stage):
    f, h = lib().bs_fork_kv, stage._h
    assert lib().bs_abi_version() == 5
    assert f(None, 0, 1, 1, 1, None) == -1
    for args in [(-1, 0, 1, 1), (0, -1, 1, 1), (0, 1, -1, 1), (0, 1, 1, -1),      # negative
                 (MB, 0, 1, 1), (0, MB, 1, 1), (0, 3, 3, 1), (0, 1, MB, 1),        # outside max_batch
                 (0, 1, 1, CTX + 1),                                                  # beyond max_ctx
                 (0, 0, 1, 1), (2, 0, 3, 1), (2, 2, 1, 1), (4, 2, 3, 1)]:            # the source among the destinations
        assert f(h, *args, None) == -1, args
    fill(stage, 3)
    info, before = stage.info(), snapshot(stage)
    assert f(h, 3, 0, 3, 0, None) == 0 and f(h, 3, 0, 0, 7, None) == 0  # nothing to copy
    assert np.array_equal(snapshot(stage), before)
    assert f(h, 3, 0, 3, CTX, None) == 0  # the whole row
    assert stage.info() == info


def test_a_stage_without_layers_has_nothing_to_copy():
    st = Stage(H, NH, L, V, 0, 0, dtype="bf16", max_batch=3, max_ctx=8, seed=1, is_first=False, is_last=True)
    assert lib().bs_fork_kv(st._h, 0, 1, 2, 5, None) == 0
    assert lib().bs_fork_kv(st._h, 0, 0, 1, 5, None) == -1
    st.close()
