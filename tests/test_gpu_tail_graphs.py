"""A captured graph is never replayed for a different tail.

One bf16 whole-model last stage at the smallest shape where every tail exists (hidden 64, 4 heads, 1 layer, vocab 512,
max_batch 4, max_ctx 32).  After a 4-token prefill of two rows, one fixed walk of calls on device buffers visits the
screened greedy tail, the full head, top-k, the row sampler (mixed rows), both verify tails and a scoring pass, re-using
the same buffers wherever two tails can share every other part of a graph's key.  Each decode and verify call is issued
twice (the second is a replay), the rows rolled back in between.  The same walk on a twin stage with graphs off must
give the same ids, logits (bit for bit), draw records and screening counts at every step, and the same info()."""
import numpy as np
import pytest
import torch

from distributed_inference_demo_amd.stage import Stage
from oracle import gen_np

pytestmark = pytest.mark.gpu

H, NH, L, V = 64, 4, 1, 512
PAST = 4
SAMPLER = dict(top_k=20, top_p=0.9, temperature=1.5, seed=77)


def walk(graphs):
    g = Stage(H, NH, L, V, 0, L, dtype="bf16", max_batch=4, max_ctx=32, seed=5)
    g.set_graphs(graphs)
    g.set_head_screen(True)
    g.forward_host(gen_np.prompt_ids(3, 2, PAST, V).astype(np.int32), 2, PAST, past_len=0)
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    rec = []
    with torch.cuda.stream(cs):
        sh = cs.cuda_stream
        ids = {(B, S): torch.from_numpy(gen_np.prompt_ids(40 + 8 * B + S, B, S, V).astype(np.int32)).to(dev)
               for B, S in ((1, 1), (2, 1), (2, 3))}
        tok = {k: torch.empty(k, dtype=torch.int32, device=dev) for k in ids}
        lg1 = torch.empty((1, V), dtype=torch.float32, device=dev)

        def screen_counts(B):
            ro = [g.read_head_screen(b) for b in range(B)]
            return [None if r is None else len(r["tiles"]) for r in ro]

        def call(what, B, S, logits=None, read=lambda: None, **kw):
            """The call twice on the same buffers; what it returned each time goes into the record."""
            for rep in range(2):
                tok[B, S].fill_(-1)
                if logits is not None:
                    logits.fill_(0)
                g.forward(ids[B, S], tok[B, S], B, S, slot=0, past_len=PAST, logits=logits, stream=sh, **kw)
                torch.cuda.synchronize()
                for b in range(B):
                    g.rollback(b, PAST)
                rec.append((what, rep, tok[B, S].cpu().numpy().copy(),
                            None if logits is None else logits.cpu().numpy().view(np.uint32).copy(),
                            screen_counts(B) if S == 1 else None, read()))
            return rec[-1]

        assert call("1 greedy B=1", 1, 1)[4] != [None]                   # screened
        assert call("2 greedy B=1 + logits", 1, 1, logits=lg1)[4] == [None]  # full head
        assert None not in call("3 greedy B=2", 2, 1)[4]
        g.set_sampling(top_k=4, temperature=0.8, seed=11)
        assert call("4 top-k B=2", 2, 1)[4] == [None, None]
        g.set_sampling(top_k=1)
        # other tokens in the same buffer from here on: what the screened tail left on the device at step 3 is stale
        ids[2, 1].copy_(torch.from_numpy(gen_np.prompt_ids(91, 2, 1, V).astype(np.int32)))
        g.set_row_sampler(1, stream=sh, **SAMPLER)
        draws = lambda: [g.read_row_draw(b) for b in range(2)]  # noqa: E731
        r6 = call("6 row sampler on row 1, B=2", 2, 1, read=draws)
        assert r6[4] == [None, None] and r6[5][1]["token"] == int(r6[2][1, 0])
        g.clear_row_sampler(stream=sh)
        # step 6's buffers and flags, step 3's tail: a replay of step 6's graph would rewrite the rows' draw records
        r7 = call("7 sampler cleared, B=2", 2, 1, read=draws)
        assert None not in r7[4] and r7[5] == r6[5]
        call("8 verify S=3", 2, 3, verify=True)
        g.set_row_sampler(1, stream=sh, **SAMPLER)
        r9 = call("9 verify-draw S=3", 2, 3, verify=True, draw=True,
                  read=lambda: [g.read_verify_draw(b, t) for b in range(2) for t in range(3)])
        assert [d["token"] for d in r9[5]] == r9[2].reshape(-1).tolist()
        top = torch.empty((2, 3), dtype=torch.int32, device=dev)
        sc = torch.empty((2, 3, 3), dtype=torch.float32, device=dev)
        g.score(ids[2, 3], None, top, sc, 2, 3, slot=0, past_len=PAST, stream=sh)
        torch.cuda.synchronize()
        rec.append(("10 score", 0, top.cpu().numpy().copy(), sc.cpu().numpy().view(np.uint32).copy(), None, None))
    info = g.info()
    g.close()
    return rec, info


def test_replayed_graphs_match_eager_launches_for_every_tail():
    captured, info_c = walk(True)
    eager, info_e = walk(False)
    assert len(captured) == len(eager) == 2 * 8 + 1  # eight decode / verify calls twice, one scoring pass
    for c, e in zip(captured, eager):
        what = f"{c[0]} (call {c[1]})"
        assert c[0] == e[0] and c[1] == e[1]
        assert np.array_equal(c[2], e[2]), f"{what}: ids {c[2].tolist()} captured, {e[2].tolist()} eager"
        assert (c[3] is None) == (e[3] is None) and (c[3] is None or np.array_equal(c[3], e[3])), f"{what}: logits differ"
        assert c[4] == e[4], f"{what}: screening counts {c[4]} captured, {e[4]} eager"
        assert c[5] == e[5], f"{what}: draw records differ"
    assert info_c == info_e
