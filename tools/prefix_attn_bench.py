"""prefix_attn_bench.py — what the shared-prefix decode attention (bs_set_row_prefix, csrc/attn_prefix.hip) costs and saves.

    python tools/prefix_attn_bench.py --models bloom-7b1,bloom-1b1 --rounds 15 --out profiles/prefix_attention_ab.txt

One process per run, one full-depth bf16 stage per model with synthetic weights and 33 KV rows: a template row prefilled
once and forked into rows 0 .. 31.  Device events on one stream, the plain and the shared route alternating inside every
round (the declaration is set or cleared outside the timed span), graph-replayed S = 1 steps, --inner consecutive steps a
timing, medians over the rounds with min and max beside them (the run's own spread).

Part 1, per model, P in {256, 1024, 1984} and B in {4, 8, 32}: the decode step of B rows at context P + 20 (20 own
  positions per row), plain route against shared route, and the byte model's attention bytes per layer (B ctx against
  P + B (ctx - P) positions of K and V).  A shape reads GAIN when the shared route's median is below the plain route's
  and the two min .. max ranges do not overlap, LOSS the other way round, SAME when they overlap.
Part 2 (--beam): BeamSearcher W = 4 on the first model, tokens per second with and without prefix_attention.
"""
import argparse
import os
import statistics
import sys
import time

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.beam import BeamSearcher  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

ROWS, OWN = 32, 20
PREFIXES = (256, 1024, 1984)
BATCHES = (4, 8, 32)


def verdict(shared, plain):
    if max(shared) < min(plain):
        return "GAIN"
    return "LOSS" if min(shared) > max(plain) else "SAME (ranges overlap)"


def step_ab(m, rounds, inner, dev, lines):
    ctx_max = max(PREFIXES) + OWN
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=ROWS + 1,
               max_ctx=ctx_max + inner + 4, max_tokens=ctx_max, seed=3)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tmpl = torch.from_numpy(prompt_ids(7, 1, ctx_max, m.vocab).reshape(1, -1).copy()).to(dev)
    ids = torch.from_numpy(prompt_ids(99, 1, ROWS, m.vocab).reshape(-1).copy()).to(dev)
    out = torch.empty(ROWS, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        st.forward(tmpl, out, 1, ctx_max, slot=ROWS, past_len=0, stream=sh)
        st.fork_kv(ROWS, 0, npos=ctx_max, count=ROWS, stream=sh)
    lines.append(f"# {m.name} bf16, {m.n_layer} layers, {m.n_head} heads x {m.hidden // m.n_head}; graph-replayed decode "
                 f"steps, {rounds} rounds, routes alternating, {inner} steps a timing; us per step: median min max")
    lines.append(f"{'shape':24s} {'plain':>27s} {'shared':>27s}  shared/plain  attention MB/layer plain -> shared")

    def timed(B, ctx):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for i in range(inner):
                st.forward(ids, out, B, 1, slot=0, past_len=ctx + i, stream=sh)
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / inner

    for P in PREFIXES:
        for B in BATCHES:
            ctx = P + OWN
            t = {"plain": [], "shared": []}
            for r in range(rounds + 3):  # three warm-up rounds: captures, code objects
                for route in t:
                    st.set_row_prefix(0, ROWS, P if route == "shared" else 0, count=B, stream=sh)
                    us = timed(B, ctx)
                    if r >= 3:
                        t[route].append(us)
            st.set_row_prefix(0, ROWS, 0, count=ROWS, stream=sh)
            f = lambda v: f"{statistics.median(v):9.1f} {min(v):8.1f} {max(v):8.1f}"
            pos_bytes = m.hidden * 2 * 2 / 1e6  # K and V of one position, every head, bf16
            lines.append(f"P={P:<5d} B={B:<3d} ctx={ctx:<5d} {f(t['plain'])} {f(t['shared'])}  "
                         f"{statistics.median(t['shared']) / statistics.median(t['plain']):8.3f}      "
                         f"{B * (ctx + 1) * pos_bytes:8.1f} -> {(P + B * (ctx + 1 - P)) * pos_bytes:6.1f}  "
                         f"{verdict(t['shared'], t['plain'])}")
    lines.append("")
    st.close()


def beam_ab(m, dev, lines, W=4, prompt=1024, new=32):
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=W,
               max_ctx=prompt + new + 2, max_tokens=prompt, seed=3)
    ids = prompt_ids(11, 1, prompt, m.vocab).reshape(-1).tolist()
    lines.append(f"# {m.name} beam search W={W}, prompt {prompt}, {new} new tokens: tokens/s of the best hypothesis (3 runs)")
    for pa in (False, True, False, True):
        bs = BeamSearcher([st], W, prefix_attention=pa)
        st.reset(-1)  # the last searcher's declarations go with the rows
        bs.generate(ids, 4)  # captures
        tps = []
        for _ in range(3):
            st.reset(-1)
            t0 = time.perf_counter()
            seqs, _, _ = bs.generate(ids, new)
            tps.append(len(seqs[0]) / (time.perf_counter() - t0))
        lines.append(f"prefix_attention={int(pa)}: " + " ".join(f"{v:8.1f}" for v in tps))
    lines.append("")
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="bloom-7b1,bloom-1b1")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--beam", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    models = [config.get(n) for n in a.models.split(",")]
    for m in models:
        step_ab(m, a.rounds, a.inner, dev, lines)
        if a.out:  # keep what is measured so far
            open(a.out, "w").write("\n".join(lines) + "\n")
    if a.beam:
        beam_ab(models[-1], dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
