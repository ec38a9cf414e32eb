"""lora_bench.py — what per-row LoRA adapters (bs_set_row_adapter, csrc/lora.hip) add to a decode step.

    python tools/lora_bench.py --models bloom-1b1,bloom-7b1 --rounds 15 --out profiles/lora_ab.txt

One process per run, one full-depth bf16 stage per model with synthetic weights.  Device events on one stream, the plain
and the adapted step alternating inside every round (the rows' adapters are set or cleared outside the timed span),
graph-replayed S = 1 steps at context 128 of max_ctx 512 (8 chunks: at B = 1 the decode attention splits and the dense
GEMV merges the partials in its prologue, so the adapted step holds the ctx merge launch too), --inner consecutive steps a timing, medians over the rounds with min and max
beside them (the run's own spread).  Per model, rank in {16, 64} and B in {1, 8, 32}: every row on its own adapter
(adapter b % 16), all three targets.  The plain step is the same build's step of rows that name no adapter: the launches
and bits of a stage that never loaded one.  Reported: us per step, us added per step and per layer.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lora_bench.py --trace bloom-1b1

--trace MODEL runs adapted steps only (rank 16, B = 8, 50 graph replays behind a prefill of the 8 rows), for a
kernel trace in a run of its own: the share of lora_shrink_kernel + lora_expand_kernel in the trace's kernel time.
"""
import argparse
import os
import statistics
import sys

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config, lora  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

ROWS, CTX, MAX_CTX = 32, 128, 512
RANKS = (16, 64)
BATCHES = (1, 8, 32)


def bench(m, rounds, inner, dev, lines):
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines.append(f"# {m.name} bf16, {m.n_layer} layers, hidden {m.hidden}; graph-replayed decode steps at context {CTX}, "
                 f"{rounds} rounds, plain / adapted alternating, {inner} steps a timing; us per step: median min max")
    lines.append(f"{'shape':20s} {'plain':>27s} {'adapted':>27s}  added us/step  us/layer  adapted/plain")
    for rank in RANKS:
        st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=ROWS,
                   max_ctx=MAX_CTX, max_tokens=ROWS * CTX, seed=3)
        n_ad = 16
        for k in range(n_ad):  # one adapter's host arrays at a time
            st.load_adapter(lora.synthetic(k, rank, lora.TARGETS, m.hidden, m.n_layer, 0.05))
        ids = torch.from_numpy(prompt_ids(7, ROWS, CTX, m.vocab).copy()).to(dev)
        tok = torch.from_numpy(prompt_ids(99, 1, ROWS, m.vocab).reshape(-1).copy()).to(dev)
        out = torch.empty(ROWS, dtype=torch.int32, device=dev)
        with torch.cuda.stream(stream):
            st.forward(ids, out, ROWS, CTX, past_len=0, stream=sh)

        def timed(B):
            with torch.cuda.stream(stream):
                for i in range(2):  # the first replay of a shape captures
                    st.forward(tok[:B], out[:B], B, 1, past_len=CTX + i, stream=sh)
                ev[0].record(stream)
                for i in range(inner):
                    st.forward(tok[:B], out[:B], B, 1, past_len=CTX + 2 + i, stream=sh)
                ev[1].record(stream)
            stream.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / inner

        for B in BATCHES:
            t = {False: [], True: []}
            for _ in range(rounds):
                for on in (False, True):
                    for b in range(B):
                        st.set_row_adapter(b, b % n_ad if on else -1, stream=sh)
                    t[on].append(timed(B))
            med = {on: statistics.median(v) for on, v in t.items()}
            fmt = lambda v: f"{statistics.median(v):9.1f} {min(v):8.1f} {max(v):8.1f}"
            add = med[True] - med[False]
            lines.append(f"r={rank:<3d} B={B:<3d}          {fmt(t[False])} {fmt(t[True])}  {add:13.1f}  {add / m.n_layer:8.2f}  "
                         f"{med[True] / med[False]:13.3f}")
            print(lines[-1], flush=True)
        st.close()


def trace(m, dev, steps=50, B=8, rank=16):
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=B, max_ctx=MAX_CTX,
               max_tokens=B * CTX, seed=3)
    for k in range(B):
        st.set_row_adapter(k, st.load_adapter(lora.synthetic(k, rank, lora.TARGETS, m.hidden, m.n_layer, 0.05)))
    stream = torch.cuda.Stream(dev)
    ids = torch.from_numpy(prompt_ids(7, B, CTX, m.vocab).copy()).to(dev)
    out = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        st.forward(ids, out, B, CTX, past_len=0, stream=stream.cuda_stream)
        for i in range(steps):
            st.forward(ids[:, 0].contiguous(), out, B, 1, past_len=CTX + i, stream=stream.cuda_stream)
    stream.synchronize()
    print(f"traced {steps} adapted decode steps of {m.name}, B = {B}, rank {rank}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None, help="MODEL: adapted steps only, for a kernel trace")
    ap.add_argument("--models", default="bloom-1b1,bloom-7b1")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.trace:
        return trace(config.get(a.trace), dev)
    lines = []
    for name in a.models.split(","):
        bench(config.get(name), a.rounds, a.inner, dev, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
