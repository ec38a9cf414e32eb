"""tools/logit_proc_bench.py — what the per-row logit processors cost a decode step.

Layer-free bf16 last stages (ln_f + the tied lm_head + the tail) at bloom-1b1 and bloom-7b1 width, V = 250 880, B = 1,
8 and 32, decode steps on device buffers (graph replay).  Per (width, B): the greedy screened step (B <= 2 only), the
greedy full-head step, the `rows p=1` step (every row holds a sampler with top_p = 1: the route of a processed step
without its two launches -- its code is the parent commit's, so this column is the yardstick), and per history length
64 / 1024 / 2048 the processed step with the penalty only and with penalty, n = 3 and 16 bias entries -- greedy (rows
without sampler state, which leave the sampler's six selection launches at once) and, for the yardstick's difference,
with the `rows p=1` sampler as well -- and the apply and note launches alone (bs_process_logits on a device buffer;
bs_note_tokens of one device token into one row).

A timing is one round: the rows' state is set and their history noted afresh (untimed), then STEPS steps run back to
back between two device events; a column is the median (min, max) of ROUNDS rounds, routes alternating inside a round
so that drift hits every column alike (the screened step runs in rounds of its own, before the others: switching the
screen drops the captured graphs).  The history grows by one token a step, STEPS tokens a round at most.

    python tools/logit_proc_bench.py --out profiles/logit_processors_ab.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributed_inference_demo_amd.stage import Stage  # noqa: E402

V = 250880
WIDTHS = (("bloom-1b1", 1536, 16), ("bloom-7b1", 4096, 32))
BATCHES = (1, 8, 32)
HISTORIES = (64, 1024, 2048)
ROUNDS, STEPS, WARM = 20, 10, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "logit_processors_ab.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    sh = cs.cuda_stream
    rng = np.random.default_rng(0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, h, nh in WIDTHS:
        max_ctx = max(HISTORIES) + (WARM + 1) * STEPS + 8
        g = Stage(h, nh, 2, V, 0, 0, dtype="bf16", max_batch=max(BATCHES), max_ctx=max_ctx, seed=1, is_first=False,
                  is_last=True)
        bias16 = [(int(t), 0.25) for t in rng.choice(V, size=16, replace=False)]
        states = {"penalty": dict(repetition_penalty=1.3),
                  "pen+n3+16bias": dict(repetition_penalty=1.3, no_repeat_ngram=3, bias=bias16)}
        for B in BATCHES:
            x = torch.randn((B, 1, h), dtype=torch.float32, device=dev)
            tok = torch.empty(B, dtype=torch.int32, device=dev)
            lg = torch.empty((B, V), dtype=torch.float32, device=dev)
            one = torch.zeros(1, dtype=torch.int32, device=dev)

            def step():
                g.forward(x, tok, B, 1, slot=0, past_len=0, stream=sh)

            def prepare(route, hist):
                """Untimed: the stage's state for `route` (every row alike)."""
                kind = route[0]
                g.clear_row_sampler(stream=sh)
                g.clear_row_processor(stream=sh)
                if kind in ("screened", "full"):
                    pass
                elif kind == "rows":
                    g.set_row_sampler(0, top_p=1.0, temperature=1.0, seed=7, count=B, stream=sh)
                else:
                    if kind == "proc+rows":
                        g.set_row_sampler(0, top_p=1.0, temperature=1.0, seed=7, count=B, stream=sh)
                    g.set_row_processor(0, count=B, stream=sh, **states[route[1]])
                    for r in range(B):
                        g.note_tokens(r, hist[r], stream=sh)

            def run(route):
                kind = route[0]
                if kind == "apply":
                    for _ in range(STEPS):
                        g.process_logits(lg, slot=0, batch=B, stream=sh)
                elif kind == "note":
                    for _ in range(STEPS):
                        g.note_tokens(0, one, n=1, generated=True, stream=sh)
                else:
                    for _ in range(STEPS):
                        step()

            routes = ([("screened",)] if B <= 2 else []) + [("full",), ("rows",)]
            for n in HISTORIES:
                routes += [("proc", "penalty", n), ("proc", "pen+n3+16bias", n), ("proc+rows", "penalty", n),
                           ("proc+rows", "pen+n3+16bias", n), ("apply", "pen+n3+16bias", n), ("note", "penalty", n)]
            hists = {n: [rng.integers(0, V, size=n).astype(np.int32) for _ in range(B)] for n in HISTORIES}
            times = {r: [] for r in routes}
            torch.cuda.synchronize()
            with torch.cuda.stream(cs):
                for group in ([routes[:1], routes[1:]] if B <= 2 else [routes]):
                    g.set_head_screen(group[0][0] == "screened")  # once a group: it drops the captured graphs
                    for rnd in range(WARM + ROUNDS):
                        for route in group:
                            hist = hists.get(route[2]) if len(route) > 2 else None
                            prepare(route, hist)
                            if rnd == 0:  # captures and first launches stay out of every timing
                                run(route)
                                prepare(route, hist)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(cs)
                            run(route)
                            e1.record(cs)
                            e1.synchronize()
                            if rnd >= WARM:
                                times[route].append(e0.elapsed_time(e1) * 1000.0 / STEPS)
                g.clear_row_sampler(stream=sh)
                g.clear_row_processor(stream=sh)
                g.set_head_screen(True)
            emit(f"# {name} width (hidden {h}), layer-free bf16 last stage, V {V}, B = {B}; graph-replayed decode steps, "
                 f"{ROUNDS} rounds of {STEPS} steps, routes alternating; us per step (or per launch), device events: "
                 "median min max")
            med = {}
            for route in routes:
                t = np.array(times[route])
                med[route] = float(np.median(t))
                label = {"screened": "greedy screened step", "full": "greedy full-head step", "rows": "rows p=1 step",
                         "proc": "processed greedy step", "proc+rows": "processed rows p=1 step",
                         "apply": "apply launch alone", "note": "note launch alone (1 row)"}[route[0]]
                if len(route) > 2:
                    label += f" [{route[1]}] history {route[2]}"
                emit(f"{label:<62s}{med[route]:10.1f}{t.min():10.1f}{t.max():10.1f}")
            for st in states:
                add = [med[("proc+rows", st, n)] - med[("rows",)] for n in HISTORIES]
                ratio = f"added time x{add[-1] / add[0]:.2f}" if add[0] > 0 else "the 64-token difference is inside the spread"
                emit(f"added to the rows p=1 step [{st}]: " + ", ".join(f"{n}: {d:+.1f} us" for n, d in zip(HISTORIES, add))
                     + f"; history x{HISTORIES[-1] // HISTORIES[0]} -> {ratio}")
            emit(f"rows p=1 step over greedy full-head step: {med[('rows',)] - med[('full',)]:+.1f} us (the sampled step's "
                 f"own overhead); processed greedy step [penalty, history 64] over greedy full-head step: "
                 f"{med[('proc', 'penalty', 64)] - med[('full',)]:+.1f} us")
            emit()
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
