"""tools/guide_bench.py — what guided decoding costs a decode step.

Layer-free bf16 last stages (ln_f + the tied lm_head + the tail) at bloom-1b1 and bloom-7b1 width, V = 250 880, and at
bloom-1b1 width with V = 512 (a default-allow state must cost the same at both), B = 1 and 32, decode steps on device
buffers (graph replay).  The yardsticks are the parent commit's routes: the `rows p=1` step (every row holds a sampler
with top_p = 1) for sampled steps and the processed greedy step (every row holds a repetition penalty and a history of
64 tokens, no sampler: TAIL_ROWS_PROC) for processed greedy steps.  Against each, the same rows guided as well, every
row in one of three kinds of state, each looping to itself so that the state stays put over a round:
  one       default-ban, one allowed token
  1000      default-ban, 1000 random allowed tokens (V = 512: 256)
  allow-64  default-allow, 64 random explicit bans
and the guide apply launch (bs_guide_logits on a device buffer, B rows) and the advance launch (bs_advance_row_guide of
one device token into one row) alone.

A timing is one round: the rows' state is set afresh (untimed), then STEPS steps run back to back between two device
events; a column is the median (min, max) of ROUNDS rounds, routes alternating inside a round so that drift hits every
column alike.

    python tools/guide_bench.py --out profiles/guided_decoding_ab.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributed_inference_demo_amd.guide import Guide  # noqa: E402
from distributed_inference_demo_amd.stage import Stage  # noqa: E402

CONFIGS = (("bloom-1b1", 1536, 16, 250880), ("bloom-7b1", 4096, 32, 250880), ("bloom-1b1", 1536, 16, 512))
BATCHES = (1, 32)
KINDS = ("one", "1000", "allow-64")
ROUNDS, STEPS, WARM = 20, 10, 3
HISTORY = 64


def bench_guide(V, rng):
    """Three states, one per kind, each looping to itself."""
    many = np.sort(rng.choice(V, size=min(1000, V // 2), replace=False))
    bans = np.sort(rng.choice(V, size=64, replace=False))
    tok = [int(V // 3)] + many.tolist() + bans.tolist()
    nxt = [0] + [1] * many.size + [-1] * bans.size
    return Guide(3, 0, [0, 1, 1 + many.size, len(tok)], tok, nxt, [-1, -1, 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "guided_decoding_ab.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cs = torch.cuda.Stream()
    sh = cs.cuda_stream
    rng = np.random.default_rng(0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, h, nh, V in CONFIGS:
        g = Stage(h, nh, 2, V, 0, 0, dtype="bf16", max_batch=max(BATCHES), max_ctx=HISTORY + (WARM + 2) * STEPS + 8,
                  seed=1, is_first=False, is_last=True)
        gid = g.load_guide(bench_guide(V, rng).validate(V))
        for B in BATCHES:
            x = torch.randn((B, 1, h), dtype=torch.float32, device=dev)
            tok = torch.empty(B, dtype=torch.int32, device=dev)
            lg = torch.empty((B, V), dtype=torch.float32, device=dev)
            one = torch.full((1,), V // 3, dtype=torch.int32, device=dev)
            hist = [rng.integers(0, V, size=HISTORY).astype(np.int32) for _ in range(B)]

            def prepare(route):
                """Untimed: the stage's state for `route` (every row alike)."""
                kind = route[0]
                g.clear_row_sampler(stream=sh)
                g.clear_row_processor(stream=sh)
                g.clear_row_guide(stream=sh)
                if "rows" in kind:
                    g.set_row_sampler(0, top_p=1.0, temperature=1.0, seed=7, count=B, stream=sh)
                if "proc" in kind:
                    g.set_row_processor(0, count=B, stream=sh, repetition_penalty=1.3)
                    for r in range(B):
                        g.note_tokens(r, hist[r], stream=sh)
                if len(route) > 1:
                    g.set_row_guide(0, gid, states=KINDS.index(route[1]), count=B, stream=sh)

            def run(route):
                for _ in range(STEPS):
                    if route[0] == "apply":
                        g.guide_logits(lg, slot=0, batch=B, stream=sh)
                    elif route[0] == "advance":
                        g.advance_row_guide(0, one, n=1, stream=sh)
                    else:
                        g.forward(x, tok, B, 1, slot=0, past_len=0, stream=sh)

            routes = [("rows",), ("proc",)]
            for k in KINDS:
                routes += [("guide+rows", k), ("guide+proc", k), ("apply", k)]
            routes.append(("advance", "one"))
            times = {r: [] for r in routes}
            torch.cuda.synchronize()
            with torch.cuda.stream(cs):
                for rnd in range(WARM + ROUNDS):
                    for route in routes:
                        prepare(route)
                        if rnd == 0:  # captures and first launches stay out of every timing
                            run(route)
                            prepare(route)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(cs)
                        run(route)
                        e1.record(cs)
                        e1.synchronize()
                        if rnd >= WARM:
                            times[route].append(e0.elapsed_time(e1) * 1000.0 / STEPS)
                prepare(("none",))
            emit(f"# {name} width (hidden {h}), layer-free bf16 last stage, V {V}, B = {B}; graph-replayed decode steps, "
                 f"{ROUNDS} rounds of {STEPS} steps, routes alternating; us per step (or per launch), device events: "
                 "median min max")
            med = {}
            for route in routes:
                t = np.array(times[route])
                med[route] = float(np.median(t))
                label = {"rows": "rows p=1 step (yardstick, sampled)",
                         "proc": "processed greedy step (yardstick, TAIL_ROWS_PROC)",
                         "guide+rows": "guided rows p=1 step", "guide+proc": "guided processed greedy step",
                         "apply": f"guide apply launch alone ({B} rows)",
                         "advance": "guide advance launch alone (1 row, 1 token)"}[route[0]]
                if len(route) > 1:
                    label += f" [{route[1]}]"
                emit(f"{label:<62s}{med[route]:10.1f}{t.min():10.1f}{t.max():10.1f}")
            for base, guided in (("rows", "guide+rows"), ("proc", "guide+proc")):
                spread = max(times[(base,)]) - min(times[(base,)])
                emit(f"added to the {base} step: " + ", ".join(f"{k}: {med[(guided, k)] - med[(base,)]:+.1f} us" for k in KINDS)
                     + f" (the yardstick's own min-max spread: {spread:.1f} us)")
            emit()
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
