"""sample_bench.py — what the per-row sampler costs against the other tail picks and against the lm_head GEMV.

    python tools/sample_bench.py --rounds 20 --out profiles/row_sampler_ab.txt

One process.  Per width (bloom-1b1: hidden 1536, bloom-7b1: hidden 4096) two layer-free first + last bf16 stages with
the real vocabulary (250 880): a decode step is the embedding LayerNorm, ln_f fused into the lm_head GEMV, and the
pick, so the step time is the tail of a real decode step.  Routes, alternating inside every round, graph-replayed,
device events on one stream, medians over the rounds, B in {1, 8, 32} rows:
  greedy        full head + argmax_finalize (head screening off)
  topk16        full head + topk_sample_kernel at k = 16 (bs_set_sampling)
  rows p=0.9    full head + the row sampler, every row at (top_k 0, top_p 0.9, temperature 1)
  rows p=1      ... at (0, 1, 1)
  rows k=50     ... at (50, 0.95, 1): the count passes run too
and, eagerly launched back to back, `sampler alone`: bs_sample_logits on the step's own logits at (0, 0.9, 1).
`gemv` is the lm_head GEMV's own time (bs_profile_enable class 1, eager launches).  The table prints every route's
step and step - gemv: the embedding LayerNorm plus the pick.
"""
import argparse
import os
import statistics
import sys

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

V = 250880
WIDTHS = (("bloom-1b1", 1536, 16), ("bloom-7b1", 4096, 32))
BATCHES = (1, 8, 32)
INNER = 8


def bench_width(name, h, nh, rounds, dev, lines):
    mk = lambda: Stage(h, nh, 2, V, 0, 0, dtype="bf16", max_batch=max(BATCHES), max_ctx=INNER + 2, seed=1,  # noqa: E731
                       is_first=True, is_last=True)
    a, b = mk(), mk()
    a.set_head_screen(False)
    b.set_sampling(16, 1.0, 7)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lg = torch.empty((max(BATCHES), V), dtype=torch.float32, device=dev)

    def timed(fn, n):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for i in range(n):
                fn(i)
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n  # us per call

    for B in BATCHES:
        ids = torch.from_numpy(prompt_ids(3, 1, B, V).reshape(-1).copy()).to(dev)
        out = torch.empty(B, dtype=torch.int32, device=dev)

        def rows(k, p):  # the states change between the timings, stream-ordered, and no graph is dropped
            return lambda: a.set_row_sampler(0, top_k=k, top_p=p, temperature=1.0, seed=list(range(B)), count=B,
                                             stream=sh)

        step_a = lambda i: a.forward(ids, out, B, 1, past_len=i, stream=sh)  # noqa: E731
        routes = {"greedy": (lambda: a.clear_row_sampler(stream=sh), step_a),
                  "topk16": (None, lambda i: b.forward(ids, out, B, 1, past_len=i, stream=sh)),
                  "rows p=0.9": (rows(0, 0.9), step_a), "rows p=1": (rows(0, 1.0), step_a),
                  "rows k=50": (rows(50, 0.95), step_a)}
        with torch.cuda.stream(stream):  # the step's own logits, for the sampler alone
            a.clear_row_sampler(stream=sh)
            a.forward(ids, out, B, 1, past_len=0, logits=lg, stream=sh)
            a.set_row_sampler(0, top_k=0, top_p=0.9, temperature=1.0, seed=list(range(B)), count=B, stream=sh)
        routes["sampler alone (eager)"] = (rows(0, 0.9), lambda i: a.sample_logits(lg, list(range(i, i + B)), slot=0,
                                                                                   tokens=out, stream=sh))
        t = {k: [] for k in routes}
        for r in range(rounds + 3):  # warm-up rounds: captures, code objects
            for k, (setup, fn) in routes.items():
                if setup:
                    with torch.cuda.stream(stream):
                        setup()
                us = timed(fn, INNER)
                if r >= 3:
                    t[k].append(us)
        torch.cuda.synchronize()
        a.clear_row_sampler(stream=sh)
        a.profile_enable(1)
        with torch.cuda.stream(stream):
            for i in range(INNER):
                a.forward(ids, out, B, 1, past_len=i, stream=sh)
        ms, n, _ = a.profile_read()
        a.profile_enable(0)
        gemv = ms * 1e3 / max(n, 1)
        lines.append(f"{name} (hidden {h}), V = {V}, B = {B}: lm_head GEMV alone {gemv:8.1f} us ({n} launches)")
        for k, v in t.items():
            med = statistics.median(v)
            tail = "" if k.startswith("sampler") else f"  step - gemv {med - gemv:8.1f} us"
            lines.append(f"    {k:24s} {med:8.1f} us  (min {min(v):8.1f}, max {max(v):8.1f}){tail}"
                         + (f"  = {med / gemv:5.2f} x gemv" if k.startswith("sampler") else ""))
        print("\n".join(lines[-(len(t) + 1):]), flush=True)
    a.close()
    b.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"sample_bench: medians of {args.rounds} rounds, {INNER} consecutive steps per timing, us per step"]
    for name, h, nh in WIDTHS:
        bench_width(name, h, nh, args.rounds, dev, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
