"""spec_bench.py — what a verify pass costs against a decode step, and speculative decoding end to end.

    python tools/spec_bench.py --model bloom-1b1 --ctx 1024 --rounds 24 --out-dir profiles

One process, one full-depth bf16 stage with synthetic weights, batch 1, a warm cache of --ctx positions.

Part 1 (<out-dir>/spec_verify_ab.txt), the routes alternating inside every round, device events on the stage's
stream, medians over the rounds:
  (a) the graph-replayed decode step (S = 1; --inner consecutive steps at advancing positions, per step),
  (b) the flagged verify pass at S in {2, 4, 5, 8} (graph-replayed, positions set ahead of each replay),
  (c) the unflagged pass of the same S at the same position: eager launches, the prefill attention.
r(S) = (b) / (a).  The gate: r(5) < 5 and r(8) < 8 -- otherwise even a free drafter that is always right loses.

Part 2 (<out-dir>/spec_decode_ab.txt): tokens/s of SpeculativeDecoder against the plain greedy decode of the same
stage in the same harness (StageChain: one host round trip per step or pass, so both sides pay the same host cost;
bench.py's pipelined decode is faster than either), with a replay drafter that proposes the target's own
continuation (the upper bound), the int8-weight self-draft, and the n-gram drafter.  Synthetic weights echo the
last token, so acceptance here says nothing about real text.
"""
import argparse
import os
import statistics
import sys
import time

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.speculative import (NgramDrafter, SpeculativeDecoder, StageChain,  # noqa: E402
                                                        StageDrafter)
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

S_LIST = (2, 4, 5, 8)


class ReplayDrafter:
    """Proposes the target's own continuation (recorded from a plain decode): always right."""

    def __init__(self, truth, prompt_len):
        self.truth, self.n0 = truth, prompt_len

    def propose(self, history, k):
        done = len(history) - self.n0
        return self.truth[done:done + k]


def whole_stage(m, max_ctx, max_tokens, seed, int8=False):
    return Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=1, max_ctx=max_ctx,
                 max_tokens=max_tokens, seed=seed, int8_weights=int8)


def verify_ab(m, st, ctx, rounds, inner, dev, lines):
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ids = torch.from_numpy(prompt_ids(99, 1, 8, m.vocab).reshape(-1).copy()).to(dev)
    out = torch.empty(8, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, n=1):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for i in range(n):
                fn(i)
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n  # us per call

    routes = {"a decode S=1 (graph)": lambda i: st.forward(ids, out, 1, 1, past_len=ctx + i, stream=sh)}
    for S in S_LIST:
        routes[f"b verify S={S} (graph)"] = lambda i, S=S: st.forward(ids, out, 1, S, past_len=ctx, stream=sh,
                                                                      verify=True)
        routes[f"c unflagged S={S} (eager)"] = lambda i, S=S: st.forward(ids, out, 1, S, past_len=ctx, stream=sh)
    t = {k: [] for k in routes}
    for r in range(rounds + 3):  # three warm-up rounds: captures, code objects
        for k, fn in routes.items():
            us = timed(fn, inner if k.startswith("a") else 1)
            if r >= 3:
                t[k].append(us)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"# {m.name} bf16, {m.n_layer} layers, B = 1, context {ctx}, {rounds} rounds, routes alternating; "
                 f"us per call, device events")
    lines.append(f"{'route':30s} {'median':>9s} {'min':>9s} {'max':>9s}")
    for k, v in t.items():
        lines.append(f"{k:30s} {med[k]:9.1f} {min(v):9.1f} {max(v):9.1f}")
    a = med["a decode S=1 (graph)"]
    for S in S_LIST:
        b, c = med[f"b verify S={S} (graph)"], med[f"c unflagged S={S} (eager)"]
        lines.append(f"r({S}) = b/a = {b / a:.3f}    b/c = {b / c:.3f}  (verify pass against today's eager pass)")
    r5, r8 = med["b verify S=5 (graph)"] / a, med["b verify S=8 (graph)"] / a
    lines.append(f"gate r(5) < 5 and r(8) < 8: {'PASS' if r5 < 5 and r8 < 8 else 'FAIL'} (r(5) = {r5:.3f}, r(8) = {r8:.3f})")
    lines.append("")


def decode_ab(m, st, prompt_len, new, k, reps, seed, lines):
    prompt = prompt_ids(1234, 1, prompt_len, m.vocab).reshape(-1).tolist()
    chain = StageChain([st])

    def plain():
        toks = [chain.prefill(prompt, 0)]
        t0 = time.perf_counter()
        for i in range(new - 1):
            toks.append(chain.step(toks[-1], prompt_len + i))
        return toks, (new - 1) / (time.perf_counter() - t0), None

    truth = plain()[0]
    draft_stage = whole_stage(m, prompt_len + new + 16, prompt_len + 8, seed, int8=True)  # its first catch-up: prompt + 1

    def spec(make):
        def run():
            dec = SpeculativeDecoder(chain, make(), k)
            t0 = time.perf_counter()
            toks, stats = dec.generate(prompt, new)
            dt = time.perf_counter() - t0
            assert toks == truth, "speculative decoding changed the tokens"
            return toks, new / dt, stats  # includes the prefill (as the drafters' first catch-up does)
        return run

    def plain_with_prefill():
        t0 = time.perf_counter()
        toks = [chain.prefill(prompt, 0)]
        for i in range(new - 1):
            toks.append(chain.step(toks[-1], prompt_len + i))
        return toks, new / (time.perf_counter() - t0), None

    routes = {"plain greedy decode": plain_with_prefill,
              "replay drafter (upper bound)": spec(lambda: ReplayDrafter(truth, prompt_len)),
              "int8-weight self-draft": spec(lambda: StageDrafter([draft_stage], k)),
              "n-gram drafter": spec(lambda: NgramDrafter(k))}
    res = {n: [] for n in routes}
    stats = {}
    for r in range(reps + 1):  # one warm-up repetition
        for n, fn in routes.items():
            _, tps, s = fn()
            if r:
                res[n].append(tps)
                stats[n] = s
    lines.append(f"# {m.name} bf16 B = 1, prompt {prompt_len}, {new} new tokens (prefill included), k = {k}, "
                 f"{reps} repetitions alternating; tokens/s, host clock around synchronous passes")
    base = statistics.median(res["plain greedy decode"])
    for n, v in res.items():
        s = stats[n]
        acc = "" if not s else (f"  passes {s['passes']} plain {s['plain_steps']} drafted {s['drafted']} accepted "
                                f"{s['accepted']} ({s['accepted'] / max(1, s['drafted']):.2f})")
        lines.append(f"{n:30s} {statistics.median(v):9.1f} tok/s  x{statistics.median(v) / base:.2f}{acc}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="bloom-1b1")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--new", type=int, default=192)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--skip-decode", action="store_true")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("spec_bench needs the GPU: nothing is measured without it")
    dev = torch.device("cuda", 0)
    m = config.get(a.model)
    st = whole_stage(m, a.ctx + a.new + 16, a.ctx, a.seed)
    ids = prompt_ids(1234, 1, a.ctx, m.vocab)
    st.forward_host(ids, 1, a.ctx, past_len=0)  # the warm cache
    os.makedirs(a.out_dir, exist_ok=True)
    lines = []
    verify_ab(m, st, a.ctx, a.rounds, a.inner, dev, lines)
    with open(os.path.join(a.out_dir, "spec_verify_ab.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    if not a.skip_decode:
        lines = []
        decode_ab(m, st, a.ctx, a.new, a.k, a.reps, a.seed, lines)
        with open(os.path.join(a.out_dir, "spec_decode_ab.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
