"""tree_verify_bench.py — what a tree verify pass costs against the chain verify pass and the decode step.

    python tools/tree_verify_bench.py --model bloom-1b1 --ctx 1024 --rounds 24 --out-dir profiles

One process, one full-depth bf16 stage with synthetic weights, batch 1, a warm cache of --ctx positions.  The routes
alternate inside every round, device events on the stage's stream, medians over the rounds
(<out-dir>/tree_verify_ab.txt):
  (a) the graph-replayed decode step (S = 1; --inner consecutive steps at advancing positions, per step),
  (b) the BS_STEP_VERIFY pass at S = 8 (graph-replayed),
  (c) the graph-replayed tree pass at N = 8 and N = 16 (a branching-factor-2 tree; the mask does not change the work),
  (d) bs_compact_kv of a 4-node path with gaps.
Reported: c(8) / b and c(16) / a with the min .. max spread of the ratios' operands.  Acceptance on real text cannot
be measured here: synthetic weights echo the last token.
"""
import argparse
import os
import statistics
import sys

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402


def bench(m, st, ctx, rounds, inner, dev, lines):
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ids = torch.from_numpy(prompt_ids(99, 1, 16, m.vocab).reshape(-1).copy()).to(dev)
    out = torch.empty(16, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, n=1):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for i in range(n):
                fn(i)
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n  # us per call

    def tree(N):
        return [[-1] + [(i - 1) // 2 for i in range(1, N)]]

    routes = {"a decode S=1 (graph)": lambda i: st.forward(ids, out, 1, 1, past_len=ctx + i, stream=sh),
              "b verify S=8 (graph)": lambda i: st.forward(ids, out, 1, 8, past_len=ctx, stream=sh, verify=True)}
    for N in (8, 16):
        routes[f"c tree N={N} (graph)"] = lambda i, N=N: st.forward_tree(ids, out, tree(N), past_len=[ctx], stream=sh)
    routes["d compact_kv 4 of 16"] = lambda i: st.compact_kv(0, ctx + 1, [1, 4, 9, 14], stream=sh)
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
    a, b = "a decode S=1 (graph)", "b verify S=8 (graph)"
    for name, num, den in (("tree N=8 / verify S=8", "c tree N=8 (graph)", b), ("tree N=16 / decode step", "c tree N=16 (graph)", a),
                           ("tree N=16 / verify S=8", "c tree N=16 (graph)", b)):
        lines.append(f"{name:30s} {med[num] / med[den]:9.3f}  (spread {min(t[num]) / max(t[den]):.3f} .. "
                     f"{max(t[num]) / min(t[den]):.3f})")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="bloom-1b1")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out-dir", default="profiles")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("tree_verify_bench needs the GPU: nothing is measured without it")
    dev = torch.device("cuda", 0)
    m = config.get(a.model)
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=1, max_ctx=a.ctx + 32,
               max_tokens=a.ctx, seed=a.seed)
    st.forward_host(prompt_ids(1234, 1, a.ctx, m.vocab), 1, a.ctx, past_len=0)  # the warm cache
    os.makedirs(a.out_dir, exist_ok=True)
    lines = []
    bench(m, st, a.ctx, a.rounds, a.inner, dev, lines)
    with open(os.path.join(a.out_dir, "tree_verify_ab.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
