"""spec_sample_bench.py — what a verify-draw pass costs against a sampled decode step (spec_bench.py's part 1 for
sampled speculative decoding).

    python tools/spec_sample_bench.py --model bloom-1b1 --ctx 1024 --rounds 24 --out-dir profiles

One process, one full-depth bf16 stage with synthetic weights and two KV rows, both warm with --ctx positions: row 0
holds a sampler state (top_k 50, top_p 0.9, temperature 1), row 1 none.  Every route runs at batch 1 on device
buffers and replays its captured graph; the routes alternate inside every round, device events on the stage's stream,
medians over the rounds (<out-dir>/spec_sample_ab.txt):
  (a) the sampled decode step on row 0 (S = 1; --inner consecutive steps at advancing positions, per step),
  (g) the greedy decode step on row 1 (the screened head), for scale,
  (b) the verify-draw pass on row 0 at S in {2, 4, 5, 8} (BS_STEP_VERIFY | BS_STEP_VERIFY_DRAW),
  (v) the greedy verify pass on row 1 at the same S (the argmax tail),
  (w) the same with BS_STEP_LOGITS: the head also writes the fp32 logits of every position.
r(S) = (b) / (a).  The gate is the break-even condition: r(5) < 5 and r(8) < 8 -- otherwise even a free drafter that
is always right loses against plain sampled decoding.  (b) - (v) is what the sampled tail costs the pass over the
argmax tail; it splits into (w) - (v), writing the logits, and (b) - (w), the sampler's seven launches against the
argmax finalize.  (a) - (g) is the decode step's counterpart (where the greedy side also screens the head).
Acceptance is not measured here: synthetic weights say nothing about real text.
"""
import argparse
import os
import statistics
import sys

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

S_LIST = (2, 4, 5, 8)
STATE = dict(top_k=50, top_p=0.9, temperature=1.0, seed=1)


def sample_ab(m, st, ctx, rounds, inner, dev, lines):
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ids = torch.from_numpy(prompt_ids(99, 1, 8, m.vocab).reshape(-1).copy()).to(dev)
    out = [torch.empty(8, dtype=torch.int32, device=dev) for _ in range(2)]
    lg = torch.empty((8, m.vocab), dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    st.set_row_sampler(0, stream=sh, **STATE)

    def timed(fn, n=1):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            for i in range(n):
                fn(i)
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / n  # us per call

    routes = {"a sampled decode S=1": lambda i: st.forward(ids, out[0], 1, 1, slot=0, past_len=ctx + i, stream=sh),
              "g greedy decode S=1": lambda i: st.forward(ids, out[1], 1, 1, slot=1, past_len=ctx + i, stream=sh)}
    for S in S_LIST:
        routes[f"b verify-draw S={S}"] = lambda i, S=S: st.forward(ids, out[0], 1, S, slot=0, past_len=ctx, stream=sh,
                                                                  verify=True, draw=True)
        routes[f"v greedy verify S={S}"] = lambda i, S=S: st.forward(ids, out[1], 1, S, slot=1, past_len=ctx, stream=sh,
                                                                    verify=True)
        routes[f"w greedy verify+logits S={S}"] = lambda i, S=S: st.forward(ids, out[1], 1, S, slot=1, past_len=ctx,
                                                                           stream=sh, verify=True, logits=lg)
    t = {k: [] for k in routes}
    for r in range(rounds + 3):  # three warm-up rounds: captures, code objects
        for k, fn in routes.items():
            us = timed(fn, inner if "decode" in k else 1)
            if r >= 3:
                t[k].append(us)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"# {m.name} bf16, {m.n_layer} layers, vocab {m.vocab}, B = 1, context {ctx}, {rounds} rounds, routes "
                 f"alternating, graph replay; us per call, device events; state {STATE}")
    lines.append(f"{'route':30s} {'median':>9s} {'min':>9s} {'max':>9s}")
    for k, v in t.items():
        lines.append(f"{k:30s} {med[k]:9.1f} {min(v):9.1f} {max(v):9.1f}")
    a, g = med["a sampled decode S=1"], med["g greedy decode S=1"]
    lines.append(f"sampled step over greedy step: a - g = {a - g:.1f} us")
    for S in S_LIST:
        b, v = med[f"b verify-draw S={S}"], med[f"v greedy verify S={S}"]
        w = med[f"w greedy verify+logits S={S}"]
        lines.append(f"r({S}) = b/a = {b / a:.3f}    sampled tail over argmax tail: b - v = {b - v:.1f} us "
                     f"({100 * (b - v) / b:.1f} % of the pass) = logits w - v = {w - v:.1f} + sampler b - w = {b - w:.1f}")
    r5, r8 = med["b verify-draw S=5"] / a, med["b verify-draw S=8"] / a
    lines.append(f"gate r(5) < 5 and r(8) < 8: {'PASS' if r5 < 5 and r8 < 8 else 'FAIL'} (r(5) = {r5:.3f}, r(8) = {r8:.3f})")
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
        sys.exit("spec_sample_bench needs the GPU: nothing is measured without it")
    dev = torch.device("cuda", 0)
    m = config.get(a.model)
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=2, max_ctx=a.ctx + 16,
               max_tokens=a.ctx, seed=a.seed)
    ids = prompt_ids(1234, 1, a.ctx, m.vocab)
    for row in range(2):
        st.forward_host(ids, 1, a.ctx, slot=row, past_len=0)  # the warm caches
    os.makedirs(a.out_dir, exist_ok=True)
    lines = []
    sample_ab(m, st, a.ctx, a.rounds, a.inner, dev, lines)
    with open(os.path.join(a.out_dir, "spec_sample_ab.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
