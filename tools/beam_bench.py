"""beam_bench.py — what beam search costs: the top-k log-prob tail against the greedy and the sampled step, the KV row
pair copy against the same pairs as fork launches, and beam search end to end against plain greedy decoding.

    python tools/beam_bench.py --model bloom-1b1 --ctx 1024 --rounds 24 --out profiles/beam_ab.txt

One process, one full-depth bf16 stage with synthetic weights and 8 KV rows, a warm cache of --ctx positions in every
row (one prefill, forked).  Device events on one stream, the routes alternating inside every round, medians over
the rounds with min and max beside them (the run's own spread).  A condition "a is not slower than b" reads PASS when
a's median is not above b's, SAME when it is but the two min .. max ranges overlap, FAIL otherwise.

Part 1, per W in {2, 4, 8}, graph-replayed S = 1 steps of B = W rows (--inner consecutive steps, per step):
  (a) the top-k step, forward_topk with k = 2W;  (b) the greedy step;  (c) the sampled step (every row holds sampler
  state top_k 50, top_p 0.9: the per-row sampler's tail).  Condition: (a) <= (c).
Part 2, per W and npos in {128, 1024}: one copy_kv of the W - 1 pairs (0 -> 1 .. W - 1) against W - 1 fork_kv(count =
  1) launches of the same pairs, and the bytes moved against bs_hbm_probe's copy rate.  Condition: copy_kv is not
  slower than the forks at any point.  (One pair, and pairs with distinct sources, are the fork launches themselves.)
Part 3: tokens per second per sample of BeamSearcher (W = 4) against plain greedy decoding in the same harness
  (speculative.StageChain: one host round trip a step), and the share of the search spent in its copies (device
  events around them).  Synthetic weights echo the last token: this says nothing about hypothesis quality.
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
from distributed_inference_demo_amd.speculative import StageChain  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, hbm_probe, prompt_ids  # noqa: E402

BEAMS = (2, 4, 8)
ROWS = 8


def verdict(a, b):
    """Is route a not slower than route b?  PASS: a's median is not above b's.  SAME: it is, but the two routes' min ..
    max ranges over the rounds overlap -- no difference beyond the run's own spread.  FAIL otherwise."""
    if statistics.median(a) <= statistics.median(b):
        return "PASS"
    return "SAME (ranges overlap)" if min(a) <= max(b) else "FAIL"


def line(name, v):
    return f"{name:44s} {statistics.median(v):9.1f} {min(v):9.1f} {max(v):9.1f}"


class Timer:
    def __init__(self, dev):
        self.stream = torch.cuda.Stream(dev)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def __call__(self, fn, n=1):
        with torch.cuda.stream(self.stream):
            self.ev[0].record(self.stream)
            for i in range(n):
                fn(i)
            self.ev[1].record(self.stream)
        self.ev[1].synchronize()
        return self.ev[0].elapsed_time(self.ev[1]) * 1e3 / n  # us per call


def tail_ab(m, st, ctx, rounds, inner, dev, lines):
    timed = Timer(dev)
    sh = timed.stream.cuda_stream
    ids = torch.from_numpy(prompt_ids(99, 1, ROWS, m.vocab).reshape(-1).copy()).to(dev)
    out = torch.empty(ROWS, dtype=torch.int32, device=dev)
    top = torch.empty(ROWS, 2 * ROWS, dtype=torch.int32, device=dev)
    lps = torch.empty(ROWS, 2 * ROWS, dtype=torch.float32, device=dev)
    lines.append(f"# {m.name} bf16, {m.n_layer} layers, context {ctx}, {rounds} rounds, routes alternating, {inner} "
                 f"steps a timing; us per step, device events: median min max")
    ok = True
    for W in BEAMS:
        routes = {
            f"a top-k step B={W} k={2 * W} (graph)":
                lambda i, W=W: st.forward_topk(ids, top, lps, W, 1, 2 * W, past_len=ctx + i, stream=sh),
            f"b greedy step B={W} (graph)": lambda i, W=W: st.forward(ids, out, W, 1, past_len=ctx + i, stream=sh),
            f"c sampled step B={W} top_k 50 top_p 0.9 (graph)":
                lambda i, W=W: st.forward(ids, out, W, 1, past_len=ctx + i, stream=sh),
        }
        t = {k: [] for k in routes}
        for r in range(rounds + 3):  # three warm-up rounds: captures, code objects
            for k, fn in routes.items():
                if k.startswith("c"):
                    st.set_row_sampler(0, top_k=50, top_p=0.9, seed=7, count=W, stream=sh)
                us = timed(fn, inner)
                if k.startswith("c"):
                    st.clear_row_sampler(0, count=W, stream=sh)
                if r >= 3:
                    t[k].append(us)
        for k, v in t.items():
            lines.append(line(k, v))
        ta, _, tc = t.values()
        a, b, c = (statistics.median(v) for v in t.values())
        ok = ok and verdict(ta, tc) != "FAIL"
        lines.append(f"W={W}: top-k / greedy = {a / b:.3f}, top-k / sampled = {a / c:.3f}: top-k step not slower than "
                     f"the sampled step: {verdict(ta, tc)}")
    lines.append(f"tail condition at every W: {'PASS' if ok else 'FAIL'}")
    lines.append("")


def copy_ab(m, st, ctx, rounds, inner, dev, lines):
    timed = Timer(dev)
    sh = timed.stream.cuda_stream
    _, copy_gbps = hbm_probe(0, 1 << 30)
    lines.append(f"# {m.name} bf16 KV, {m.n_layer} layers: one copy_kv of W - 1 pairs against W - 1 fork_kv(count = 1) "
                 f"launches; us per reordering, device events: median min max; bs_hbm_probe copy {copy_gbps:.0f} GB/s")
    ok = True
    for W in BEAMS:
        pairs = [(0, j) for j in range(1, W)]
        for npos in (128, min(1024, ctx)):
            routes = {f"copy_kv   W={W} npos={npos}": lambda i: st.copy_kv(pairs, npos, stream=sh),
                      f"forks     W={W} npos={npos}": lambda i: [st.fork_kv(0, j, npos=npos, count=1, stream=sh)
                                                                  for _, j in pairs]}
            t = {k: [] for k in routes}
            for r in range(rounds + 3):
                for k, fn in routes.items():
                    us = timed(fn, inner)
                    if r >= 3:
                        t[k].append(us)
            for k, v in t.items():
                lines.append(line(k, v))
            ta, tb = t.values()
            a, b = (statistics.median(v) for v in t.values())
            moved = 2.0 * (W - 1) * m.n_layer * 2 * m.hidden * npos * 2  # read + written bytes
            ok = ok and verdict(ta, tb) != "FAIL"
            lines.append(f"W={W} npos={npos}: copy_kv / forks = {a / b:.3f}, {moved / a / 1e3:.0f} GB/s "
                         f"({moved / a / 1e3 / copy_gbps:.2f} of the probe's copy rate): "
                         f"{verdict(ta, tb)}")
    lines.append(f"copy condition at every point: {'PASS' if ok else 'FAIL'}")
    lines.append("")


class TimedSearcher(BeamSearcher):
    """BeamSearcher with device events around its copies."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.events = []

    def _copy(self, pairs, npos, fork=False):
        if not pairs:
            return
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(self._stream)
        super()._copy(pairs, npos, fork=fork)
        ev[1].record(self._stream)
        self.events.append(ev)

    def copy_seconds(self):
        torch.cuda.synchronize()
        s = sum(a.elapsed_time(b) for a, b in self.events) * 1e-3
        self.events = []
        return s


def end_to_end(m, st, prompt_len, new, reps, lines):
    prompt = prompt_ids(1234, 1, prompt_len, m.vocab).reshape(-1).tolist()
    chain = StageChain([st])
    W = 4
    bs = TimedSearcher([st], W)

    def greedy():
        t0 = time.perf_counter()
        tok = chain.prefill(prompt, 0)
        for i in range(new - 1):
            tok = chain.step(tok, prompt_len + i)
        return new / (time.perf_counter() - t0), 0.0, 0

    def beam():
        n0 = bs.kv_copies
        t0 = time.perf_counter()
        seqs, _, _ = bs.generate(prompt, new)
        dt = time.perf_counter() - t0
        return len(seqs[0]) / dt, bs.copy_seconds() / dt, bs.kv_copies - n0

    res = {"plain greedy decode": [], f"beam search W={W}": []}
    share, copies = [], 0
    for r in range(reps + 1):  # one warm-up repetition
        for name, fn in (("plain greedy decode", greedy), (f"beam search W={W}", beam)):
            tps, sh, n = fn()
            if r:
                res[name].append(tps)
                if n:
                    share.append(sh)
                    copies = n
    lines.append(f"# {m.name} bf16, prompt {prompt_len}, {new} new tokens (prefill included), {reps} repetitions "
                 f"alternating; tokens/s per sample, host clock around synchronous steps: median min max")
    for name, v in res.items():
        lines.append(line(name, v))
    g, b = (statistics.median(v) for v in res.values())
    lines.append(f"beam / greedy = {b / g:.3f}; copies: {copies} row pairs a search, "
                 f"{100 * statistics.median(share) if share else 0.0:.2f} % of the search's time (device events)")
    lines.append("synthetic weights echo the last token: nothing here speaks about hypothesis quality")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="bloom-1b1")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="profiles/beam_ab.txt")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("beam_bench needs the GPU: nothing is measured without it")
    dev = torch.device("cuda", 0)
    m = config.get(a.model)
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=ROWS,
               max_ctx=a.ctx + a.new + 16, max_tokens=a.ctx, seed=a.seed)
    st.forward_host(prompt_ids(1234, 1, a.ctx, m.vocab), 1, a.ctx, past_len=0)  # the warm cache, in every row
    st.fork_kv(0, 1, count=ROWS - 1)
    torch.cuda.synchronize()  # the fork ran on the stage's own stream
    lines = []
    tail_ab(m, st, a.ctx, a.rounds, a.inner, dev, lines)
    copy_ab(m, st, a.ctx, a.rounds, a.inner, dev, lines)
    end_to_end(m, st, a.ctx, a.new, a.reps, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
