"""kv_fork_bench.py — what a KV row fork (bs_fork_kv) costs against the prefix prefill it replaces.

    python tools/kv_fork_bench.py --rounds 20 --out profiles/kv_fork_ab.txt
    python tools/kv_fork_bench.py --e2e --out profiles/kv_fork_e2e.txt

One process.  Per shape (bloom-1b1 and bloom-7b1 at full depth with a bf16 cache, bloom-7b1 also with the int8
cache) one whole-model bf16 stage, and for P in {128, 1024} and count in {1, 7}, alternating inside every round, device
events on one stream, medians over the rounds:
  (a) fork     fork_kv of positions [0, P) of row 0 to rows [1, 1 + count)
  (b) prefill  the B = 1 prefill pass of P tokens into row 0 that a fork replaces
and once per process (c) the bs_hbm_probe copy rate.  The table prints (a) and (b) in microseconds and the fork's
(read + written bytes) / (a) as a fraction of (c); the gate is (a) < (b) at every point.

--e2e: serve on bloom-7b1, 16 samples, 8 in flight, 32 tokens each, prompts of 1024 shared + 64 own tokens, three
alternating repetitions of --shared-prefix 1024 with the fork, the same without it (--prefix-fork 0), and
--shared-prefix 0; tokens/s of each run.
"""
import argparse
import os
import statistics
import sys

import torch  # before the library (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, hbm_probe, prompt_ids  # noqa: E402

SHAPES = (("bloom-1b1", False), ("bloom-7b1", False), ("bloom-7b1", True))
PREFIXES = (128, 1024)
COUNTS = (1, 7)


def bench_shape(name, kv_int8, rounds, dev, copy_gbps, lines):
    m = config.get(name)
    st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=1 + max(COUNTS),
               max_ctx=max(PREFIXES) + 8, max_tokens=max(PREFIXES), seed=1, kv_int8=kv_int8)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tok = torch.empty(1, dtype=torch.int32, device=dev)

    def timed(fn):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3  # us

    hd = m.hidden // m.n_head
    pos_bytes = m.n_layer * 2 * m.n_head * (hd + 4 if kv_int8 else 2 * hd)  # one position of one row, every layer
    ok = True
    for P in PREFIXES:
        ids = torch.from_numpy(prompt_ids(3, 1, P, m.vocab).copy()).to(dev)
        for count in COUNTS:
            ta, tb = [], []
            for r in range(rounds + 3):  # warm-up rounds: code objects, workspace
                b = timed(lambda: st.forward(ids, tok, 1, P, slot=0, past_len=0, stream=sh))
                a = timed(lambda: st.fork_kv(0, 1, npos=P, count=count, stream=sh))
                if r >= 3:
                    ta.append(a)
                    tb.append(b)
            a, b = statistics.median(ta), statistics.median(tb)
            moved = (1 + count) * P * pos_bytes
            rate = moved / (a * 1e-6) / 1e9
            ok = ok and a < b
            lines.append(f"{name:10s} kv {'int8' if kv_int8 else 'bf16'}  P {P:5d} count {count}:  fork {a:9.1f} us "
                         f"(min {min(ta):9.1f}, max {max(ta):9.1f})  prefill {b:10.1f} us (min {min(tb):10.1f})  "
                         f"{moved / 1e6:8.1f} MB moved, {rate:7.1f} GB/s = {rate / copy_gbps:5.2f} x probe copy  "
                         f"{'fork < prefill' if a < b else 'GATE FAILS: fork >= prefill'}")
            print(lines[-1], flush=True)
    st.close()
    return ok


def e2e(dev, lines, reps=3):
    from distributed_inference_demo_amd.serve import RunConfig, run_rank, synthetic_prompts
    base = dict(model="bloom-7b1", num_sample=16, core_pool_size=8, max_length=32, prompt_len=1024 + 64)
    prompts = synthetic_prompts(RunConfig(shared_prefix=1024, **base), config.get("bloom-7b1").vocab)
    settings = (("shared-prefix 1024, fork", dict(shared_prefix=1024)),
                ("shared-prefix 1024, no fork", dict(shared_prefix=1024, prefix_fork=False)),
                ("shared-prefix 0", dict()))
    tps = {k: [] for k, _ in settings}
    samples = {}
    for rep in range(reps):
        for k, kw in settings:
            res = run_rank(RunConfig(**base, **kw), 0, 1, dev, prompts=prompts)
            tps[k].append(res["tokens_per_s"])
            samples[k] = res["samples"]
            print(f"rep {rep} {k}: {res['tokens_per_s']:.1f} tokens/s, {res['seconds']:.3f} s", flush=True)
    for k, v in tps.items():
        lines.append(f"serve bloom-7b1, 16 samples x 32 tokens, 8 in flight, prompts 1024 shared + 64 own -- {k:28s}: "
                     f"median {statistics.median(v):8.1f} tokens/s (min {min(v):8.1f}, max {max(v):8.1f}, {reps} runs)")
    same = samples[settings[0][0]] == samples[settings[1][0]]
    lines.append(f"fork and no-fork runs return {'the same' if same else 'DIFFERENT'} tokens")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    ok = True
    if args.e2e:
        e2e(dev, lines)
    else:
        _, copy = hbm_probe(0, 1 << 30)
        lines.append(f"kv_fork_bench: medians of {args.rounds} rounds, device events; bs_hbm_probe copy rate "
                     f"{copy:.1f} GB/s (read + written bytes, 1 GiB)")
        for name, kv8 in SHAPES:
            ok = bench_shape(name, kv8, args.rounds, dev, copy, lines) and ok
        lines.append("gate (a) < (b): " + ("holds at every point" if ok else "FAILS at the points marked"))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
