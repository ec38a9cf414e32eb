"""A/B of the admission prefill of n samples on one full-depth bf16 stage:

  (a) n per-row bs_forward prefill passes, one sample each (serve's route without --ragged-admission);
  (b) one bs_forward_ragged pass of the n rows (--ragged-admission).

One process, device events on one stream, the two routes alternating inside every round, a buffer larger than the
last-level cache overwritten ahead of every timing (weights not left hot), medians and min..max over the rounds.
Then the attention launches alone (bs_profile_enable class 3: events around every attention launch, the host
enqueued ahead behind a stream delay): one bs_forward of n equal-length rows (attn_prefill_tr_launch) against the
ragged pass of the same rows (attn_ragged_kernel, which also writes the cache).

    python tools/ragged_prefill_bench.py --models bloom-1b1,bloom-7b1 --rounds 11 --out profiles/ragged_prefill_ab.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_inference_demo_amd import config  # noqa: E402
from distributed_inference_demo_amd.stage import Stage, prompt_ids  # noqa: E402

DEV = torch.device("cuda", 0)


def mixed(n):
    """n lengths spread over 16 .. 128."""
    return [16 + (112 * i) // max(n - 1, 1) for i in range(n)]


def fmt(xs):
    return f"{statistics.median(xs) * 1e3:9.1f} us  [{min(xs) * 1e3:8.1f} .. {max(xs) * 1e3:8.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="bloom-1b1,bloom-7b1")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default="profiles/ragged_prefill_ab.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# ragged prefill A/B on {torch.cuda.get_device_name(0)}; {a.rounds} rounds, routes alternating, device events,")
    say("# a 1 GiB buffer overwritten ahead of every timing; median [min .. max]")
    flush = torch.empty(1 << 28, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream(DEV)
    sh = stream.cuda_stream
    cases = [(f"{n} x 64", [64] * n) for n in (4, 8, 32)] + [(f"{n} mixed 16..128", mixed(n)) for n in (8, 32)]
    for name in a.models.split(","):
        m = config.get(name)
        st = Stage(m.hidden, m.n_head, m.n_layer, m.vocab, 0, m.n_layer, dtype="bf16", max_batch=32, max_ctx=160,
                   max_tokens=32 * 128, seed=1)
        ids = torch.from_numpy(prompt_ids(7, 1, 32 * 128, m.vocab).reshape(-1).copy()).to(DEV)
        out = torch.empty(32, dtype=torch.int32, device=DEV)
        say(f"\n## {name}: {m.n_layer} layers, hidden {m.hidden}, {m.n_head} heads, bf16")

        def per_row(lens):
            at = 0
            for r, n in enumerate(lens):
                st.forward(ids[at:at + n], out[r:r + 1], 1, n, slot=r, past_len=0, stream=sh)
                at += n

        def ragged(lens):
            st.forward_ragged(ids, out, list(range(len(lens))), lens, [0] * len(lens), stream=sh)

        def timed(fn, lens):
            with torch.cuda.stream(stream):
                flush.fill_(1.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(lens)
                e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1)

        say("# whole admission wave: (a) n per-row passes, (b) one ragged pass")
        for label, lens in cases:
            for fn in (per_row, ragged):  # warm every shape
                timed(fn, lens)
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(timed(per_row, lens))
                tb.append(timed(ragged, lens))
            verdict = "ranges do not overlap" if max(tb) < min(ta) or max(ta) < min(tb) else "ranges overlap"
            say(f"{label:>18}  T={sum(lens):5d}  (a) {fmt(ta)}   (b) {fmt(tb)}   a/b {statistics.median(ta) / statistics.median(tb):5.2f}  {verdict}")

        say("# attention launch alone, per layer: one bs_forward of n equal rows (attn_prefill_tr_launch) vs the ragged pass")
        st.profile_enable(3)

        def attn_us(fn):
            Stage.stream_delay(sh, 20000)
            fn()
            ms, launches, _ = st.profile_read()
            st.profile_enable(3)  # restart the accumulation
            return ms / launches

        for n in (4, 8, 32):
            lens = [64] * n
            plain = lambda: st.forward(ids[:64 * n], out[:n], n, 64, slot=0, past_len=0, stream=sh)  # noqa: E731
            rag = lambda: ragged(lens)  # noqa: E731
            attn_us(plain), attn_us(rag)
            pa, pb = [], []
            for _ in range(a.rounds):
                pa.append(attn_us(plain))
                pb.append(attn_us(rag))
            say(f"{n:3d} x 64  prefill_tr {fmt(pa)}   ragged {fmt(pb)}")
        st.profile_enable(0)
        st.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
