"""Beam search for one sample on one GPU: W hypotheses in KV rows [0, W), one top-k log-prob pass a step
(bs_forward_topk, k = 2W), selection on the host, and one bs_copy_kv call per stage that hands the rows of dead
hypotheses to the further children of living ones.

    assign_slots(parents)         which KV row every selected child takes, and the rows to copy; a pure function
    BeamSearcher(stages, num_beams, length_penalty, eos, num_return).generate(prompt, max_new)

The selection rule restates transformers' generate(num_beams=W, do_sample=False, early_stopping=False,
length_penalty=..., num_return_sequences=...) (generation/utils.py _beam_search):
  candidates  every step, each running hypothesis w (score s_w, the sum of its tokens' log-probs) offers (w, token v)
              at s_w + log p_w(v); the 2W best of all W * V are kept, ranked by score, then by the lower flat index
              w * V + v (w = the hypothesis' rank).  The 2W best lie inside the hypotheses' own 2W best tokens, which
              is what the device returns, so W <= 8 (k <= 16).
  stopped     a candidate whose token is `eos`, and every candidate of the step that reaches prompt + max_new tokens.
  running     the W best candidates that did not stop, in rank order, go on.
  finished    a stopped candidate among the W best of the 2W is a finished hypothesis with score
              s / n ** length_penalty, n = its generated tokens (eos included); the W best finished ones are kept, an
              earlier one ahead of a later one of equal score.
  the end     max_new tokens, or when W hypotheses are finished and the best running score divided by
              n ** length_penalty (n = tokens generated so far) no longer exceeds the worst finished score.
Scores are summed in float64 from the device's fp32 log-probs (transformers sums in fp32).  W = 1 without eos is
greedy decoding.

Scope: an in-process chain of stages on one GPU, like speculative.StageChain (device buffers on a stream of its own,
one host round trip a step); host_io=True runs the stages' numpy entry points instead.
"""
import numpy as np

NEG = -1.0e9  # transformers' "minus infinity" of beam scores


def assign_slots(parents):
    """parents[i]: the KV row (slot) of the parent of the i-th selected child, in rank order; W = len(parents) rows
    [0, W) exist.  Returns (slots, copies): slots[i] = the row child i takes, copies = [(src, dst)] to run before the
    next step.  The best-ranked child of every living parent keeps the parent's row (no copy); every further child
    takes the lowest row that has no child, with one copy parent -> that row.  So there are exactly as many copies as
    rows without a child, every destination is such a row and every source a row with one: no destination is a
    source or appears twice (bs_copy_kv's condition), and no spare rows are needed."""
    parents = [int(p) for p in parents]
    W = len(parents)
    if any(not 0 <= p < W for p in parents):
        raise ValueError(f"parent rows must lie in [0, {W})")
    living = set(parents)
    free = [r for r in range(W) if r not in living]
    slots, copies, kept = [], [], set()
    for p in parents:
        if p not in kept:
            kept.add(p)
            slots.append(p)
        else:
            d = free.pop(0)
            slots.append(d)
            copies.append((p, d))
    return slots, copies


class _Hyp:
    __slots__ = ("tokens", "score", "logprobs", "slot")

    def __init__(self, tokens, score, logprobs, slot):
        self.tokens, self.score, self.logprobs, self.slot = tokens, score, logprobs, slot


class BeamSearcher:
    """Beam search of one sample over an in-process chain of stages (first .. last) on one GPU, hypotheses in KV rows
    [0, num_beams).  generate() prefills the prompt in row 0 with a top-k pass (k = 2W), forks row 0 to rows 1..W-1
    (bs_fork_kv), and then runs per step: plain forwards on the stages before the last, forward_topk(B = W, S = 1,
    k = 2W) on the last, the selection on the host, and copy_kv of assign_slots' pairs on every stage.
    kv_copies counts the pairs copied (the first fork included) over the searcher's life."""

    def __init__(self, stages, num_beams, length_penalty=1.0, eos=None, num_return=1, host_io=False):
        self.stages = list(stages)
        if not self.stages or not self.stages[0].is_first or not self.stages[-1].is_last:
            raise ValueError("a chain runs from a first stage to a last stage")
        if not 1 <= num_beams <= 8:
            raise ValueError("num_beams must be in [1, 8] (a top-k pass returns at most 16 = 2 * 8 candidates)")
        if not 1 <= num_return <= num_beams:
            raise ValueError("num_return must be in [1, num_beams]")
        if min(st.max_batch for st in self.stages) < num_beams:
            raise ValueError(f"every stage needs max_batch >= num_beams ({num_beams})")
        self.W, self.lp, self.num_return, self.host_io = num_beams, float(length_penalty), num_return, host_io
        self.eos = None if eos is None or eos < 0 else int(eos)
        self.max_ctx = min(st.max_ctx for st in self.stages)
        self.vocab = self.stages[-1].vocab
        self.kv_copies = 0
        self._buf = {}
        self._stream = None

    # ---- one pass through the chain: rows [0, batch), seq tokens each at position `past`; (ids, logprobs) [batch][k]
    def _buffers(self, batch, seq):
        import torch
        if self._stream is None:
            self._dev = torch.device("cuda", self.stages[0].desc.device)
            self._stream = torch.cuda.Stream(self._dev)
        b = self._buf.get((batch, seq))
        if b is None:
            k = 2 * self.W
            ids = torch.empty(batch, seq, dtype=torch.int32, device=self._dev)
            hid = [torch.empty(batch, seq, st.hidden, dtype=torch.float32, device=self._dev) for st in self.stages[:-1]]
            top = torch.empty(batch, k, dtype=torch.int32, device=self._dev)
            lps = torch.empty(batch, k, dtype=torch.float32, device=self._dev)
            b = self._buf[(batch, seq)] = (ids, hid, top, lps)
        return b

    def _run(self, tokens, batch, seq, past):
        k = 2 * self.W
        x = np.asarray(tokens, np.int32).reshape(batch, seq)
        if self.host_io:
            for st in self.stages[:-1]:
                x = st.forward_host(x, batch, seq, slot=0, past_len=past)
            ids, lps, _ = self.stages[-1].forward_topk_host(x, batch, seq, k, slot=0, past_len=past)
            return np.asarray(ids), np.asarray(lps)
        import torch
        dids, hid, top, lps = self._buffers(batch, seq)
        with torch.cuda.stream(self._stream):
            dids.copy_(torch.from_numpy(x))
            cur = dids
            for i, st in enumerate(self.stages[:-1]):
                st.forward(cur, hid[i], batch, seq, slot=0, past_len=past, stream=self._stream.cuda_stream)
                cur = hid[i]
            self.stages[-1].forward_topk(cur, top, lps, batch, seq, k, slot=0, past_len=past,
                                         stream=self._stream.cuda_stream)
            ids_h, lps_h = top.cpu(), lps.cpu()  # synchronous copies on the searcher's stream
        return ids_h.numpy(), lps_h.numpy()

    def _copy(self, pairs, npos, fork=False):
        if not pairs:
            return
        stream = None if self.host_io else self._stream.cuda_stream
        for st in self.stages:
            if fork:  # the first step: row 0 to rows 1 .. W - 1
                st.fork_kv(0, 1, npos=npos, count=len(pairs), stream=stream)
            else:
                st.copy_kv(pairs, npos, stream=stream)
        self.kv_copies += len(pairs)

    def generate(self, prompt, max_new):
        """Returns (sequences, scores, token_logprobs): the num_return best finished hypotheses, best first -- each
        one's generated tokens (an eos included), its score (sum of log-probs / length ** length_penalty) and the
        device's fp32 log-prob of every token."""
        prompt = [int(t) for t in prompt]
        if not prompt or max_new < 1:
            raise ValueError("generate needs a prompt and max_new >= 1")
        if len(prompt) + max_new > self.max_ctx:
            raise ValueError(f"prompt ({len(prompt)}) + max_new ({max_new}) exceed max_ctx ({self.max_ctx})")
        W, V, P = self.W, self.vocab, len(prompt)
        running = [_Hyp([], 0.0, [], 0)]  # in rank order
        finished = []                     # (score, tokens, logprobs), best first, at most W
        ids, lps = self._run(prompt, 1, P, 0)
        for n in range(1, max_new + 1):  # n: tokens every candidate of this step holds
            # the 2W best candidates: by score, then by the lower flat index (rank of the parent, then token id)
            cands = []
            for w, hyp in enumerate(running):
                for j in range(2 * W):
                    tok = int(ids[hyp.slot][j])
                    cands.append((-(hyp.score + float(lps[hyp.slot][j])), w * V + tok, w, tok, float(lps[hyp.slot][j])))
            cands.sort(key=lambda c: (c[0], c[1]))
            cands = cands[:2 * W]
            last = n == max_new
            nxt = []
            for rank, (neg, _, w, tok, lp) in enumerate(cands):
                stopped = last or tok == self.eos
                if stopped and rank < W:
                    hyp = running[w]
                    fin = (-neg / (n ** self.lp), hyp.tokens + [tok], hyp.logprobs + [lp])
                    at = len(finished)  # behind every kept hypothesis of an equal or better score
                    while at > 0 and finished[at - 1][0] < fin[0]:
                        at -= 1
                    finished.insert(at, fin)
                    del finished[W:]
                elif not stopped and len(nxt) < W:
                    nxt.append((w, tok, lp, -neg))
            if last:
                break
            # the end: W finished hypotheses none of which the best running one can still beat
            best_running = nxt[0][3] if nxt else NEG
            if len(finished) == W and not best_running / (n ** self.lp) > finished[-1][0]:
                break
            slots, copies = assign_slots([running[w].slot for w, _, _, _ in nxt])
            running = [_Hyp(running[w].tokens + [tok], score, running[w].logprobs + [lp], slots[i])
                       for i, (w, tok, lp, score) in enumerate(nxt)]
            self._copy(copies, P + n - 1, fork=(n == 1))
            feed = [0] * W
            for hyp in running:
                feed[hyp.slot] = hyp.tokens[-1]
            ids, lps = self._run(feed, W, 1, P + n - 1)
        out = finished[:self.num_return]
        return [f[1] for f in out], [f[0] for f in out], [f[2] for f in out]
