"""Speculative decoding for one sample on one GPU: a drafter proposes up to k tokens, one BS_STEP_VERIFY pass of the
target model over [last token, draft_1 .. draft_k] returns the greedy token of every position, and the longest
agreeing prefix of the draft plus one more token is emitted -- more than one token per pass over the weights, and
exactly the tokens plain greedy decoding produces.

    accept(draft, top)            the acceptance rule, a pure function
    NgramDrafter(k, n_max)        prompt lookup: the continuation of the most recent earlier occurrence of the
                                  history's longest repeated suffix
    StageDrafter(stages, k)       k greedy S = 1 steps of a draft model (a smaller checkpoint, or the int8 / MXFP4
                                  variant of the target) with its own KV row
    SpeculativeDecoder(stages, drafter, k).generate(prompt, max_new)

Sampled speculative decoding (sampler = {"top_k", "top_p", "temperature", "seed"} on the decoder, and on a
StageDrafter): the target's KV row holds that per-row sampler state, plain steps sample, and a verify pass runs with
BS_STEP_VERIFY_DRAW: it returns the row's own DRAW at every position.  A draw depends on (seed, position, logits)
only, so the agreeing prefix of the draft plus one more token is exactly what plain sampled decoding emits --
token-matching verification, no rejection-sampling arithmetic, the output distribution is plain sampling's.  A draft
model that holds the same state draws with the target's u at every position, so its proposal agrees wherever the two
models' CDF intervals of the token overlap at u.

A drafter is any object with `propose(history, k) -> list of at most k token ids` (history: the prompt and every
token emitted so far); an empty proposal makes the decoder take a plain S = 1 step.

Scope: an in-process chain of stages on one GPU, one sample in KV row 0.  Multi-rank pipelines are out of scope:
how many tokens a pass accepts depends on the data, while serve's schedule is derived on every rank from the prompt
lengths alone (serve.admission_schedule), so the ranks could not agree on the rows' positions without a new
exchange per pass; the RCCL pipeline with more than one rank has not run on hardware in this project either.
"""
import numpy as np


def accept(draft, top):
    """The acceptance rule for a row fed [last, d_1 .. d_k] whose verify pass returned top[0 .. k] (top[j] = the
    greedy token after the j-th fed token): n = the number of leading j with d_(j+1) == top[j].  The row emits
    top[0 .. n], n + 1 tokens (the accepted drafts and the target's own next token), and its position becomes
    past + n + 1.  Returns (n, emitted)."""
    draft, top = [int(t) for t in draft], [int(t) for t in top]
    if len(top) != len(draft) + 1:
        raise ValueError(f"{len(top)} verified positions for {len(draft)} drafted tokens")
    n = 0
    while n < len(draft) and draft[n] == top[n]:
        n += 1
    return n, top[:n + 1]


class NgramDrafter:
    """Prompt lookup: the longest suffix of the history, of length n_max down to 1, that occurred earlier; of its
    occurrences the most recent; the proposal is the up to k tokens that followed it.  Nothing found: no proposal."""

    def __init__(self, k, n_max=3):
        if k < 1 or n_max < 1:
            raise ValueError("k and n_max must be >= 1")
        self.k, self.n_max = k, n_max

    def propose(self, history, k=None):
        k = self.k if k is None else min(k, self.k)
        h = list(history)
        if k < 1:
            return []
        for n in range(min(self.n_max, len(h) - 1), 0, -1):
            suffix = h[-n:]
            for i in range(len(h) - n - 1, -1, -1):  # the most recent earlier occurrence first
                if h[i:i + n] == suffix:
                    return h[i + n:i + n + k]
        return []


class StageChain:
    """An in-process chain of stages (first .. last) on one GPU driving KV row 0: a prefill of any length, the plain
    S = 1 step and the BS_STEP_VERIFY pass.  Positions are passed per call, so rolling back is the caller passing a
    smaller `past`.  Device buffers on one stream of its own (decode steps and verify passes replay captured graphs:
    the buffers of a shape are kept); host_io=True runs the stages' forward_host instead (numpy in and out, for
    stage objects without device pointers)."""

    def __init__(self, stages, host_io=False):
        self.stages = list(stages)
        if not self.stages or not self.stages[0].is_first or not self.stages[-1].is_last:
            raise ValueError("a chain runs from a first stage to a last stage")
        self.host_io = host_io
        self.max_ctx = min(st.max_ctx for st in self.stages)
        self._buf = {}
        self._stream = None

    def _buffers(self, seq):
        import torch
        if self._stream is None:
            self._dev = torch.device("cuda", self.stages[0].desc.device)
            self._stream = torch.cuda.Stream(self._dev)
        b = self._buf.get(seq)
        if b is None:
            ids = torch.empty(seq, dtype=torch.int32, device=self._dev)
            hid = [torch.empty(seq, st.hidden, dtype=torch.float32, device=self._dev) for st in self.stages[:-1]]
            out = torch.empty(seq, dtype=torch.int32, device=self._dev)
            b = self._buf[seq] = (ids, hid, out)
        return b

    def set_sampler(self, sampler):
        """Row 0's sampler state on the last stage ({"top_k", "top_p", "temperature", "seed"}; missing keys take
        set_row_sampler's defaults), or back to greedy with None.  Ordered on the chain's stream."""
        last = self.stages[-1]
        stream = None
        if not self.host_io:
            self._buffers(1)
            stream = self._stream.cuda_stream
        if sampler is None:
            last.clear_row_sampler(0, stream=stream)
        else:
            last.set_row_sampler(0, stream=stream, **sampler)

    def _run(self, ids, past, verify, draw=False):
        seq = len(ids)
        kw = {"draw": True} if draw else {}  # stage objects without the flag are never handed it
        for st in self.stages:
            st.past[0] = past  # the rows' host mirrors follow the caller's position (Stage.rollback)
        if self.host_io:
            x = np.asarray(ids, np.int32).reshape(1, seq)
            for st in self.stages:
                x = st.forward_host(x, 1, seq, slot=0, past_len=past, verify=verify, **kw)
            return [int(t) for t in np.asarray(x).reshape(-1)]
        import torch
        dids, hid, out = self._buffers(seq)
        with torch.cuda.stream(self._stream):
            dids.copy_(torch.tensor(ids, dtype=torch.int32))
            x = dids
            for i, st in enumerate(self.stages):
                y = out if i == len(self.stages) - 1 else hid[i]
                st.forward(x, y, 1, seq, slot=0, past_len=past, stream=self._stream.cuda_stream, verify=verify, **kw)
                x = y
            n = seq if verify else 1
            res = out[:n].cpu()  # a synchronous copy on the chain's stream
        return [int(t) for t in res.tolist()]

    def prefill(self, ids, past=0):
        """Feed len(ids) tokens at position `past` through the unflagged path; the greedy token after the last."""
        return self._run(list(ids), past, False)[0]

    def step(self, tok, past):
        return self._run([tok], past, False)[0]

    def verify(self, ids, past, draw=False):
        """Feed 2..8 tokens at position `past`; the greedy token after each of them, or with draw=True
        (BS_STEP_VERIFY_DRAW) the row sampler's draw after each of them."""
        return self._run(list(ids), past, True, draw)


class StageDrafter:
    """k greedy S = 1 steps of a draft model: an in-process chain of stages with the target's vocabulary.  The draft
    keeps its own KV row: before drafting it rolls the row back to the prefix it shares with the history (the
    accepted length) and catches up on the tokens it has not seen (one S = 1 step, or one short prefill pass).
    sampler: the draft row holds this sampler state (the target's: same seed), so every draft is drawn with the
    target's u at its position; None: greedy drafts."""

    def __init__(self, stages, k, host_io=False, sampler=None):
        if k < 1:
            raise ValueError("k must be >= 1")
        self.chain = stages if isinstance(stages, StageChain) else StageChain(stages, host_io=host_io)
        self.k = k
        if sampler is not None:
            self.chain.set_sampler(dict(sampler))
        self.fed = []  # the tokens whose K / V the draft's row holds

    def propose(self, history, k=None):
        k = self.k if k is None else min(k, self.k)
        h = [int(t) for t in history]
        k = min(k, self.chain.max_ctx - len(h))  # the draft's row holds the history and k - 1 drafts
        if k < 1 or not h:
            return []
        c = 0
        lim = min(len(self.fed), len(h) - 1)  # the last token is always fed: its output is the first draft
        while c < lim and self.fed[c] == h[c]:
            c += 1
        new = h[c:]
        tok = self.chain.step(new[0], c) if len(new) == 1 else self.chain.prefill(new, c)
        self.fed = h[:]
        draft = [tok]
        while len(draft) < k:
            tok = self.chain.step(draft[-1], len(self.fed))
            self.fed.append(draft[-1])
            draft.append(tok)
        return draft


class SpeculativeDecoder:
    """Greedy generation of one sample (KV row 0) over an in-process chain of stages on one GPU, k drafted tokens a
    pass.  The prompt is prefilled through the unflagged path; each round the drafter proposes d <= k tokens and one
    BS_STEP_VERIFY pass of d + 1 positions emits accept()'s tokens; without a proposal the round is a plain S = 1
    step.  The tokens equal plain greedy decoding's whenever the target's top-2 logit margins exceed what the
    batched and the single-row kernels may differ by (different summation orders).
    sampler ({"top_k", "top_p", "temperature", "seed"}): sampled generation.  generate() sets row 0's sampler state
    before the prefill (the first token is sampled), plain steps sample and verify passes return draws
    (draw=True); accept() is unchanged.  The tokens equal plain sampled decoding's with that state wherever u lies
    further inside the drawn token's CDF interval than the kernels' logit differences move its ends."""

    def __init__(self, stages, drafter, k, host_io=False, sampler=None):
        if not 1 <= k <= 7:
            raise ValueError("k must be in [1, 7] (a verify pass holds at most 8 positions)")
        self.chain = stages if isinstance(stages, StageChain) else StageChain(stages, host_io=host_io)
        self.drafter, self.k = drafter, k
        self.sampler = None if sampler is None else dict(sampler)

    def generate(self, prompt, max_new):
        """Returns (tokens [max_new], {"passes": verify passes, "drafted": tokens proposed in them, "accepted":
        drafted tokens that were emitted, "plain_steps": S = 1 rounds})."""
        prompt = [int(t) for t in prompt]
        if not prompt or max_new < 1:
            raise ValueError("generate needs a prompt and max_new >= 1")
        if len(prompt) + max_new > self.chain.max_ctx:
            raise ValueError(f"prompt ({len(prompt)}) + max_new ({max_new}) exceed max_ctx ({self.chain.max_ctx})")
        stats = {"passes": 0, "drafted": 0, "accepted": 0, "plain_steps": 0}
        if self.sampler is not None:
            self.chain.set_sampler(self.sampler)
        hist = prompt + [self.chain.prefill(prompt, 0)]
        pos = len(prompt)  # positions the target's row holds; hist[pos:] is not cached yet (always one token)
        while len(hist) - len(prompt) < max_new:
            left = max_new - (len(hist) - len(prompt))
            # a pass of d drafts emits up to d + 1 tokens and appends d + 1 positions
            room = min(self.k, left - 1, self.chain.max_ctx - pos - 1)
            draft = [int(t) for t in self.drafter.propose(hist, room)][:room] if room >= 1 else []
            if not draft:
                emitted = [self.chain.step(hist[-1], pos)]
                stats["plain_steps"] += 1
            else:
                top = (self.chain.verify([hist[-1]] + draft, pos, draw=True) if self.sampler is not None
                       else self.chain.verify([hist[-1]] + draft, pos))
                n, emitted = accept(draft, top)
                stats["passes"] += 1
                stats["drafted"] += len(draft)
                stats["accepted"] += n
            pos += len(emitted)  # rollback: the rejected drafts' positions are simply not counted
            hist += emitted
        for st in self.chain.stages:
            st.past[0] = pos
        return hist[len(prompt):], stats
