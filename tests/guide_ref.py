"""TEST INFRASTRUCTURE: the guided-decoding rule (include/bloomstage.h "Guided decoding") in
numpy fp32.  Given the logits and the state the result is defined bit for bit, so device results are compared with
`logit_proc_ref.bits_equal`, never with a tolerance.  A guide is anything with the six CSR tables as attributes
(distributed_inference_demo_amd.guide.Guide); this file reads the tables itself and shares no code with it."""
import numpy as np

import logit_proc_ref as lref

BAN = lref.BAN


def step(guide, q, t):
    """The state after token t in state q, or -1 where t is not allowed."""
    lo, hi = int(guide.row_ptr[q]), int(guide.row_ptr[q + 1])
    e = np.flatnonzero(np.asarray(guide.edge_token[lo:hi]) == int(t))  # a linear scan: no search to get wrong
    return int(guide.edge_next[lo + int(e[0])]) if e.size else int(guide.default_next[q])


def allowed_mask(guide, q, V):
    lo, hi = int(guide.row_ptr[q]), int(guide.row_ptr[q + 1])
    tok, nxt = np.asarray(guide.edge_token[lo:hi]), np.asarray(guide.edge_next[lo:hi])
    mask = np.full(V, int(guide.default_next[q]) >= 0)
    mask[tok] = nxt >= 0
    return mask


def apply(logits, guide, q):
    """Masked copy of fp32 logits [V] for a row in state q: -FLT_MAX where the token is not allowed, the input's bits
    elsewhere."""
    l = np.array(logits, dtype=np.float32).reshape(-1).copy()
    l[~allowed_mask(guide, q, l.size)] = BAN
    return l


def advance(guide, q, t):
    """(state, rejected) after the pick t: a token that is not allowed leaves the state."""
    n = step(guide, q, t)
    return (n, 0) if n >= 0 else (q, 1)


def walk(guide, q, tokens, V):
    """(state, n_steps, n_rejected) after `tokens`; an id outside [0, V) is rejected."""
    rej = 0
    for t in tokens:
        r = 1
        if 0 <= int(t) < V:
            q, r = advance(guide, q, int(t))
        rej += r
    return q, len(tokens), rej


def generate(logits_fn, prompt, guide, steps, proc=None, pick=None, state=None):
    """A per-sample loop: logits_fn(tokens) -> raw fp32 logits [V] of the next position.  proc: logit_proc_ref
    parameters applied first (the history is prompt + generated), then the guide, then the pick (default: the first
    index of the largest logit).  The guide sees generated tokens only.  Returns (ids, masked logits, final state,
    n_rejected)."""
    T = [int(t) for t in prompt]
    q = guide.start if state is None else state
    out, scores, rej = [], [], 0
    for g in range(steps):
        l = logits_fn(T)
        if proc is not None:
            l = lref.apply(l, T, proc, n_generated=g)
        l = apply(l, guide, q)
        tok = lref.first_argmax(l) if pick is None else int(pick(l, len(T)))
        q, r = advance(guide, q, tok)
        rej += r
        scores.append(l)
        out.append(tok)
        T.append(tok)
    return out, scores, q, rej
