"""TEST INFRASTRUCTURE: the per-row logit processor rule (include/bloomstage.h "Per-row logit processors", DESIGN.md
section 5j) in numpy fp32.  Given the logits, the token history and the parameters the result is defined bit for bit, so
device results are compared with `bits_equal`, never with a tolerance."""
import numpy as np

BAN = np.float32(-np.finfo(np.float32).max)  # "ban" stores -FLT_MAX, never -inf


def params(repetition_penalty=1.0, no_repeat_ngram=0, min_new_tokens=0, eos_id=-1, bias=(), bad_tokens=()):
    """The state of one row.  bias: (token, value) pairs in entry order; bad_tokens: entries of -inf after them."""
    ent = [(int(t), float(v)) for t, v in (bias.items() if isinstance(bias, dict) else bias)]
    ent += [(int(t), float("-inf")) for t in bad_tokens]
    return {"repetition_penalty": float(repetition_penalty), "no_repeat_ngram": int(no_repeat_ngram),
            "min_new_tokens": int(min_new_tokens), "eos_id": int(eos_id), "bias": ent}


def apply(logits, history, p, n_generated=0, *, penalty_per_occurrence=False, bias_after_penalty=False):
    """Processed copy of fp32 logits [V] for a row whose history is `history` (prompt + generated tokens, in order) and
    which has generated `n_generated` tokens since its state was set.  The two keyword switches build deliberately
    WRONG variants (the penalty once per occurrence instead of once per distinct token; bias and penalty swapped):
    tests use them to show that the comparison rejects such results."""
    l = np.array(logits, dtype=np.float32).reshape(-1).copy()
    T = [int(t) for t in history]
    r = np.float32(p["repetition_penalty"])

    def bias():
        for t, v in p["bias"]:
            if np.isfinite(v):
                l[t] = np.float32(l[t] + np.float32(v))

    def penalty():
        for v in (T if penalty_per_occurrence else sorted(set(T))):
            x = l[v]
            l[v] = np.float32(x * r) if x < 0 else np.float32(x / r)  # -0.0 < 0 is false

    if bias_after_penalty:
        penalty(); bias()
    else:
        bias(); penalty()
    n = p["no_repeat_ngram"]
    if n > 0 and len(T) + 1 >= n:
        last = T[len(T) - (n - 1):] if n > 1 else []
        for i in range(len(T) - n + 1):
            if T[i:i + n - 1] == last:
                l[T[i + n - 1]] = BAN
    for t, v in p["bias"]:
        if v == float("-inf"):
            l[t] = BAN
    if p["eos_id"] >= 0 and n_generated < p["min_new_tokens"]:
        l[p["eos_id"]] = BAN
    return l


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def first_argmax(logits):
    l = np.asarray(logits, np.float32).reshape(-1) + np.float32(0.0)
    return int(np.argmax(l))


def generate(logits_fn, prompt, p, steps, pick=None):
    """A per-sample loop: logits_fn(tokens) -> raw fp32 logits [V] of the next position; returns (ids, the processed
    logits of every step).  pick(processed, position) -> token, default the first index of the largest logit."""
    T = [int(t) for t in prompt]
    out, scores = [], []
    for g in range(steps):
        proc = apply(logits_fn(T), T, p, n_generated=g)
        tok = first_argmax(proc) if pick is None else int(pick(proc, len(T)))
        scores.append(proc)
        out.append(tok)
        T.append(tok)
    return out, scores
