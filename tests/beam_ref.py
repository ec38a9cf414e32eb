"""tests/beam_ref.py — TEST INFRASTRUCTURE: beam search as transformers' `_beam_search` runs it (generation/utils.py,
generate(num_beams=W, do_sample=False, early_stopping=False)), restated in numpy array steps, one per step of that
function: no KV reuse (every hypothesis' whole sequence is fed again), full-vocabulary log-softmax, a flat top-2W over
W * V.  Pinned to transformers by tests/golden/tiny_beam.npz (tests/test_beam_host.py); the product's
beam.BeamSearcher is checked against it.

Two deliberate restatements: cumulative scores are float64 (transformers: fp32; the fixture records the difference
and the selection margins), and every top-k ranks equal scores by the lower index (torch.topk leaves it open).
"""
import numpy as np

NEG = -1.0e9


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def topk(x, k):
    """Indices of the k largest of a 1-d array, best first, the lower index first among equals."""
    return np.argsort(-x, kind="stable")[:k]


def search(logits_fn, prompt, max_new, num_beams, length_penalty=1.0, eos=None, num_return=1, stats=None):
    """logits_fn(sequences) -> [len(sequences)][V] logits of each token list's last position.
    Returns (sequences, scores): the num_return best finished hypotheses' generated tokens (an eos included) and
    scores.  stats (a dict): 'min_gap' receives the smallest score gap between the last kept and the first dropped
    candidate over all steps (the flat top-2W cut, the running top-W cut, the cut between the W candidates that may
    finish and the rest, the finished top-W cut) and between the returned hypotheses' scores."""
    W, K, P = num_beams, 2 * num_beams, len(prompt)
    run_seq = [list(prompt) for _ in range(W)]
    run_score = np.full(W, NEG)
    run_score[0] = 0.0
    fin_seq = [list(prompt) for _ in range(W)]
    fin_score = np.full(W, NEG)
    fin_done = np.zeros(W, bool)
    min_gap = np.inf
    cur = P
    while True:
        lp = log_softmax64(logits_fn(run_seq))                      # b. log probs + running scores
        V = lp.shape[1]
        acc = (lp + run_score[:, None]).reshape(-1)
        order = topk(acc, K + 1)                                    # c. top-K continuations (one more: the gap)
        min_gap = min(min_gap, acc[order[K - 1]] - acc[order[K]])
        idx = order[:K]
        top_lp = acc[idx]
        top_seq = [run_seq[i // V] + [int(i % V)] for i in idx]
        hit = np.array([(eos is not None and s[-1] == eos) or len(s) >= P + max_new for s in top_seq])  # d.
        run_lp = top_lp + hit * NEG                                 # e. running beams of the next iteration
        nxt = topk(run_lp, W + 1) if K > W else topk(run_lp, W)
        if not hit.all() and len(nxt) > W and run_lp[nxt[W]] > NEG / 2:
            min_gap = min(min_gap, run_lp[nxt[W - 1]] - run_lp[nxt[W]])
        nxt = nxt[:W]
        new_seq, new_score = [top_seq[i] for i in nxt], run_lp[nxt]
        just = hit & (np.arange(K) < W)                             # f. finished beams
        if hit.any():  # only the W best of the 2W may finish: that cut decides too
            min_gap = min(min_gap, top_lp[W - 1] - top_lp[W])
        f_lp = top_lp / ((cur + 1 - P) ** length_penalty) + (~just) * NEG
        m_seq = fin_seq + top_seq
        m_score = np.concatenate([fin_score, f_lp])
        m_done = np.concatenate([fin_done, just])
        keep = topk(m_score, W + 1)
        if m_score[keep[W]] > NEG / 2:
            min_gap = min(min_gap, m_score[keep[W - 1]] - m_score[keep[W]])
        keep = keep[:W]
        fin_seq, fin_score, fin_done = [m_seq[i] for i in keep], m_score[keep], m_done[keep]
        run_seq, run_score = new_seq, new_score
        cur += 1                                                    # g. the stopping condition
        best_possible = run_score[0] / ((cur - P) ** length_penalty)
        worst = np.where(fin_done, fin_score.min(), NEG)
        if fin_done.all():  # the early-stop decision has a margin too
            min_gap = min(min_gap, abs(best_possible - fin_score.min()))
        if not (best_possible > worst).any() or hit.all():
            break
    for a, b in zip(fin_score[:num_return], fin_score[1:num_return]):  # the order of the returned hypotheses
        min_gap = min(min_gap, a - b)
    if stats is not None:
        stats["min_gap"] = float(min_gap)
    return [s[P:] for s in fin_seq[:num_return]], [float(v) for v in fin_score[:num_return]]
