"""TEST INFRASTRUCTURE: float64 restatement of the per-row sampling rule (include/bloomstage.h "Per-row sampling",
DESIGN.md section 5g) and the tolerant checker of a device draw.

The device works on 2^40 fixed-point weights from fp32 arithmetic, so a draw may differ from this float64 rule where
a threshold falls within the arithmetic's error.  The checker therefore does not compare tokens: given the logits, the
state and the device's read-out (t, |N|, |C|, u24, token) it asserts that the read-out is a correct answer up to

    EPS = 2^-16 relative on every mass, plus V * 2^-39 absolute on the two running masses of the pick.

EPS is derived, not measured: the weight's argument (l_v - max l) / temperature carries two fp32 roundings, at most
|arg| * 2^-23 for the |arg| <= 40 that can matter (exp(-40) * 2^40 rounds to zero), i.e. a relative 2^-17.7 on
exp(arg); expf adds one ulp (2^-23); the fixed-point quantisation adds V * 2^-41 <= 2^-23 in total against a mass
>= 1.  The sum is about 2^-17, and the bound doubles it.
"""
import numpy as np

from oracle.gen_np import M64, gen_bits, sm64
from oracle.sampling_ref import order_key

ROW_TAG = 0x524F575300000000  # "ROWS": the key tag of the per-row draws (topk_sample_kernel's is 0x5A4D504C...)
EPS = 2.0 ** -16


def draw_u24(seed, pos):
    """Top 24 bits of the counter generator keyed by (seed, position); the KV row is not in the key."""
    key = sm64((int(seed) ^ sm64(ROW_TAG)) & M64)
    return int(gen_bits(key, np.uint32(int(pos) & 0xFFFFFFFF))) >> 8


def _prep(logits, top_k, top_p, temperature):
    l32 = np.asarray(logits, np.float32).reshape(-1) + np.float32(0.0)  # -0.0 and +0.0 are one level
    l = l32.astype(np.float64)
    temp = float(np.float32(temperature))
    w = np.exp((l - l.max()) / temp)
    V = l.size
    if top_k == 0 or top_k >= V:
        tk = -np.inf
    else:
        tk = np.partition(l, V - top_k)[V - top_k]  # the top_k-th largest value
    return l, w, tk, float(np.float32(top_p))


def reference(logits, top_k, top_p, temperature, seed, pos):
    """The rule in float64: {"t", "n_nucleus", "n_candidates", "u24", "token", "mass_nucleus", "mass_candidates"}."""
    l, w, tk, p = _prep(logits, top_k, top_p, temperature)
    cand = l >= tk
    mass_c = w[cand].sum()
    idx = np.flatnonzero(cand)
    order = idx[np.argsort(-l[idx], kind="stable")]
    ls, cum = l[order], np.cumsum(w[order])
    ends = np.flatnonzero(np.append(ls[1:] != ls[:-1], True))  # last member of every level, top level first
    reach = np.flatnonzero(cum[ends] >= p * mass_c)
    t = ls[ends[reach[0] if reach.size else -1]]
    nuc = l >= t
    mass_n = w[nuc].sum()
    u24 = draw_u24(seed, pos)
    run = np.cumsum(np.where(nuc, w, 0.0))
    hit = np.flatnonzero(nuc & (run > (u24 / 2.0 ** 24) * mass_n))
    token = int(hit[0]) if hit.size else int(np.flatnonzero(nuc)[-1])
    return {"t": float(t), "n_nucleus": int(nuc.sum()), "n_candidates": int(cand.sum()), "u24": u24, "token": token,
            "mass_nucleus": float(mass_n), "mass_candidates": float(mass_c)}


def check_draw(logits, top_k, top_p, temperature, seed, pos, t, n_nucleus, n_candidates, u24, token, what=""):
    """Assert that a device read-out is a correct draw within EPS (module docstring).  No case is excluded."""
    l, w, tk, p = _prep(logits, top_k, top_p, temperature)
    V = l.size
    t = float(np.float32(t) + np.float32(0.0))
    assert t >= tk, f"{what}: threshold {t} below the top-k level {tk}"
    assert n_candidates == int((l >= tk).sum()), f"{what}: |C| = {n_candidates}, the logits give {int((l >= tk).sum())}"
    nuc = l >= t
    assert n_nucleus == int(nuc.sum()), f"{what}: |N| = {n_nucleus}, the logits give {int(nuc.sum())} at t = {t}"
    assert n_nucleus >= 1, f"{what}: empty nucleus"
    mass_c = w[l >= tk].sum()
    mass_ge, mass_gt = w[nuc].sum(), w[l > t].sum()
    assert mass_ge >= p * mass_c * (1 - EPS), \
        f"{what}: nucleus short: mass(l >= t) = {mass_ge!r} < top_p * mass(C) = {p * mass_c!r}"
    assert mass_gt <= p * mass_c * (1 + EPS), \
        f"{what}: nucleus long: mass(l > t) = {mass_gt!r} > top_p * mass(C) = {p * mass_c!r}"
    assert u24 == draw_u24(seed, pos), f"{what}: u24 = {u24}, the generator gives {draw_u24(seed, pos)} at {pos}"
    assert 0 <= token < V and nuc[token] and w[token] > 0, f"{what}: token {token} is not a weighted member of N"
    target = (u24 / 2.0 ** 24) * mass_ge
    before = w[:token][nuc[:token]].sum()
    through = before + w[token]
    slack = V * 2.0 ** -39
    assert before <= target * (1 + EPS) + slack, \
        f"{what}: token {token} late: mass before it {before!r} > u * mass(N) = {target!r}"
    assert through >= target * (1 - EPS) - slack, \
        f"{what}: token {token} early: mass through it {through!r} < u * mass(N) = {target!r}"


def check_readout(logits, state, pos, draw, what=""):
    """check_draw on a Stage.read_row_draw dict; state = (top_k, top_p, temperature, seed)."""
    top_k, top_p, temperature, seed = state
    check_draw(logits, top_k, top_p, temperature, seed, pos, draw["threshold"], draw["n_nucleus"],
               draw["n_candidates"], draw["u24"], draw["token"], what)


def first_argmax(logits):
    l = np.asarray(logits, np.float32).reshape(-1) + np.float32(0.0)
    return int(np.argmax(l))


def fixture(kind, V, seed=0):
    """Constructed logits [V] fp32: "normal" (N(0, 2^2)), "tied" (integer-rounded: many ties at every level),
    "spike" (one logit 30 above the rest: |N| == 1), "equal" (one level)."""
    rng = np.random.default_rng(1000 + seed)
    l = (rng.standard_normal(V) * 2.0).astype(np.float32)
    if kind == "normal":
        return l
    if kind == "tied":
        return np.rint(l).astype(np.float32)
    if kind == "spike":
        l[int(rng.integers(V))] = l.max() + np.float32(30.0)
        return l
    if kind == "equal":
        return np.full(V, 1.25, np.float32)
    raise ValueError(kind)


def device_model(logits, top_k, top_p, temperature, seed, pos, ulp=0):
    """A host model of the device arithmetic (fp32 argument, expf moved by `ulp` ulps, 2^40 fixed point, exact integer
    thresholds): a draw in check_draw's argument order.  Shows on the CPU that the checker accepts what the kernel
    is specified to compute."""
    l = np.asarray(logits, np.float32).reshape(-1) + np.float32(0.0)
    V = l.size
    arg = ((l - l.max()).astype(np.float32) / np.float32(temperature)).astype(np.float32)
    w = np.exp(arg.astype(np.float64)).astype(np.float32)
    if ulp:
        w = np.where((arg < 0) & (w > 1e-30), (w.view(np.uint32).astype(np.int64) + ulp).astype(np.uint32).view(np.float32), w)
    q = np.rint(w.astype(np.float64) * 2.0 ** 40).astype(np.uint64)  # sums stay below 2^58: exact in uint64
    keys = order_key(l)
    tk = 0 if top_k == 0 or top_k >= V else int(np.sort(keys)[V - top_k])
    idx = np.flatnonzero(keys >= tk)
    mass_c = int(q[idx].sum(dtype=np.uint64))
    mant, ex = np.frexp(np.float64(np.float32(top_p)))
    m24, sh = int(mant * 2 ** 24), 24 - int(ex)  # top_p = m24 * 2^-sh exactly
    thr = -((-m24 * mass_c) >> sh)  # ceil(top_p * mass(C))
    order = idx[np.argsort(-keys[idx].astype(np.int64), kind="stable")]
    ks, cum = keys[order], np.cumsum(q[order], dtype=np.uint64)
    ends = np.flatnonzero(np.append(ks[1:] != ks[:-1], True))
    end = ends[np.flatnonzero(cum[ends] >= np.uint64(thr))[0]]
    t_key, mass_n = int(ks[end]), int(cum[end])
    u24 = draw_u24(seed, pos)
    target = (u24 * mass_n) >> 24
    nuc = keys >= t_key
    run = np.cumsum(np.where(nuc, q, np.uint64(0)), dtype=np.uint64)
    token = int(np.flatnonzero(nuc & (run > np.uint64(target)))[0])
    return float(l[order[end]]), int(end) + 1, int(idx.size), u24, token
