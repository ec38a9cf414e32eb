"""Token automata for guided decoding (include/bloomstage.h "Guided decoding").

A Guide is a DFA over token ids in CSR form: state q owns the edges row_ptr[q] .. row_ptr[q + 1), each a token (strictly
ascending inside a state) and a next state, and a default next state for every other token; -1 means "not allowed".
The library takes exactly these tables (Stage.load_guide); compiling a regex or a grammar against a tokenizer is the
caller's business -- from_state_maps takes what such front ends emit.  Host only, numpy only."""
import json
from dataclasses import dataclass

import numpy as np

MAX_STATES = 1 << 20
TABLES = ("row_ptr", "edge_token", "edge_next", "default_next")


@dataclass
class Guide:
    n_states: int
    start: int
    row_ptr: np.ndarray
    edge_token: np.ndarray
    edge_next: np.ndarray
    default_next: np.ndarray

    def __post_init__(self):
        for k in TABLES:
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.int32).reshape(-1))

    # ---- the rule
    def step(self, state, token):
        """The state after `token` in `state`, or -1 if the token is not allowed there."""
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        e = lo + int(np.searchsorted(self.edge_token[lo:hi], token))
        if e < hi and self.edge_token[e] == token:
            return int(self.edge_next[e])
        return int(self.default_next[state])

    def allowed(self, state, vocab=None):
        """The sorted token ids allowed in `state`; a default-allow state needs the vocabulary size."""
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        tok, nxt = self.edge_token[lo:hi], self.edge_next[lo:hi]
        if self.default_next[state] < 0:
            return tok[nxt >= 0].astype(np.int64)
        if vocab is None:
            raise ValueError(f"state {state} allows by default: allowed() needs the vocabulary size")
        mask = np.ones(vocab, bool)
        mask[tok[nxt < 0]] = False
        return np.flatnonzero(mask)

    def walk(self, tokens, state=None):
        """(state, n_rejected) after `tokens`: a token that is not allowed leaves the state and counts as rejected."""
        q, rej = self.start if state is None else state, 0
        for t in tokens:
            n = self.step(q, int(t))
            if n >= 0:
                q = n
            else:
                rej += 1
        return q, rej

    def validate(self, vocab):
        """Raise ValueError, naming the offending state, unless the tables are what bs_load_guide accepts."""
        n = self.n_states
        if not 1 <= n <= MAX_STATES:
            raise ValueError("n_states must be in [1, 2^20]")
        if not 0 <= self.start < n:
            raise ValueError("start state outside [0, n_states)")
        if self.row_ptr.size != n + 1 or self.default_next.size != n:
            raise ValueError("row_ptr needs n_states + 1 entries and default_next n_states")
        if self.row_ptr[0] != 0:
            raise ValueError("row_ptr must start at 0 (state 0)")
        d = np.flatnonzero(np.diff(self.row_ptr) < 0)
        if d.size:
            raise ValueError(f"row_ptr decreases at state {int(d[0])}")
        if self.edge_token.size != self.row_ptr[n] or self.edge_next.size != self.row_ptr[n]:
            raise ValueError("edge_token and edge_next need row_ptr[n_states] entries")
        for q in range(n):
            at = f" in state {q}"
            dn = int(self.default_next[q])
            if not -1 <= dn < n:
                raise ValueError("default_next outside [-1, n_states)" + at)
            tok = self.edge_token[self.row_ptr[q]:self.row_ptr[q + 1]]
            nxt = self.edge_next[self.row_ptr[q]:self.row_ptr[q + 1]]
            if tok.size and (tok.min() < 0 or tok.max() >= vocab):
                raise ValueError("edge token outside [0, vocab)" + at)
            if np.any(np.diff(tok) <= 0):
                raise ValueError("edge tokens not strictly ascending" + at)
            if nxt.size and (nxt.min() < -1 or nxt.max() >= n):
                raise ValueError("edge_next outside [-1, n_states)" + at)
            allowed = vocab - int((nxt < 0).sum()) if dn >= 0 else int((nxt >= 0).sum())
            if allowed <= 0:
                raise ValueError("no token is allowed" + at)
        return self

    # ---- JSON: the tables and nothing else
    def to_json(self):
        d = {"n_states": int(self.n_states), "start": int(self.start)}
        d.update({k: getattr(self, k).tolist() for k in TABLES})
        return json.dumps(d)

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        return cls(int(d["n_states"]), int(d["start"]), *[d[k] for k in TABLES])

    @classmethod
    def from_file(cls, path):
        with open(path) as f:
            return cls.from_json(f.read())


def _encode(states, start, vocab):
    """states: per state a dict token -> next (the allowed tokens).  Each state takes the encoding with fewer edges:
    default-ban (one edge per allowed token) or, when the vocabulary size is known, default-allow to its most frequent
    next state (one edge per token that goes elsewhere, one ban edge per token that is not allowed)."""
    row_ptr, tok, nxt, dflt = [0], [], [], []
    for m in states:
        edges, dn = sorted(m.items()), -1
        if vocab is not None and m:
            nexts = list(m.values())
            best = max(sorted(set(nexts)), key=nexts.count)
            n_allow = sum(1 for v in nexts if v != best) + (vocab - len(m))
            if n_allow < len(m):
                dn = best
                other = {t: v for t, v in m.items() if v != best}
                other.update({t: -1 for t in range(vocab) if t not in m})
                edges = sorted(other.items())
        tok += [t for t, _ in edges]
        nxt += [v for _, v in edges]
        dflt.append(dn)
        row_ptr.append(len(tok))
    return Guide(len(states), start, row_ptr, tok, nxt, dflt)


def from_choices(sequences, eos_id, vocab=None):
    """A trie over token-id sequences: exactly one of them is generated, then only eos_id.  A completed sequence enters
    a sink state that allows only eos_id; a sequence that is a prefix of another may end (eos_id) or go on."""
    seqs = sorted({tuple(int(t) for t in s) for s in sequences})
    if not seqs or any(len(s) == 0 for s in seqs):
        raise ValueError("from_choices needs at least one sequence, none of them empty")
    eos_id = int(eos_id)
    done = set(seqs)
    inner = sorted({s[:i] for s in seqs for i in range(len(s))} | {s for s in seqs if any(o[:len(s)] == s and o != s for o in seqs)})
    ids = {p: i for i, p in enumerate(inner)}  # () is first: state 0
    sink = len(inner)
    states = [dict() for _ in range(sink + 1)]
    for s in seqs:
        for i in range(len(s)):
            states[ids[s[:i]]][s[i]] = ids.get(s[:i + 1], sink)
    for p in inner:
        if p in done:
            states[ids[p]][eos_id] = sink
    states[sink][eos_id] = sink
    g = _encode(states, 0, vocab)
    return g.validate(vocab if vocab is not None else max(max(max(s) for s in seqs), eos_id) + 1)


def from_state_maps(maps, start, finals, eos_id, vocab):
    """The state -> {token -> next state} dictionary that guided-decoding front ends emit (any hashable state names);
    `finals` additionally allow eos_id into a sink state that allows only eos_id."""
    names = list(maps)
    for m in maps.values():
        names += [v for v in m.values() if v not in maps]
    names += [f for f in finals if f not in maps]
    order = sorted(set(names), key=lambda x: (str(type(x)), x))
    ids = {name: i for i, name in enumerate(order)}
    finals = set(finals)
    sink = len(order) if finals else None
    states = []
    for name in order:
        m = {int(t): ids[v] for t, v in maps.get(name, {}).items()}
        if name in finals:
            m[int(eos_id)] = sink
        states.append(m)
    if finals:
        states.append({int(eos_id): sink})
    return _encode(states, ids[start], int(vocab)).validate(int(vocab))
