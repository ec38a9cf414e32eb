"""LoRA adapters for `Stage.load_adapter` (include/bloomstage.h "Per-row LoRA adapters").

An adapter holds, for each adapted linear of a stage's local layers, PEFT's two matrices in PEFT's orientation:
`lora_A.weight` [rank][K] and `lora_B.weight` [N][rank]; the layer computes `W x + scale * B (A x)`, scale = alpha / rank.
Targets are BLOOM's `self_attention.query_key_value` (PEFT's standard BLOOM recipe), `self_attention.dense` and
`mlp.dense_4h_to_h`.
"""
import re

import numpy as np

BS_LORA_QKV, BS_LORA_DENSE, BS_LORA_FC2 = 1, 2, 4
TARGETS = ("qkv", "dense", "fc2")  # index t <-> mask bit 1 << t
TARGET_BITS = {"qkv": BS_LORA_QKV, "dense": BS_LORA_DENSE, "fc2": BS_LORA_FC2}
PEFT_MODULES = {"self_attention.query_key_value": "qkv", "self_attention.dense": "dense", "mlp.dense_4h_to_h": "fc2"}


def target_shape(target, hidden):
    """(K, N) of a target's linear."""
    return (4 * hidden if target == "fc2" else hidden, 3 * hidden if target == "qkv" else hidden)


def bf16_round(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32: what the device keeps of A and B."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


class Adapter:
    """rank, scale and, per target name, A fp32 [layers][rank][K] and B fp32 [layers][N][rank]."""

    def __init__(self, rank, scale, a, b):
        self.rank, self.scale = int(rank), float(scale)
        self.a = {t: np.ascontiguousarray(v, dtype=np.float32) for t, v in a.items()}
        self.b = {t: np.ascontiguousarray(v, dtype=np.float32) for t, v in b.items()}
        if set(self.a) != set(self.b) or not set(self.a) <= set(TARGETS):
            raise ValueError(f"adapter targets {sorted(self.a)} / {sorted(self.b)}: the same subset of {TARGETS}")
        for t in self.a:
            la, r, _ = self.a[t].shape
            lb, _, rb = self.b[t].shape
            if (la, r, rb) != (lb, self.rank, self.rank):
                raise ValueError(f"adapter target {t}: A {self.a[t].shape} and B {self.b[t].shape} at rank {self.rank}")

    @property
    def targets(self):
        return sum(TARGET_BITS[t] for t in self.a)


def synthetic(seed, rank, targets, hidden, layers, amplitude=1.0):
    """A reproducible adapter for tests and benchmarks: normal A and B, scaled so that a unit-variance input gives a
    delta of about `amplitude` per output element; scale = 2 (alpha = 2 * rank)."""
    rng = np.random.default_rng(seed)
    a, b = {}, {}
    for t in targets:
        K, N = target_shape(t, hidden)
        a[t] = (rng.standard_normal((layers, rank, K)) / np.sqrt(K)).astype(np.float32)
        b[t] = (rng.standard_normal((layers, N, rank)) * (amplitude / (2.0 * np.sqrt(rank)))).astype(np.float32)
    return Adapter(rank, 2.0, a, b)


_PEFT_NAME = re.compile(r"(?:^|\.)h\.(\d+)\.(self_attention\.query_key_value|self_attention\.dense|mlp\.dense_4h_to_h)"
                        r"\.lora_([AB])(?:\.[^.]+)?\.weight$")


def from_peft_tensors(tensors, alpha, rank, layer_begin, layer_end):
    """An Adapter for layers [layer_begin, layer_end) from a dict of PEFT tensor names to arrays, e.g.
    `base_model.model.transformer.h.3.self_attention.query_key_value.lora_A.weight` (an adapter name between `lora_A`
    and `weight`, as in `lora_A.default.weight`, is accepted).  A target must be present for every layer of the range
    or for none; other names are ignored."""
    found = {}
    for name, arr in tensors.items():
        m = _PEFT_NAME.search(name)
        if m and layer_begin <= int(m.group(1)) < layer_end:
            found[(PEFT_MODULES[m.group(2)], m.group(3), int(m.group(1)))] = np.asarray(arr, dtype=np.float32)
    a, b = {}, {}
    for t in TARGETS:
        have = [l for l in range(layer_begin, layer_end) if (t, "A", l) in found and (t, "B", l) in found]
        if not have:
            continue
        if len(have) != layer_end - layer_begin:
            raise ValueError(f"adapter target {t}: layers {have} of [{layer_begin}, {layer_end})")
        a[t] = np.stack([found[(t, "A", l)] for l in have])
        b[t] = np.stack([found[(t, "B", l)] for l in have])
    if not a:
        raise ValueError("no lora_A / lora_B tensors of the layer range")
    return Adapter(rank, float(alpha) / rank, a, b)


def matrix_offsets(hidden, layers, vocab, first=True, last=True):
    """{(local layer, target): offset} of the three adaptable matrices in the stage's canonical host-weight vector
    (bs_stage_weight_count's order)."""
    h = hidden
    off = (vocab * h if first or last else 0) + (2 * h if first else 0)
    out = {}
    for l in range(layers):
        off += 2 * h                      # ln1
        out[(l, "qkv")] = off
        off += 3 * h * h + 3 * h
        out[(l, "dense")] = off
        off += h * h + h + 2 * h          # dense w, b, ln2
        off += 4 * h * h + 4 * h          # fc1
        out[(l, "fc2")] = off
        off += 4 * h * h + h
    return out


def merged_weights(canonical_weights, adapter, hidden, vocab, first=True, last=True):
    """The stage's canonical host-weight vector with W + scale * bf16(B) . bf16(A) formed in float64 for every adapted
    matrix (the model a merged deployment would serve; the stage rounds it to bf16 on upload)."""
    w = np.array(canonical_weights, dtype=np.float32).reshape(-1)
    layers = next(iter(adapter.a.values())).shape[0]
    offs = matrix_offsets(hidden, layers, vocab, first, last)
    for t in adapter.a:
        K, N = target_shape(t, hidden)
        for l in range(layers):
            o = offs[(l, t)]
            d = bf16_round(adapter.b[t][l]).astype(np.float64) @ bf16_round(adapter.a[t][l]).astype(np.float64)
            w[o:o + N * K] = (w[o:o + N * K].astype(np.float64) + adapter.scale * d.reshape(-1)).astype(np.float32)
    return w
