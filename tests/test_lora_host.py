"""lora.py on the host: PEFT tensor names to targets, and merged weights in the canonical stage order."""
import numpy as np
import pytest

from distributed_inference_demo_amd import lora

H, V, RANK = 32, 64, 3


def peft_tensors(layers):
    rng = np.random.default_rng(0)
    out = {}
    for l in layers:
        for mod, t in lora.PEFT_MODULES.items():
            K, N = lora.target_shape(t, H)
            if t == "dense":
                continue  # PEFT's BLOOM recipes adapt query_key_value (and here dense_4h_to_h), not every module
            base = f"base_model.model.transformer.h.{l}.{mod}"
            out[f"{base}.lora_A.default.weight"] = rng.standard_normal((RANK, K)).astype(np.float32)
            out[f"{base}.lora_B.weight"] = rng.standard_normal((N, RANK)).astype(np.float32)
    out["base_model.model.transformer.h.0.mlp.dense_h_to_4h.lora_A.weight"] = np.zeros((RANK, H), np.float32)
    return out


def test_from_peft_tensors_maps_names_and_layer_range():
    t = peft_tensors(range(4))
    ad = lora.from_peft_tensors(t, alpha=6, rank=RANK, layer_begin=1, layer_end=3)
    assert ad.scale == 2.0 and ad.targets == lora.BS_LORA_QKV | lora.BS_LORA_FC2
    assert ad.a["qkv"].shape == (2, RANK, H) and ad.b["qkv"].shape == (2, 3 * H, RANK)
    assert ad.a["fc2"].shape == (2, RANK, 4 * H) and ad.b["fc2"].shape == (2, H, RANK)
    k = "base_model.model.transformer.h.2.mlp.dense_4h_to_h.lora_B.weight"
    assert np.array_equal(ad.b["fc2"][1], t[k])
    with pytest.raises(ValueError):
        lora.from_peft_tensors(peft_tensors([0, 2]), 6, RANK, 0, 3)  # layer 1 is missing


@pytest.mark.parametrize("first,last", [(True, True), (False, False), (False, True)])
def test_merged_weights_changes_the_adapted_matrices_only(first, last):
    layers = 2
    ad = lora.synthetic(3, RANK, ["qkv", "fc2"], H, layers)
    per_layer = 12 * H * H + 13 * H
    n = (V * H if first or last else 0) + (2 * H if first else 0) + layers * per_layer + (2 * H if last else 0)
    w = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    m = lora.merged_weights(w, ad, H, V, first, last)
    offs = lora.matrix_offsets(H, layers, V, first, last)
    changed = np.zeros(n, bool)
    for l in range(layers):
        for t in ("qkv", "fc2"):
            K, N = lora.target_shape(t, H)
            o = offs[(l, t)]
            changed[o:o + N * K] = True
            d = ad.scale * lora.bf16_round(ad.b[t][l]).astype(np.float64) @ lora.bf16_round(ad.a[t][l]).astype(np.float64)
            assert np.abs(m[o:o + N * K].reshape(N, K) - (w[o:o + N * K].reshape(N, K) + d)).max() <= 2.0 ** -22
    assert np.array_equal(m[~changed], w[~changed]) and np.all(m[changed] != w[changed])
    assert offs[(layers - 1, "fc2")] + 4 * H * H + H == n - (2 * H if last else 0)
