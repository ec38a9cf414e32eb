"""The canonical weight order of a stage (csrc/stage_weights.h), host side: for every stage position and head option,
bs_stage_weight_count and the pre-device check of bs_init_stage_file against this file's own restatement of the
order -- which tensors a stage holds, under which checkpoint names and shapes, and how many elements it takes of each.
The restatement is written out here; nothing of it is read from the library."""
import re

import pytest
import torch
from safetensors.torch import save_file

from distributed_inference_demo_amd import stage as bs
from distributed_inference_demo_amd.stage import BloomStageError, Stage

H, NH, L, V = 64, 4, 4, 512
SLICE = (64, 192)
POSITIONS = {"first": (0, 2, 1, 0), "middle": (1, 3, 0, 0), "last": (2, 4, 0, 1), "whole": (0, 4, 1, 1)}
# (position, head slice, n_labels): a classifier needs the last stage and takes no head slice
CASES = [(p, s, 0) for p in POSITIONS for s in (None, SLICE)] + [("last", None, 3), ("whole", None, 3)]
BLOCK = [("input_layernorm.weight", (H,)), ("input_layernorm.bias", (H,)),
         ("self_attention.query_key_value.weight", (3 * H, H)), ("self_attention.query_key_value.bias", (3 * H,)),
         ("self_attention.dense.weight", (H, H)), ("self_attention.dense.bias", (H,)),
         ("post_attention_layernorm.weight", (H,)), ("post_attention_layernorm.bias", (H,)),
         ("mlp.dense_h_to_4h.weight", (4 * H, H)), ("mlp.dense_h_to_4h.bias", (4 * H,)),
         ("mlp.dense_4h_to_h.weight", (H, 4 * H)), ("mlp.dense_4h_to_h.bias", (H,))]


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def canonical(pos, head, n_labels):
    """[(checkpoint tensor, its shape, elements the stage takes of it)] in BS_WEIGHTS_HOST order."""
    lb, le, first, last = POSITIONS[pos]
    ln_f = [("ln_f.weight", (H,), H), ("ln_f.bias", (H,), H)]
    owns_embedding = first or (last and not n_labels)
    out = []
    if owns_embedding:
        out.append(("word_embeddings.weight", (V, H), V * H))
    if first:
        out += [("word_embeddings_layernorm.weight", (H,), H), ("word_embeddings_layernorm.bias", (H,), H)]
    for l in range(lb, le):
        out += [(f"h.{l}.{n}", s, numel(s)) for n, s in BLOCK]
    if last:
        out += ln_f
    if n_labels:
        out.append(("score.weight", (n_labels, H), n_labels * H))
    if head:
        if not owns_embedding:  # its rows of the embedding, held on their own
            out.append(("word_embeddings.weight", (V, H), (head[1] - head[0]) * H))
        if not last:
            out += ln_f
    return out


def desc_kw(pos, head, n_labels):
    lb, le, first, last = POSITIONS[pos]
    kw = dict(hidden=H, n_head=NH, n_layer=L, vocab=V, ln_eps=1e-5, layer_begin=lb, layer_end=le, is_first=first,
              is_last=last, dtype=16, max_batch=1, max_ctx=8)
    if head:
        kw.update(head_vocab_begin=head[0], head_vocab_end=head[1])
    if n_labels:
        kw.update(flags=bs.BS_FLAG_CLASSIFIER, n_labels=n_labels)
    return kw


def init_status(path, pos, head, n_labels):
    """(status, message) of bs_init_stage_file; a stage that came up is released again."""
    lb, le, first, last = POSITIONS[pos]
    try:
        Stage(H, NH, L, V, lb, le, dtype="bf16", max_ctx=8, is_first=first, is_last=last, head_slice=head,
              n_labels=n_labels, weights_file=path).close()
        return 0, ""
    except BloomStageError as e:
        return int(re.match(r"bloomstage error (-?\d+):", str(e)).group(1)), str(e)


@pytest.mark.parametrize("pos,head,n_labels", CASES, ids=[f"{p}-{'slice' if s else 'cls' if n else 'plain'}" for p, s, n in CASES])
def test_count_and_file_check_follow_the_canonical_order(tmp_path, pos, head, n_labels):
    order = canonical(pos, head, n_labels)
    assert bs.weight_count(**desc_kw(pos, head, n_labels)) == sum(n for _, _, n in order)
    tensors = {name: torch.zeros(shape, dtype=torch.bfloat16) for name, shape, _ in order}
    full = str(tmp_path / "full.safetensors")
    save_file(tensors, full)
    rc, msg = init_status(full, pos, head, n_labels)
    # every tensor found and shaped right: the call gets as far as the device (and fails there without one)
    assert rc == (0 if torch.cuda.is_available() else -2), msg
    for gone in tensors:
        f = str(tmp_path / "less.safetensors")
        save_file({k: v for k, v in tensors.items() if k != gone}, f)
        rc, msg = init_status(f, pos, head, n_labels)
        assert rc == -1 and f"no tensor '{gone}'" in msg, (gone, rc, msg)
