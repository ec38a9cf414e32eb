"""serve --adapters on one GPU: 6 samples over 3 rows in flight, sample i on adapter i % 3 - 1.  Every sample's ids are
checked against a stage built from its adapter's merged weights (the base weights for -1) that is fed the served ids
(teacher forcing, so one near-tie cannot cascade), under the top-2 margin rule; the base-model samples equal a run
without the option."""
import numpy as np
import pytest
import torch

from distributed_inference_demo_amd import lora
from distributed_inference_demo_amd.config import BloomDims
from distributed_inference_demo_amd.serve import RunConfig, run_rank, synthetic_prompts
from distributed_inference_demo_amd.stage import Stage
from test_gpu_parity import assert_ids_match, canonical_weights

pytestmark = pytest.mark.gpu


def test_serve_adapters_match_merged_weights_per_sample():
    h, L, nh, V, n_new = 256, 2, 4, 1024, 8
    model = BloomDims("tinygpu", h, L, nh, vocab=V)
    kw = dict(model=model, num_sample=6, max_length=n_new, core_pool_size=3, prompt_len=9, seed=11)
    cfg = RunConfig(adapters=2, adapter_rank=8, adapter_amplitude=4.0, **kw)  # large enough to change tokens
    res = run_rank(cfg, 0, 1, torch.device("cuda", 0))
    base = run_rank(RunConfig(**kw), 0, 1, torch.device("cuda", 0))
    assert res["sample_adapters"] == [-1, 0, 1, -1, 0, 1]
    w = canonical_weights(11, h, L, V)
    ads = cfg.make_adapters(h, L)
    prompts = synthetic_prompts(cfg, V)
    for k in (-1, 0, 1):
        ref = Stage(h, nh, L, V, 0, L, max_batch=1, max_ctx=32,
                    host_weights=w if k < 0 else lora.merged_weights(w, ads[k], h, V))
        for i in range(k + 1, 6, 3):
            got = res["samples"][i]
            if k < 0:
                assert got == base["samples"][i]
            ref.reset()
            fed = [prompts[i]] + [[t] for t in got[:-1]]
            lgs, past = [], 0
            for f in fed:
                lgs.append(ref.forward_host(np.array(f, np.int32), 1, len(f), past_len=past, want_logits=True)[1][0])
                past += len(f)
            lgs = np.stack(lgs)
            assert_ids_match(got, lgs.argmax(-1), lgs, f"sample {i} on adapter {k}")
    assert any(res["samples"][i] != base["samples"][i] for i in (1, 2, 4, 5)), "no adapter changed any token"
