"""serve with ragged_admission: every admission wave is one bs_forward_ragged pass; the tokens are the per-sample
checker's.  Plus the config combinations the option refuses (no GPU)."""
import numpy as np
import pytest

from distributed_inference_demo_amd.config import BloomDims
from distributed_inference_demo_amd.serve import RunConfig, run_rank, synthetic_prompts
from oracle.oracle import OracleStage


@pytest.mark.gpu
def test_ragged_admission_matches_the_checker_per_sample():
    """7 samples of 2..11 prompt tokens, 3 rows in flight: waves of 3, 3 and 1 samples, three ragged passes."""
    import torch
    model = BloomDims("tinygpu", 256, 2, 4, vocab=1024)
    cfg = RunConfig(model=model, num_sample=7, max_length=6, core_pool_size=3, prompt_len=11, dtype="bf16", seed=11,
                    ragged_admission=True)
    prompts = [p[:n] for p, n in zip(synthetic_prompts(cfg, model.vocab), (2, 11, 5, 9, 3, 1, 7))]
    res = run_rank(cfg, 0, 1, torch.device("cuda", 0), prompts=prompts)
    assert res["ragged_admission"] and res["prefill_passes"] == 3 and res["prefill_tokens"] == sum(map(len, prompts))
    for i, (p, got) in enumerate(zip(prompts, res["samples"])):
        o = OracleStage(256, 4, 2, 1024, 0, 2, bf16=True, max_batch=1, max_ctx=32, seed=11)
        x, past = np.array(p, np.int32), 0
        for k in range(cfg.max_length):
            tok, lg = o.forward(x.reshape(1, -1), 1, len(x), past_len=past, want_logits=True)
            past += len(x)
            if got[k] != int(tok[0]):  # only a near-tie of the checker may differ; the sample then goes its own way
                top2 = np.sort(lg[0])[-2:]
                assert top2[1] - top2[0] < 2e-2, f"sample {i} token {k}: {got[k]} != {int(tok[0])}, checker top-2 {top2}"
                break
            x = tok
        o.close()


@pytest.mark.parametrize("kw", [
    dict(sample=True), dict(repetition_penalty=1.3), dict(bad_token=(3,)), dict(choice=("1,2",), eos_id=3),
    dict(guide_file="g.json"), dict(shared_prefix=4), dict(speculate=2), dict(sample=True, sample_speculate=2),
    dict(num_beams=2), dict(kv="int8"), dict(prefill=False)])
def test_ragged_admission_refuses_what_it_cannot_serve(kw):
    RunConfig(ragged_admission=True)
    with pytest.raises(ValueError, match="ragged_admission"):
        RunConfig(ragged_admission=True, **kw)


@pytest.mark.parametrize("world,factory", [(2, None), (1, lambda *a, **k: None)])
def test_ragged_admission_is_one_rank_with_the_hip_stage(world, factory):
    import torch
    with pytest.raises(ValueError, match="ragged_admission"):
        run_rank(RunConfig(ragged_admission=True), 0, world, torch.device("cpu"), executor_factory=factory)
