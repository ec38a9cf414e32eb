"""MXFP4 KV cache, the parts that need no GPU: RunConfig(kv="mxfp4") and the serve options that exclude it, the
build_rank refusals (raised before any stage is built) and the byte model."""
import pytest
import torch

from distributed_inference_demo_amd import config, pipeline
from distributed_inference_demo_amd.serve import RunConfig
from distributed_inference_demo_amd.stage import BS_FLAG_MXFP4_KV


@pytest.mark.parametrize("kw", [dict(speculate=3), dict(sample_speculate=3, sample=True), dict(ragged_admission=True),
                                dict(speculate_tree=4), dict(num_beams=2, prefix_attention=True)],
                         ids=lambda kw: next(iter(kw)))
def test_serve_options_that_exclude_int8_exclude_mxfp4(kw):
    RunConfig(kv="bf16", **kw)
    for kv in ("int8", "mxfp4"):
        with pytest.raises(ValueError, match="kv"):
            RunConfig(kv=kv, **kw)


def test_build_rank_refusals(monkeypatch):
    tiny, cpu = config.get("tiny"), torch.device("cpu")
    with pytest.raises(ValueError, match="bf16"):
        pipeline.build_rank(tiny, 0, 1, cpu, dtype="fp32", kv_mxfp4=True)
    with pytest.raises(ValueError, match="executor_factory"):
        pipeline.build_rank(tiny, 0, 1, cpu, dtype="bf16", kv_mxfp4=True, executor_factory=lambda *a, **k: 1 / 0)
    with pytest.raises(ValueError, match="one"):
        pipeline.build_rank(tiny, 0, 1, cpu, dtype="bf16", kv_mxfp4=True, kv_int8=True)
    monkeypatch.setattr(pipeline, "stage_ranges", lambda world, n_layer: [(0, 0)] * world)
    with pytest.raises(ValueError, match="vocabulary slice"):
        pipeline.build_rank(tiny, 0, 1, cpu, dtype="bf16", kv_mxfp4=True)


def test_flag_run_config_and_kv_bytes_per_element():
    assert BS_FLAG_MXFP4_KV == 16 and RunConfig(kv="mxfp4").kv == "mxfp4"
    for name in ("bloom-560m", "bloom-7b1"):  # hd 64 and 128
        m = config.get(name)
        assert config.kv_bytes_per_element(m, kv_mxfp4=True) == 0.5 + 1 / 32
        assert config.kv_bytes_per_element(m, True) == 1 + 4 / m.head_dim and config.kv_bytes_per_element(m) == 2
