"""serve --prefix-attention: config validation (no GPU)."""
import pytest

from distributed_inference_demo_amd.serve import RunConfig


@pytest.mark.parametrize("kw", [{}, {"shared_prefix": 8, "prefix_fork": False}, {"shared_prefix": 8, "kv": "int8"},
                                {"num_beams": 4, "kv": "int8"}, {"num_beams": 4, "dtype": "fp32"}])
def test_prefix_attention_is_rejected(kw):
    with pytest.raises(ValueError, match="prefix_attention"):
        RunConfig(prefix_attention=True, prompt_len=16, **kw)


@pytest.mark.parametrize("kw", [{"shared_prefix": 8}, {"num_beams": 4}])
def test_prefix_attention_is_accepted(kw):
    assert RunConfig(prefix_attention=True, prompt_len=16, **kw).prefix_attention
    assert not RunConfig(prompt_len=16, **kw).prefix_attention
