"""CPU side of the weight-only MXFP4 variant (BS_FLAG_MXFP4_WEIGHTS): the rule on hand-made blocks, exactness of the
dequantised values in bf16, the model names and byte model, and the C-ABI's argument checks (no GPU needed)."""
import numpy as np
import pytest

import mxfp4_np
from distributed_inference_demo_amd import config
from distributed_inference_demo_amd.stage import BloomStageError, Stage
from oracle import gen_np


def _block(values, fill=0.0):
    b = np.full(32, fill, np.float32)
    b[:len(values)] = values
    return b


def test_ties_go_to_the_even_code():
    """amax = 6 gives X = 1 (floor(log2 6) - 2 = 0): every midpoint between two grid values, both signs."""
    vals = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for sign in (1.0, -1.0):
        w = _block([sign * v for v in vals])
        idx, neg, E = mxfp4_np.quantize(w)
        assert E.tolist() == [127]
        got = mxfp4_np.dequantize(idx, neg, E)
        assert np.array_equal(got[:8] + 0.0, np.array(want, np.float32) * sign + 0.0)
        assert not got[8:].any()
    # just off the midpoints: nearest wins
    w = _block([6.0, 0.2578125, 0.74609375, 1.2578125, 1.7421875, 2.515625, 3.484375, 5.03125])
    assert mxfp4_np.roundtrip(w)[:8].tolist() == [6.0, 0.5, 0.5, 1.5, 1.5, 3.0, 3.0, 6.0]


def test_saturation_zero_and_tiny_blocks():
    got = mxfp4_np.roundtrip(_block([7.0, 7.5, -7.5, 4.0]))  # amax 7.5: X = 1, above 6 saturates
    assert got[:4].tolist() == [6.0, 6.0, -6.0, 4.0]
    idx, neg, E = mxfp4_np.quantize(np.zeros(32, np.float32))
    assert E.tolist() == [127] and not idx.any()
    tiny = _block([2.0 ** -101, -(2.0 ** -110)])  # amax < 2^-100: E = 127, all codes 0
    idx, neg, E = mxfp4_np.quantize(tiny)
    assert E.tolist() == [127] and not idx.any()
    assert not mxfp4_np.dequantize(idx, neg, E).any()
    edge = _block([2.0 ** -100])  # the smallest scaled block: E = 27 - 2, value = 4 * 2^-102
    idx, neg, E = mxfp4_np.quantize(edge)
    assert E.tolist() == [25] and idx[0] == 6
    assert mxfp4_np.dequantize(idx, neg, E)[0] == np.float32(2.0 ** -100)


def test_scale_is_floor_log2_amax_minus_emax_and_blocks_are_independent():
    w = np.concatenate([_block([0.02, -0.013]), _block([3.0, -48.0, 1.0]), _block([2.0 ** -20])])
    w = gen_np.bf16_round(w)
    idx, neg, E = mxfp4_np.quantize(w.reshape(1, 96))
    amax = np.abs(w.reshape(3, 32)).max(axis=1)
    assert E[0].tolist() == [int(np.floor(np.log2(a))) - 2 + 127 for a in amax]
    got = mxfp4_np.dequantize(idx, neg, E).reshape(3, 32)
    assert got[1, :3].tolist() == [4.0, -48.0, 0.0]  # X = 8: 3 / 8 = 0.375 -> 0.5, 1 / 8 -> 0
    assert np.signbit(got[0, 1]) and got[2, 0] == np.float32(2.0 ** -20)


def test_dequantised_values_are_exact_in_bf16_and_close():
    w = gen_np.bf16_round(gen_np.tensor(3, 0, 8, (64, 256)))  # layer 0 fc1 rows
    w[5] = 0.0
    idx, neg, E = mxfp4_np.quantize(w)
    got = mxfp4_np.dequantize(idx, neg, E)
    assert np.array_equal(gen_np.bf16_round(got).view(np.uint32), got.view(np.uint32))
    assert not got[5].any() and (E[5] == 127).all()
    X = np.repeat(np.exp2(E.astype(np.float64) - 127.0), 32, axis=-1)
    r = np.abs(w) / X
    assert r.max() < 8.0 and (r.reshape(64, 8, 32).max(axis=-1)[np.arange(64) != 5] >= 4.0).all()
    # half the widest grid step below 6 (|W| / X in (4, 6): step 2), and at most 2 where 6 saturates
    err = np.abs(got.astype(np.float64) - w) / X
    assert (err[r <= 6.0] <= 1.0).all() and (err <= 2.0).all()
    rel = np.linalg.norm(got - w) / np.linalg.norm(w)
    assert 0.05 < rel < 0.2  # round-to-nearest 4-bit weights are lossy: opt-in


def test_mxfp4_model_names():
    a, b = config.get("bloom-7b1"), config.get("bloom-7b1-mxfp4")
    assert (b.name, b.mxfp4_weights, b.int8_weights) == ("bloom-7b1-mxfp4", True, False)
    assert (b.hidden, b.n_layer, b.n_head, b.vocab) == (a.hidden, a.n_layer, a.n_head, a.vocab) == (4096, 30, 32, 250880)
    assert not a.mxfp4_weights and not config.get("bloom-7b1-int8").mxfp4_weights
    c = config.get("bloom560m-mxfp4")
    assert (c.name, c.mxfp4_weights, c.hidden) == ("bloom-560m-mxfp4", True, 1024)


def test_decode_step_bytes_takes_fractional_weight_bytes():
    m = config.get("bloom-7b1")
    assert config.MXFP4_BYTES_PER_WEIGHT == mxfp4_np.BYTES_PER_WEIGHT == 0.53125
    plain = config.decode_step_bytes(m, 30, 1, 128, False, False)
    assert plain == config.decode_step_bytes(m, 30, 1, 128, False, False, matrix_bytes=2)
    mx = config.decode_step_bytes(m, 30, 1, 128, False, False, matrix_bytes=config.MXFP4_BYTES_PER_WEIGHT)
    assert plain - mx == 30 * 12 * 4096 * 4096 * (2 - 0.53125)
    half = config.decode_step_bytes(m, 30, 1, 128, False, False, w_bytes=0.53125)  # a fractional w_bytes as well
    assert isinstance(half, float) and half < mx
    # bloom-7b1's 30 blocks: 12.1 GB in bf16, 3.2 GB in MXFP4
    assert round(30 * 12 * 4096 ** 2 * 0.53125 / 1e9, 1) == 3.2


def test_mxfp4_flag_rejected_on_fp32_stage():
    with pytest.raises(BloomStageError, match="error -5.*BFLOAT16"):
        Stage(64, 4, 1, 256, 0, 1, dtype="fp32", max_ctx=4, mxfp4_weights=True)


def test_mxfp4_flag_rejected_with_int8_weights():
    with pytest.raises(BloomStageError, match="error -1.*INT8_WEIGHTS"):
        Stage(64, 4, 1, 256, 0, 1, dtype="bf16", max_ctx=4, mxfp4_weights=True, int8_weights=True)
