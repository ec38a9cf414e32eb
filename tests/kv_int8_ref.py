"""The int8 KV cache rule (include/bloomstage.h BS_FLAG_INT8_KV) restated in numpy fp32, for the tests.

Per (position, head) vector x of hd values (bf16-exact, held as fp32): amax = max|x|, scale = amax / 127 (fp32 IEEE
division; 1 for an all-zero vector), q = clamp(rint(x / scale), -127, 127) (round half to even), and the dequantised
value is float32(q) * scale (one fp32 product)."""
import numpy as np


def quantize(x):
    """x [..., hd] -> (codes int8 [..., hd], scales fp32 [...])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=-1, keepdims=True).astype(np.float32)
    scale = np.where(amax > 0, amax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    q = np.clip(np.rint(x / scale), -127.0, 127.0).astype(np.int8)
    return q, scale[..., 0]


def dequantize(q, scale):
    return (q.astype(np.float32) * np.asarray(scale, np.float32)[..., None]).astype(np.float32)


def roundtrip(x):
    """What bs_read_kv returns for a vector the cache took as x."""
    return dequantize(*quantize(x))


def to_bf16(x):
    """fp32 -> nearest-even bf16, returned as fp32 (what a bf16 staging copy of dequantised values holds)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def kv_bytes(n_layer, max_batch, n_head, max_ctx, head_dim):
    """bs_stage_info's kv_bytes of an int8-KV stage."""
    return n_layer * 2 * max_batch * n_head * max_ctx * (head_dim + 4)
