"""Numpy restatement of the BS_FLAG_MXFP4_WEIGHTS rule (include/bloomstage.h; OCP Microscaling Formats v1.0, MXFP4):
blocks of 32 consecutive values along the last axis share one E8M0 scale, each value becomes a 4-bit E2M1 code.

Written as "the nearest grid point, the even code on a tie" over float64 distances -- not as the comparison ladder the
device kernel uses -- so the two are independent statements of one rule.
"""
import numpy as np

BLOCK = 32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # E2M1 magnitudes by 3-bit index
EMAX = 2                                                   # exponent of the largest E2M1 binade (4 <= 6 < 8)
BYTES_PER_WEIGHT = 0.5 + 1.0 / BLOCK


def quantize(w):
    """w: float32 array of bf16-representable values, last axis a multiple of 32.
    Returns (index uint8 like w, negative bool like w, E uint8 [..., K / 32])."""
    w = np.ascontiguousarray(w, np.float32)
    blk = w.reshape(w.shape[:-1] + (w.shape[-1] // BLOCK, BLOCK))
    amax = np.abs(blk).max(axis=-1)
    small = amax < 2.0 ** -100
    field = (amax.view(np.uint32) >> 23) & 0xFF  # biased exponent: floor(log2 amax) + 127
    E = np.where(small, 127, field.astype(np.int64) - EMAX).astype(np.int64)
    r = np.abs(blk).astype(np.float64) * np.exp2(127.0 - E)[..., None]  # |w| / X, exact
    r = np.where(small[..., None], 0.0, r)
    d = np.abs(r[..., None] - GRID)               # [..., 32, 8]; above 6 the nearest point is 6 (saturation)
    best = d == d.min(axis=-1, keepdims=True)
    codes = np.arange(8)
    even = np.where(best & (codes % 2 == 0), codes, 99).min(axis=-1)
    idx = np.where(even < 99, even, np.argmax(best, axis=-1)).astype(np.uint8)
    return idx.reshape(w.shape), np.signbit(w), E.astype(np.uint8)


def dequantize(idx, neg, E):
    """+-GRID[idx] * 2^(E - 127) as float32 (exact: at most 2 significant bits times a power of two)."""
    shape = idx.shape
    mag = GRID[idx.reshape(shape[:-1] + (shape[-1] // BLOCK, BLOCK))] * np.exp2(E.astype(np.float64) - 127.0)[..., None]
    out = np.where(neg.reshape(mag.shape), -mag, mag).astype(np.float32)
    return out.reshape(shape)


def roundtrip(w):
    """The values an MXFP4 stage computes with in place of w."""
    return dequantize(*quantize(w))
