"""The two LoRA kernels (lora.hip) against float64, element by element, through Stage.adapter_delta.

Reference, with A, B and x rounded to bf16 first: ref[m][n] = scale * sum_j B[n][j] * sum_k A[j][k] * x[m][k].
Bound: fp32 accumulation in any order (K terms in the first product, r in the second, 2 ulp-halves each) plus the
hi + lo bf16 split of scale * u (relative 2^-16), against the sum of the absolute terms:
  |delta - ref| <= ((2K + 2r) * 2^-24 + 2^-16) * scale * sum_j |B[n][j]| * sum_k |A[j][k]| * |x[m][k]|
The caller's buffer holds a non-zero pattern p, so what is read back is fp32(p + delta): one more fp32 rounding of the
sum, 2^-24 * |p + ref|, is added to the bound.

Shapes: a target's (K, N) is fixed by the stage's hidden size, so (256, 768) is h = 256 query_key_value, (1024, 256) is
h = 256 dense_4h_to_h (two K slices), and the K = 4096 case (eight K slices, the ordered sum of the partials) is h = 1024
dense_4h_to_h, (4096, 1024): no target of any stage is (4096, 256).
"""
import functools

import numpy as np
import pytest
import torch

from distributed_inference_demo_amd import lora
from distributed_inference_demo_amd.stage import Stage
from test_gpu_parity import record_error

pytestmark = pytest.mark.gpu
GUARD = 16  # rows behind the last token: a store of a dead token of the last tile would land here


@functools.lru_cache(maxsize=None)
def stage(h):
    return Stage(h, 8, 1, 256, 0, 1, dtype="bf16", max_batch=3, max_ctx=32, max_tokens=64)


RANK_CASES = [(r, 256, "qkv", b, s) for r in (1, 16, 33, 64) for b, s in ((3, 1), (1, 15), (1, 16), (2, 17))]


@pytest.mark.parametrize("rank,h,target,batch,seq", RANK_CASES + [(64, 1024, "fc2", 2, 17), (16, 256, "fc2", 2, 17)])
def test_adapter_delta_matches_float64(rank, h, target, batch, seq):
    st = stage(h)
    K, N = lora.target_shape(target, h)
    M = batch * seq
    ad = lora.synthetic(100 + rank, rank, [target], h, 1)
    aid = st.load_adapter(ad)
    try:
        g = torch.Generator().manual_seed(rank * 1000 + M)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
        idx = np.arange((M + GUARD) * N, dtype=np.int64).reshape(M + GUARD, N)
        p = (((idx % 13) - 6) / 8.0 + 0.0625).astype(np.float32)  # never zero
        out = torch.from_numpy(p).cuda()
        st.adapter_delta(aid, 0, lora.TARGET_BITS[target], x, out, batch, seq)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    finally:
        st.unload_adapter(aid)
    A = lora.bf16_round(ad.a[target][0]).astype(np.float64)
    B = lora.bf16_round(ad.b[target][0]).astype(np.float64)
    xs = x.float().cpu().numpy().astype(np.float64)
    ref = p[:M].astype(np.float64) + ad.scale * (xs @ A.T) @ B.T
    mag = ad.scale * (np.abs(xs) @ np.abs(A).T) @ np.abs(B).T
    bound = ((2 * K + 2 * rank) * 2.0 ** -24 + 2.0 ** -16) * mag + 2.0 ** -24 * np.abs(ref)
    err = np.abs(got[:M].astype(np.float64) - ref)
    frac = record_error(f"lora delta r={rank} K={K} N={N} B={batch} S={seq}", err / bound, np.zeros_like(err), 1.0,
                        "lora kernels, fraction of the bound")
    print(f"worst fraction of the bound: {frac:.4f}")
    assert np.abs(got[:M] - p[:M]).min() > 0, "an element of a live token was not updated"
    assert frac <= 1.0, f"|got - ref| reaches {frac:.3f} of the bound"
    assert np.array_equal(got[M:].view(np.uint32), p[M:].view(np.uint32)), "a token past seq was stored"
