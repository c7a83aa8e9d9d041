"""CPU half of tests/test_attention_infer_gpu.py: the per-row bound it puts on sam_attn_probs is the arithmetic's, not a measurement of the kernel.
A plain fp32 evaluation of softmax(scale * q k^T over the allowed keys) on the GPU test's own inputs meets the same assertions against fp64."""
import numpy as np
import pytest
import torch

from tests.test_attention_infer_gpu import B, INV_KEEP, LENS, P_DROP, make_inputs, reference_probs, softmax_probs
from tests.util import assert_close_bf16_sliced


@pytest.mark.parametrize("per_head", [False, True], ids=["shared", "per_head"])
def test_plain_fp32_softmax_meets_the_per_row_probability_bound(per_head):
    """|P_fp32 - P_fp64| <= 1e-3 * max of the query row, exact zeros at masked keys and in rows with no allowed key, live rows summing to 1 within 1e-3:
    what tests/test_attention_infer_gpu.py asserts of sam_attn_probs, at every length it uses"""
    worst = 0.0
    for n in LENS:
        pr = make_inputs(n, per_head)
        ref = reference_probs(n, per_head)
        p32 = softmax_probs(pr["qkv"], pr["allow"], B, dtype=torch.float32)
        worst = max(worst, assert_close_bf16_sliced(p32, ref, slice_dims=(-1,), ulps=0, name="fp32 softmax N=%d" % n))
        allow = pr["allow"].expand_as(ref)
        alive = allow.any(-1)
        assert (p32[~allow] == 0).all() and (ref[~allow] == 0).all() and (p32[~alive] == 0).all()
        if per_head:
            assert not alive[pr["dead"]]
        assert (p32.double().sum(-1)[alive] - 1.0).abs().max().item() <= 1e-3
    print("fp32 softmax against fp64: %.2e of the row maximum at worst (bound 1e-3)" % worst)


def test_fp32_inv_keep_leaves_room_for_the_one_ulp_dropout_bound():
    """the GPU test's "P_drop = P * inv_keep within one fp32 ulp" rests on the library's fp32 inv_keep = 1 / (1 - thr16 / 65536) lying under half an fp32
    ulp (2^-24 relative, at the bottom of a binade) from the exact quotient, so that the multiply's own half ulp keeps the product within one"""
    thr16 = round(P_DROP * 65536)
    f32 = np.float32(1.0) / (np.float32(1.0) - np.float32(thr16) / np.float32(65536.0))
    assert abs(float(f32) - INV_KEEP) / INV_KEEP < 0.5 * 2.0 ** -24
