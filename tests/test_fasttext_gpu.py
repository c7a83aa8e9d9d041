"""GPU: FastText vectors of the OCR tokens from their text (csrc/fasttext.hip) -- the kernel against the host twin bit for bit
(order-sensitive data, clamps, guard band, both widths), its bf16 / normalised forms against l2norm_pack of the twin's rows, and its limits.
The twin is the contract: nothing here compares with the fastText library."""
import functools

import numpy as np
import pytest
import torch

from tests.test_fasttext_cpu import manual_vector, toy_index, toy_model

pytestmark = pytest.mark.gpu

B, NO, LW = 3, 5, 12
TOKENS = (("the", "thex", "</s>", "", "q"), ("a  b", "é€😀", "日本語 café", "abcdefghijkl", "The"), ("stop the", "within", "w3 ", "naïve", "😀"))


@functools.lru_cache(maxsize=None)
def gpu_index(bucket=64, minn=3, maxn=6, dim=300):
    from sam_textvqa_amd import fasttext as FT
    return FT.index_to(toy_index(bucket, minn, maxn, dim), "cuda")


def packed_tokens(ld_text=LW + 3, seed=1):
    """TOKENS packed at Lw = 12 inside rows of ld_text columns whose tail (and every slot's columns behind its token) holds random letters: what lies
    behind a length must not matter, and does when a length is over-long"""
    from sam_textvqa_amd import phoc as P
    assert len(TOKENS[1][3]) == LW
    p = P.pack_ocr_text([list(t) for t in TOKENS], max_ocr_tokens=NO, max_chars=LW)
    g = torch.Generator().manual_seed(seed)
    wide = torch.randint(97, 123, (B, NO, ld_text), generator=g, dtype=torch.int32)
    keep = torch.arange(ld_text)[None, None, :] < p["ocr_text_len"][..., None]
    wide[..., :LW] = torch.where(keep[..., :LW], p["ocr_text"], wide[..., :LW])
    return wide, p["ocr_text_len"].clone()


def launch(wide, ln, counts, index, dst, col0, normalize=False):
    """the C entry point itself, on the first LW columns of the wider text rows"""
    from sam_textvqa_amd import _capi as capi
    text, ln = wide.cuda(), ln.cuda()
    c = None if counts is None else counts.cuda()
    cp = index["cp"]
    capi.call("sam_fasttext_from_text", capi.ptr(text), text.shape[2], capi.ptr(ln), capi.ptr(c), B, NO, LW, capi.ptr(index["matrix"]), index["matrix"].stride(0),
              capi.ptr(cp), cp.stride(0), capi.ptr(index["len"]), capi.ptr(index["slots"]), cp.shape[1], index["slots"].numel(), index["minn"], index["maxn"],
              index["bucket"], index["nwords"], index["eos"], index["dim"], capi.ptr(dst), dst.stride(0), col0, int(dst.dtype == torch.float32), int(normalize), 1e-12,
              capi.stream_handle())
    torch.cuda.synchronize()
    return dst


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("bucket,minn,maxn,dim", [(64, 3, 6, 300), (64, 1, 1, 300), (64, 2, 8, 300), (1, 3, 6, 300), (1, 1, 1, 300), (1, 2, 8, 300), (64, 3, 6, 8)])
def test_kernel_equals_the_host_twin_bit_for_bit(bucket, minn, maxn, dim, monkeypatch):
    from sam_textvqa_amd import fasttext as FT
    cpu, index = toy_index(bucket, minn, maxn, dim), gpu_index(bucket, minn, maxn, dim)
    wide, ln = packed_tokens()
    col0, ld = 8, dim + 20
    runs = [(ln, None), (ln, torch.tensor([0, NO, NO + 3], dtype=torch.int32)), (ln, torch.tensor([2, -1, 4], dtype=torch.int32))]
    odd = ln.clone()                                                   # lengths over Lw and below 0: clamped, never trusted
    odd[0, 0], odd[0, 1], odd[1, 1], odd[2, 2], odd[2, 4] = LW + 1, 1 << 30, -1, -(1 << 31), 99
    runs.append((odd, None))
    for lens, counts in runs:
        want = torch.from_numpy(FT.vectors_host_text(wide[..., :LW], lens, cpu, counts)).view(B * NO, dim)
        dst = torch.full((B * NO, ld), -7.0, dtype=torch.float32, device="cuda")
        out = launch(wide, lens, counts, index, dst, col0).cpu()
        assert (out[:, :col0] == -7.0).all() and (out[:, col0 + dim:] == -7.0).all()                      # the guard band on both sides
        got = out[:, col0: col0 + dim]
        bad = [(r // NO, r % NO) for r in range(B * NO) if not torch.equal(bits(got[r]), bits(want[r]))]
        assert not bad, (bad, counts)
        if counts is not None:
            for b, c in enumerate(counts.clamp(0, NO).tolist()):
                assert not got[b * NO + c: (b + 1) * NO].any()
        else:
            assert got.abs().sum(1).gt(0).sum() >= (10 if lens is ln else 8)
    # the same text through the package's own call (contiguous rows), as the model makes it: the torch op, then the ctypes route of the wrapper
    for route in ("1", "0"):
        monkeypatch.setenv("SAM_COARSE_OPS", route)
        got = FT.fasttext_from_text(wide[..., :LW].contiguous().cuda(), ln.cuda(), index)
        assert torch.equal(bits(got.cpu()), bits(torch.from_numpy(FT.vectors_host_text(wide[..., :LW], ln, cpu)))), route
    if bucket > 1:
        # bit-equality says something about ORDER only if order matters on this data: summed in sorted id order, the twin's own rows come out different
        differs = 0
        for w in ("within", "thex", "naïve", "abcdefghijkl"):
            ids = FT.word_ids(w, cpu)
            differs += int(sorted(ids) != ids and not np.array_equal(manual_vector(ids, toy_model(bucket, minn, maxn, dim)["matrix"]),
                                                                     manual_vector(sorted(ids), toy_model(bucket, minn, maxn, dim)["matrix"])))
        assert differs >= 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("normalize", [False, True])
def test_bf16_and_normalised_rows_equal_l2norm_pack_of_the_twin(dtype, normalize):
    from sam_textvqa_amd import fasttext as FT, ops
    cpu, index = toy_index(), gpu_index()
    wide, ln = packed_tokens()
    counts = torch.tensor([NO, NO, 3], dtype=torch.int32)
    host = torch.from_numpy(FT.vectors_host_text(wide[..., :LW], ln, cpu, counts)).view(B * NO, 300)
    col0, ld = 304, 1000
    if dtype == torch.bfloat16:
        ref = torch.zeros((B * NO, ld), dtype=dtype, device="cuda")
        ops.l2norm_pack(host.cuda(), ref, col0, normalize)
    else:                        # the fp32 destination of the same row body: the expansion of the twin's rows, every slot valid
        ref = torch.zeros((B * NO, ld), dtype=dtype, device="cuda")
        ops.ragged_expand(torch.full((B,), NO, dtype=torch.int32, device="cuda"), NO, [(host.cuda(), ref, col0, normalize, 0)])
    want = ref[:, col0: col0 + 300].cpu()
    if normalize:
        assert ((want.float().norm(dim=1) - 1).abs() < 1e-2)[host.abs().sum(1) > 0].all()
    dst = torch.full((B * NO, ld), -7.0, dtype=dtype, device="cuda")
    out = launch(wide, ln, counts, index, dst, col0, normalize).cpu()
    assert (out[:, :col0] == -7.0).all() and (out[:, col0 + 300:] == -7.0).all()
    assert torch.equal(bits(out[:, col0: col0 + 300]), bits(want))
    assert not out[[3, 13, 14], col0: col0 + 300].any() and out[0, col0: col0 + 300].any()                # "", and the slots behind the count


def test_limits_return_unsupported_without_a_launch():
    from sam_textvqa_amd import _capi as capi
    index = gpu_index()
    wide, ln = packed_tokens(ld_text=80)
    text, ln = wide.cuda(), ln.cuda()
    dst = torch.full((B * NO, 600), -7.0, dtype=torch.float32, device="cuda")

    def rc(Lw=LW, dim=300, minn=3, maxn=6, col0=0, ld_dst=600):
        cp = index["cp"]
        return capi.lib().sam_fasttext_from_text(capi.ptr(text), text.shape[2], capi.ptr(ln), None, B, NO, Lw, capi.ptr(index["matrix"]), index["matrix"].stride(0),
                                                 capi.ptr(cp), cp.stride(0), capi.ptr(index["len"]), capi.ptr(index["slots"]), cp.shape[1], index["slots"].numel(),
                                                 minn, maxn, 64, 40, 2, dim, capi.ptr(dst), ld_dst, col0, 1, 0, 1e-12, capi.stream_handle())
    for kw in (dict(Lw=65), dict(dim=298), dict(dim=516, ld_dst=600), dict(maxn=9), dict(col0=2), dict(ld_dst=598)):
        assert rc(**kw) == capi.CONSTANTS["SAM_ERR_UNSUPPORTED"] == -2, kw
    assert rc(minn=7) == capi.CONSTANTS["SAM_ERR_ARG"]
    torch.cuda.synchronize()
    assert (dst == -7.0).all()                                         # nothing was launched
    assert rc() == 0
    torch.cuda.synchronize()
    assert (dst[:, :300] != -7.0).all() and (dst[:, 300:] == -7.0).all()
