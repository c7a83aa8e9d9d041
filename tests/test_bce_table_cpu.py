"""CPU (no GPU needed): the host side of the answer-table loss path -- answers.bce_from_table_torch (the torch twin of
sam_bce_loss_table) against the oracle's M4CDecodingBCEWithMaskLoss + autograd on the dense targets of every reference-generated draw,
answers.decode_predictions on hand-written cases, and the new entry point's presence in the library at an unchanged ABI version."""
import numpy as np
import pytest
import torch

from oracle import sa_m4c_oracle as O
from sam_textvqa_amd import answers as A
from tests.test_answers_cpu import case_tables, golden, records_by_round


def test_twin_matches_the_oracle_loss_on_every_golden_draw():
    """loss within 1e-6 relative (the bound the project uses between two routes of this loss), gradients within 1e-6 of their max, pred == argmax"""
    meta, g = golden()
    _, _, table = case_tables(meta)
    W, L = meta["W"], meta["max_copy_steps"]
    B = table["meta"].shape[0]
    No = meta["max_ocr_tokens"]
    V = W - No
    gen = torch.Generator().manual_seed(11)
    rounds = 0
    for choice, _ in records_by_round(g):
        fixed = torch.randn(B, L, V, generator=gen) * 3.0
        ocr = torch.randn(B, L, No, generator=gen) * 3.0
        dense = A.sample_answers_torch(table, torch.from_numpy(choice))
        fx, oc = fixed.clone().requires_grad_(True), ocr.clone().requires_grad_(True)
        want = O.m4c_decoding_bce_with_mask_loss(torch.cat([fx, oc], -1), dense["targets"], dense["train_loss_mask"])
        want.backward()
        loss, d_fixed, d_ocr, pred = A.bce_from_table_torch(fixed, ocr, table, dense["answer_choice"], dense["train_loss_mask"])
        print("round %d: loss %.9g oracle %.9g" % (rounds, loss.item(), want.item()))
        assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()), (loss.item(), want.item())
        gmax = max(fx.grad.abs().max().item(), oc.grad.abs().max().item())
        assert (d_fixed - fx.grad.reshape(B * L, V)).abs().max().item() <= 1e-6 * gmax
        assert (d_ocr - oc.grad.reshape(B * L, No)).abs().max().item() <= 1e-6 * gmax
        assert torch.equal(pred, torch.argmax(torch.cat([fixed, ocr], -1), -1).reshape(-1))
        rounds += 1
    assert rounds >= 2


def test_twin_scales_like_the_kernel_under_grad_scale_and_global_count():
    meta, g = golden()
    _, _, table = case_tables(meta)
    W, L, No = meta["W"], meta["max_copy_steps"], meta["max_ocr_tokens"]
    B = table["meta"].shape[0]
    choice = records_by_round(g)[0][0]
    dense = A.sample_answers_torch(table, torch.from_numpy(choice))
    gen = torch.Generator().manual_seed(5)
    fixed, ocr = torch.randn(B * L, W - No, generator=gen), torch.randn(B * L, No, generator=gen)
    l0, f0, o0, _ = A.bce_from_table_torch(fixed, ocr, table, choice, dense["train_loss_mask"])
    n = dense["train_loss_mask"].sum().item()
    l1, f1, o1, _ = A.bce_from_table_torch(fixed, ocr, table, choice, dense["train_loss_mask"], grad_scale=4.0, global_count=torch.tensor([2.0 * n]))
    assert abs(l1.item() - 0.5 * l0.item()) <= 1e-6 * abs(l0.item())
    assert torch.allclose(f1, 2.0 * f0, rtol=1e-6, atol=0) and torch.allclose(o1, 2.0 * o0, rtol=1e-6, atol=0)
    # a masked row contributes nothing and receives no gradient
    masked = dense["train_loss_mask"].reshape(-1) == 0
    assert masked.any() and not f0[masked].any() and not o0[masked].any()


VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "coca", "cola", "'s", "joe", "stop"]      # EOS = 2, len 9: OCR slot j is index 9 + j


def test_decode_predictions_hand_written_cases():
    voc = A.AnswerVocab(VOCAB)
    toks = [["pepsi", "max"], ["a"], ["x", "y", "z"], [], ["bar"]]
    pred = torch.tensor([[2, 4, 5, 2, 0, 0],            # EOS first: the empty answer
                         [4, 5, 8, 4, 5, 8],            # no EOS within L: all six words
                         [9, 11, 4, 10, 2, 7],          # OCR copies mixed with vocabulary words
                         [7, 6, 8, 2, 2, 2],            # the 's join
                         [9, 6, 2, 9, 9, 9]])           # ... also behind an OCR word
    out = A.decode_predictions(pred, voc, toks)
    assert out[0] == ("", [], ["vocab+eos"])
    assert out[1] == ("coca cola stop coca cola stop", ["coca", "cola", "stop", "coca", "cola", "stop"], ["vocab"] * 6)
    assert out[2] == ("x z coca y", ["x", "z", "coca", "y"], ["ocr", "ocr", "vocab", "ocr", "vocab+eos"])
    assert out[3] == ("joe's stop", ["joe", "'s", "stop"], ["vocab", "vocab", "vocab", "vocab+eos"])
    assert out[4] == ("bar's", ["bar", "'s"], ["ocr", "vocab", "vocab+eos"])
    # plain lists and an explicit EOS index work the same
    assert A.decode_predictions([[4, 8, 5]], VOCAB, [[]], eos_idx=8) == [("coca", ["coca"], ["vocab", "vocab+eos"])]


def test_decode_predictions_raises_on_an_ocr_index_beyond_the_token_list():
    voc = A.AnswerVocab(VOCAB)
    with pytest.raises(IndexError, match="sample 1"):
        A.decode_predictions(torch.tensor([[9, 2], [10, 2]]), voc, [["a"], ["b"]])
    with pytest.raises(ValueError):
        A.decode_predictions(torch.tensor([[2]]), voc, [["a"], ["b"]])
    # an out-of-range slot BEHIND the EOS is never walked
    assert A.decode_predictions(torch.tensor([[4, 2, 30]]), voc, [[]])[0][0] == "coca"


def test_library_exports_the_table_loss_and_keeps_the_abi_version():
    from sam_textvqa_amd import _capi as capi
    assert "sam_bce_loss_table" in capi.SIGNATURES
    l = capi.lib()
    assert hasattr(l, "sam_bce_loss_table")
    assert l.sam_abi_version() == 9


def test_table_loss_entry_point_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from sam_textvqa_amd import _capi as capi
    l = capi.lib()
    nn = C.c_void_p(16)

    def call(fixed=nn, table=nn, B=2, L=12, R=24, V=200, No=50, d_fixed=nn, d_ocr=nn, ld=None):
        ldf, ldo = (V, No) if ld is None else ld
        return l.sam_bce_loss_table(fixed, ldf, nn, ldo, *([table] * 8), B, 200, L, 64, 256, nn, nn, R, V, No, 1.0, None, nn, d_fixed, V, d_ocr, No, None, None)

    assert call(fixed=None) == -1 and b"null" in l.sam_last_error()
    assert call(table=None) == -1 and b"null table" in l.sam_last_error()
    assert call(d_ocr=None) == -1 and b"together" in l.sam_last_error()
    assert call(R=25) == -1 and b"B * L" in l.sam_last_error()
    assert call(V=15951) == -1 and b"LDS" in l.sam_last_error()           # 15951 + 50 > 16000 floats
    assert call(ld=(199, 50)) == -1 and b"stride" in l.sam_last_error()


def test_sampler_entry_point_accepts_null_targets_but_still_checks_the_rest():
    import ctypes as C
    from sam_textvqa_amd import _capi as capi
    l = capi.lib()
    nn = C.c_void_p(16)
    # targets NULL passes the pointer check and is caught by the next one (bos outside the width), before anything is launched
    rc = l.sam_answer_sample(*([nn] * 8), 1, 200, 12, 64, 256, 62, 62, 0, None, 0, None, None, 0, *([nn] * 4), None)
    assert rc == -1 and b"bos" in l.sam_last_error()
    rc = l.sam_answer_sample(*([nn] * 8), 1, 200, 12, 64, 256, 62, 1, 0, None, 0, None, None, 0, None, *([nn] * 3), None)
    assert rc == -1 and b"null output" in l.sam_last_error()


def test_trainer_rejects_inconsistent_answer_modes():
    from sam_textvqa_amd.trainer import Trainer
    with pytest.raises(ValueError, match="answer_targets"):
        Trainer(None, answer_targets="sparse")
    with pytest.raises(ValueError, match="predictions"):
        Trainer(None, predictions=True)
