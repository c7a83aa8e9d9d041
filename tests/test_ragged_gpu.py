"""GPU: sam_ragged_expand (csrc/ragged.hip) and the ragged batch path through the model, the trainer and the decoders.

Kernel cases: B = 5 (not a multiple of the 4 rows of a block), max_obj = 9, max_ocr = 6, the real widths 2048 / 300 / 604 / 5 (the width-specific code
paths), counts obj [9, 0, 1, 4, 9] / ocr [0, 6, 0, 3, 1], one valid row all zeros, source rows past the total NaN, destinations pre-filled with 7.0.
The padded oracle is computed once on the host (the torch twin of ragged.py, itself checked against _pad_features in test_ragged_cpu.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close_bf16

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
B, MAX_OBJ, MAX_OCR = 5, 9, 6
OBJ_COUNTS, OCR_COUNTS = [9, 0, 1, 4, 9], [0, 6, 0, 3, 1]
WIDTHS = dict(obj_rows=2048, obj_box_rows=5, ocr_rows=2048, ocr_ft_rows=300, ocr_phoc_rows=604, ocr_box_rows=5)


@functools.lru_cache(maxsize=None)
def case(dtype):
    """(ragged host batch with NaN past the totals, padded oracle: the twin's expansion of the same stored values) -- built once per source dtype"""
    from sam_textvqa_amd import ragged as R
    g = torch.Generator().manual_seed(5)
    scale = dict(obj_rows=0.2, ocr_rows=0.2, ocr_ft_rows=1.0, ocr_phoc_rows=3.0)
    host = {}
    for cnt_key, counts, n_max in (("obj_count", OBJ_COUNTS, MAX_OBJ), ("ocr_count", OCR_COUNTS, MAX_OCR)):
        total = sum(counts)
        for k, w in WIDTHS.items():
            if k[:3] != cnt_key[:3]:
                continue
            rows = torch.full((B * n_max, w), float("nan"))
            rows[:total] = torch.randn(total, w, generator=g) * scale.get(k, 1.0)
            host[k] = rows if k in R.BOX_KEYS else rows.to(dtype)
        host[cnt_key] = torch.tensor(counts, dtype=torch.int32)
    host["ocr_phoc_rows"][7] = 0                      # a valid row (sample 3, row 1) that is all zeros: x / max(0, eps) = 0, no NaN
    host["obj_rows"][2] = 0
    return host, R.to_padded(host)


def cuda(bd):
    return {k: (v.cuda() if torch.is_tensor(v) else ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v)) for k, v in bd.items()}


def pack_ocr(ops, dev, counts, normalize, fill=7.0):
    """the OCR encoder operand FastText 300 | PHOC 604 | FRCN 2048 | 50 zeros, K padded 3002 -> 3008, + boxes + mask: one launch"""
    out = torch.full((B * MAX_OCR, 3008), fill, dtype=BF16, device="cuda")
    boxes = torch.full((B * MAX_OCR, 5), fill, device="cuda")
    mask = torch.full((B, MAX_OCR), 7, dtype=torch.int64, device="cuda")
    parts = [(dev["ocr_box_rows"], boxes, 0, False, 0), (dev["ocr_ft_rows"], out, 0, normalize, 0), (dev["ocr_phoc_rows"], out, 300, normalize, 0),
             (dev["ocr_rows"], out, 904, normalize, 3008)]
    ops.ragged_expand(counts, MAX_OCR, parts, mask=mask)
    return out, boxes, mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("normalize", [True, False])
def test_packed_operand_matches_normalize_cat_of_the_padded_oracle(normalize, dtype):
    from sam_textvqa_amd import ops
    host, pad = case(dtype)
    dev = cuda(host)
    nz = (lambda x: F.normalize(x, dim=-1)) if normalize else (lambda x: x)
    # OCR: three blocks, 50 zero columns and the K padding
    out, boxes, mask = pack_ocr(ops, dev, dev["ocr_count"], normalize)
    ref = torch.cat([nz(pad["ocr_fasttext"]), nz(pad["ocr_phoc"]), nz(pad["pad_ocr_features"]), torch.zeros(B, MAX_OCR, 56)], dim=-1).view(B * MAX_OCR, 3008)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    assert (got[:, 2952:] == 0).all()                                          # the 50 zero columns and the K padding
    padded = (pad["pad_ocr_mask"] == 0).view(-1)
    assert padded.sum() == B * MAX_OCR - sum(OCR_COUNTS) and (got[padded] == 0).all()
    assert_close_bf16(got, ref, ulps=1, name="ragged ocr operand")
    assert (got[3 * MAX_OCR + 1, 300:904] == 0).all()                          # the all-zero PHOC row (source row 7 = sample 3, row 1)
    assert torch.equal(mask.cpu(), pad["pad_ocr_mask"]) and torch.equal(boxes.cpu().view(B, MAX_OCR, 5), pad["pad_ocr_bboxes"])
    # objects: one 2048-wide block
    out = torch.full((B * MAX_OBJ, 2048), 7.0, dtype=BF16, device="cuda")
    ops.ragged_expand(dev["obj_count"], MAX_OBJ, [(dev["obj_rows"], out, 0, normalize, 2048)])
    got = out.float().cpu()
    assert torch.isfinite(got).all() and (got[(pad["pad_obj_mask"] == 0).view(-1)] == 0).all()
    assert_close_bf16(got, nz(pad["pad_obj_features"]).view(B * MAX_OBJ, 2048), ulps=1, name="ragged obj operand")
    assert (got[2] == 0).all()                                                 # the all-zero object row


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_copy_form_is_bit_exact(dtype):
    from sam_textvqa_amd import ops, ragged as R
    host, pad = case(dtype)
    dev = cuda(host)
    got = R.to_padded(dev)
    for k in R.PADDED_KEYS:
        assert got[k].dtype == pad[k].dtype and torch.equal(got[k].cpu(), pad[k]), k
    assert not set(R.RAGGED_KEYS) & set(got)
    # the same through pre-filled destinations: nothing of the 7.0 survives
    dsts = {k: torch.full((B * MAX_OCR, WIDTHS[k]), 7.0, device="cuda") for k, _ in R.OCR_PARTS}
    mask = torch.full((B, MAX_OCR), 7, dtype=torch.int64, device="cuda")
    ops.ragged_expand(dev["ocr_count"], MAX_OCR, [(dev[k], dsts[k], 0, False, 0) for k, _ in R.OCR_PARTS], mask=mask)
    for k, pk in R.OCR_PARTS:
        assert torch.equal(dsts[k].cpu().view(B, MAX_OCR, -1), pad[pk]), k
    assert torch.equal(mask.cpu(), pad["pad_ocr_mask"])


def test_edge_cases_counts_clamps_determinism_and_bad_arguments():
    from sam_textvqa_amd import _capi as capi, ops
    from sam_textvqa_amd._capi import SamHipError
    host, pad = case(torch.float32)
    dev = cuda(host)
    # all counts 0: everything zero, no source row read (all NaN here)
    nan_src = {k: torch.full_like(v, float("nan")) if v.is_floating_point() else v for k, v in dev.items()}
    out, boxes, mask = pack_ocr(ops, nan_src, torch.zeros(B, dtype=torch.int32, device="cuda"), True)
    assert (out == 0).all() and (boxes == 0).all() and (mask == 0).all()
    # planted counts 12 and -3 are clamped to n_max and 0: the output of the clamped counts
    full = {k: torch.nan_to_num(v, nan=0.5) if v.is_floating_point() else v for k, v in dev.items()}      # (12 -> 6 moves rows: every source row is read)
    planted = torch.tensor([12, -3, 0, 3, 1], dtype=torch.int32, device="cuda")
    clamped = torch.tensor([6, 0, 0, 3, 1], dtype=torch.int32, device="cuda")
    a, b = pack_ocr(ops, full, planted, True), pack_ocr(ops, full, clamped, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[2].cpu().tolist() == [[1] * 6, [0] * 6, [0] * 6, [1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    assert torch.equal(a[1].view(B, MAX_OCR, 5)[3, :3], full["ocr_box_rows"][6:9])      # sample 3 starts behind the 6 + 0 + 0 rows in front of it
    # two identical calls: identical bits
    c, d = pack_ocr(ops, dev, dev["ocr_count"], True), pack_ocr(ops, dev, dev["ocr_count"], True)
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    # bad arguments
    out = torch.empty((B * MAX_OCR, 3008), dtype=BF16, device="cuda")
    with pytest.raises(SamHipError):
        ops.ragged_expand(dev["ocr_count"], MAX_OCR, [(dev["ocr_rows"], out, 964, True, 0)])          # col0 + width = 3012 > ld_dst = 3008
    with pytest.raises(SamHipError):
        ops.ragged_expand(dev["ocr_count"], MAX_OCR, [(dev["ocr_ft_rows"], out, 0, True, 0)] * 7)     # more than 6 parts
    with pytest.raises(SamHipError):
        ops.ragged_expand(None, MAX_OCR, [(dev["ocr_ft_rows"], out, 0, True, 0)], batch=B)            # null counts
    with pytest.raises(SamHipError):
        capi.call("sam_ragged_expand", None, B, MAX_OCR, B * MAX_OCR, None, 0, 1e-12, None, None)


SHAPES = (7, 20, 9, 3)                 # a small config of tests/test_model_gpu.py::test_sam4c_train_forward_backward_vs_oracle


def small_batch(seed, n=3, device="cpu"):
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(n, *SHAPES, vocab=300, context=3, device=device, seed=seed)
    bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
    return bd


def test_model_forward_on_a_ragged_batch_vs_oracle():
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    from tests.test_model_gpu import L, _small_full_model, score_err, within
    model, ref = _small_full_model(3, ("n", "s"), SHAPES)
    rag_cpu = R.from_padded(small_batch(11), feature_dtype=torch.float32)
    pad_cpu = R.to_padded(rag_cpu)                                             # the padded batch as the dataset builds it: zero rows behind the valid ones
    ref.train()
    with torch.no_grad():
        out_ref = ref(clone_batch(pad_cpu))["textvqa_scores"]
    model.cuda().train()
    prepare(model)
    bd = cuda(rag_cpu)
    out = model(bd)["textvqa_scores"]
    torch.cuda.synchronize()
    for k in ("pad_obj_mask", "pad_ocr_mask", "pad_obj_bboxes", "pad_ocr_bboxes"):
        assert bd[k].dtype == pad_cpu[k].dtype and torch.equal(bd[k].cpu(), pad_cpu[k]), k
    assert "pad_obj_features" not in bd and "_sam_obj_operand" not in bd and "_sam_ocr_operand" not in bd
    within("sam4c scores on a ragged batch", score_err(out, out_ref), L["sam4c_scores"])
    with pytest.raises(ValueError):
        model(dict(cuda(rag_cpu), pad_ocr_features=pad_cpu["pad_ocr_features"].cuda()))


def test_trainer_replays_the_captured_step_on_other_counts():
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_model_gpu import _small_full_model
    batches = [R.from_padded(small_batch(s, n=4, device="cuda")) for s in (21, 22)]        # fp16 rows
    assert not torch.equal(batches[0]["ocr_count"], batches[1]["ocr_count"])
    order = [0, 1, 0, 1]                                                       # warm-up, capture + replay, replay, replay
    runs = []
    for use_graph in (True, False):
        model, _ = _small_full_model(3, ("n", "s"), SHAPES)
        tr = Trainer(model, base_lr=1e-3, seed=3, use_graph=use_graph)
        losses, graphs = [], []
        for i in order:
            losses.append(tr.step(clone_batch(batches[i])).item())
            graphs.append(tr._graph)
        if use_graph:
            assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[2:])      # other counts: no recapture
            bufs = tr.input_buffers()
            assert set(R.RAGGED_KEYS) <= set(bufs) and not set(R.PADDED_KEYS) & set(bufs)
            assert bufs["obj_rows"].dtype == torch.float16 and bufs["ocr_count"].dtype == torch.int32
        tr.flush_update()
        runs.append(losses)
    l1, l0 = runs
    assert all(torch.isfinite(torch.tensor(l1))) and l1[0] != l1[1]
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(l0, l1)), (l0, l1)


def test_greedy_and_beam_decoding_of_a_ragged_batch_equal_the_padded_form():
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.registry import registry
    from sam_textvqa_amd.synthetic import clone_batch
    from tests.test_model_gpu import _small_full_model
    model, _ = _small_full_model(3, ("n", "s"), SHAPES)
    model.cuda().eval()
    prepare(model)
    rag = R.from_padded(small_batch(23, n=4, device="cuda"))
    rag["train_prev_inds"] = torch.zeros_like(rag["train_prev_inds"])
    rag["train_prev_inds"][:, 0] = 1
    pad = R.to_padded(rag)
    registry.EOS_IDX, registry.BOS_IDX = 2, 1
    model.set_beam_size(3)
    with torch.no_grad():
        a, b = clone_batch(rag), clone_batch(pad)
        sa, sb = model(a)["textvqa_scores"], model(b)["textvqa_scores"]
        assert torch.equal(sa.argmax(-1), sb.argmax(-1)) and torch.equal(a["train_prev_inds"], b["train_prev_inds"])
        assert "pad_ocr_features" in a and "ocr_count" not in a             # greedy decoding expands first, then runs as on a padded batch
        ba, bb = model(clone_batch(rag), use_beam_search=True), model(clone_batch(pad), use_beam_search=True)
        assert ba["complete_seqs"].reshape(-1, SHAPES[3]).shape[0] == 4 * 3
        assert torch.equal(ba["complete_seqs"], bb["complete_seqs"]) and torch.equal(ba["topkscores"], bb["topkscores"])
