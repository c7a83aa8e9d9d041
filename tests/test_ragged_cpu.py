"""CPU (no GPU needed): the ragged batch contract of sam_textvqa_amd.ragged -- collate_ragged / to_padded (torch twin) against a NumPy restatement of
the dataset's _pad_features (sam/datasets/textvqa_dataset.py:285-305), the from_padded round trip, the argument errors, and upload's prefix-only copies."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import ragged as R

MAX_OBJ, MAX_OCR, DF = 7, 4, 24
N_OBJ = [7, 0, 3, 11, 1]              # 11 > MAX_OBJ: truncated
N_OCR = [0, 4, 9, 2, 1]               # 9 > MAX_OCR: truncated


def pad_features_np(features, bboxes, num_boxes, max_feat_num):
    """textvqa_dataset.py:285-305 restated: mix_num_boxes = min(num_boxes, max); zero-filled [max, D] features and [max, 5] boxes holding the first
    mix_num_boxes rows; mask = [1] * mix_num_boxes, padded with 0"""
    mix_num_boxes = min(int(num_boxes), int(max_feat_num))
    mask = [1] * mix_num_boxes
    while len(mask) < max_feat_num:
        mask.append(0)
    mix_boxes_pad = np.zeros((max_feat_num, 5), dtype=np.float32)
    mix_boxes_pad[:mix_num_boxes] = bboxes[:mix_num_boxes]
    mix_features_pad = np.zeros((max_feat_num, features.shape[-1]), dtype=np.float32)
    mix_features_pad[:mix_num_boxes] = features[:mix_num_boxes]
    return mix_features_pad, np.array(mask, dtype=np.int64), mix_boxes_pad


def make_samples(seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return [dict(obj_features=rn(n, 2048), obj_bboxes=torch.rand(n, 5, generator=g), ocr_features=rn(m, DF), ocr_fasttext=rn(m, 300),
                 ocr_phoc=torch.rand(m, 604, generator=g), ocr_bboxes=torch.rand(m, 5, generator=g)) for n, m in zip(N_OBJ, N_OCR)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_collate_then_to_padded_equals_pad_features(dtype):
    samples = make_samples()
    host = R.collate_ragged(samples, MAX_OBJ, MAX_OCR, feature_dtype=dtype)
    assert host["obj_count"].dtype == torch.int32 and host["obj_count"].tolist() == [min(n, MAX_OBJ) for n in N_OBJ]
    assert host["ocr_count"].tolist() == [min(m, MAX_OCR) for m in N_OCR]
    assert host["obj_rows"].shape == (len(samples) * MAX_OBJ, 2048) and host["obj_rows"].dtype == dtype
    assert host["ocr_rows"].shape == (len(samples) * MAX_OCR, DF) and host["ocr_phoc_rows"].dtype == dtype
    assert host["obj_box_rows"].dtype == torch.float32 and host["ocr_box_rows"].dtype == torch.float32
    for k in ("obj_rows", "ocr_rows", "ocr_ft_rows", "ocr_phoc_rows", "obj_box_rows", "ocr_box_rows"):      # rows past the total must never be read
        total = int(host["obj_count" if k.startswith("obj") else "ocr_count"].sum())
        host[k][total:] = float("nan")
    pad = R.to_padded(host)
    assert set(R.PADDED_KEYS) <= set(pad) and not set(R.RAGGED_KEYS) & set(pad)
    rt = lambda x: x.to(dtype).float().numpy()                # what the stored dtype keeps of a feature
    for b, s in enumerate(samples):
        f, m, bx = pad_features_np(rt(s["obj_features"]), s["obj_bboxes"].numpy(), N_OBJ[b], MAX_OBJ)
        np.testing.assert_array_equal(pad["pad_obj_features"][b].numpy(), f)
        np.testing.assert_array_equal(pad["pad_obj_mask"][b].numpy(), m)
        np.testing.assert_array_equal(pad["pad_obj_bboxes"][b].numpy(), bx)
        f, m, bx = pad_features_np(rt(s["ocr_features"]), s["ocr_bboxes"].numpy(), N_OCR[b], MAX_OCR)
        np.testing.assert_array_equal(pad["pad_ocr_features"][b].numpy(), f)
        np.testing.assert_array_equal(pad["pad_ocr_mask"][b].numpy(), m)
        np.testing.assert_array_equal(pad["pad_ocr_bboxes"][b].numpy(), bx)
        np.testing.assert_array_equal(pad["ocr_fasttext"][b].numpy(), pad_features_np(rt(s["ocr_fasttext"]), s["ocr_bboxes"].numpy(), N_OCR[b], MAX_OCR)[0])
        np.testing.assert_array_equal(pad["ocr_phoc"][b].numpy(), pad_features_np(rt(s["ocr_phoc"]), s["ocr_bboxes"].numpy(), N_OCR[b], MAX_OCR)[0])
    assert pad["pad_obj_mask"].dtype == torch.int64 and pad["pad_obj_features"].dtype == torch.float32


def test_from_padded_round_trips():
    host = R.collate_ragged(make_samples(1), MAX_OBJ, MAX_OCR, feature_dtype=torch.float32)
    host["question_indices"] = torch.arange(10).view(5, 2)
    pad = R.to_padded(host)
    assert pad["question_indices"] is host["question_indices"]            # other entries are carried over
    back = R.from_padded(pad, feature_dtype=torch.float32)
    assert torch.equal(back["obj_count"], host["obj_count"]) and torch.equal(back["ocr_count"], host["ocr_count"]) and back["obj_count"].dtype == torch.int32
    for k in R.RAGGED_KEYS:
        if k.endswith("count"):
            continue
        total = int(host["obj_count" if k.startswith("obj") else "ocr_count"].sum())
        assert back[k].shape == host[k].shape and back[k].dtype == host[k].dtype
        assert torch.equal(back[k][:total], host[k][:total]) and (back[k][total:] == 0).all(), k
    again = R.to_padded(back)
    for k in R.PADDED_KEYS:
        assert torch.equal(again[k], pad[k]), k
    half = R.from_padded(pad)                                                # default: fp16 features, fp32 boxes
    assert half["obj_rows"].dtype == torch.float16 and half["ocr_ft_rows"].dtype == torch.float16 and half["obj_box_rows"].dtype == torch.float32


def test_twin_clamps_counts_and_source_rows():
    rows = torch.arange(12, dtype=torch.float32).view(6, 2) + 1
    out, mask = R.expand_rows_torch(rows, torch.tensor([5, -3, 2], dtype=torch.int32), 2)       # 5 -> 2, -3 -> 0
    assert mask.tolist() == [[1, 1], [0, 0], [1, 1]]
    assert torch.equal(out[0], rows[0:2]) and (out[1] == 0).all() and torch.equal(out[2], rows[2:4])


def test_non_prefix_mask_and_mixed_keys_raise():
    pad = R.to_padded(R.collate_ragged(make_samples(2), MAX_OBJ, MAX_OCR))
    bad = dict(pad)
    bad["pad_ocr_mask"] = pad["pad_ocr_mask"].clone()
    bad["pad_ocr_mask"][1, 1] = 0                                            # 1 0 1 1: a hole
    with pytest.raises(ValueError, match="prefix"):
        R.from_padded(bad)
    host = R.collate_ragged(make_samples(2), MAX_OBJ, MAX_OCR)
    mixed = dict(host, pad_obj_features=pad["pad_obj_features"])
    with pytest.raises(ValueError, match="padded"):
        R.to_padded(mixed)
    with pytest.raises(ValueError, match="padded"):
        R.check(dict(host, pad_ocr_features=pad["pad_ocr_features"]))
    lacking = {k: v for k, v in host.items() if k != "ocr_phoc_rows"}
    with pytest.raises(ValueError, match="lacks"):
        R.to_padded(lacking)


def test_model_forward_refuses_ragged_rows_next_to_padded_features():
    """SAM4C.forward checks the batch before anything is launched"""
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n",), n_dec=3, T=7, n_obj=MAX_OBJ, n_ocr=MAX_OCR)
    md.update(intermediate_size=64)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1, intermediate_size=64, vocab_size=50)),
                    num_answers=20, bos_idx=1)
    host = R.collate_ragged(make_samples(2), MAX_OBJ, MAX_OCR)
    host["pad_obj_features"] = torch.zeros(5, MAX_OBJ, 2048)
    with pytest.raises(ValueError, match="padded"):
        model(host)


def test_upload_moves_only_the_valid_prefix():
    host = R.collate_ragged(make_samples(3), MAX_OBJ, MAX_OCR)
    host["question_indices"] = torch.arange(10).view(5, 2)
    dev = {k: torch.full_like(v, 77) for k, v in host.items()}
    dev["unrelated"] = torch.full((3,), 77.0)
    got = R.upload(host, dev)
    assert got is dev
    for k in R.RAGGED_KEYS:
        if k.endswith("count"):
            assert torch.equal(dev[k], host[k])
            continue
        total = int(host["obj_count" if k.startswith("obj") else "ocr_count"].sum())
        assert 0 < total < host[k].shape[0]
        assert torch.equal(dev[k][:total], host[k][:total]), k
        assert (dev[k][total:] == 77).all(), k                               # rows past the total keep the sentinel
    assert torch.equal(dev["question_indices"], host["question_indices"]) and (dev["unrelated"] == 77).all()
    with pytest.raises(ValueError):
        R.upload(host, dict(dev, obj_rows=dev["obj_rows"].float()))
