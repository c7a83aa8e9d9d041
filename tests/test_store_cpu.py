"""CPU: the resident feature store (sam_textvqa_amd/store.py) without a GPU -- the reader's 5-column boxes against the fixture
recorded from the reference's ImageFeaturesH5Reader, the host twin of the gather against ragged.collate_ragged, what build() refuses, the header registry
and the entry points' argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store.npz")


def _golden_items():
    """the fixture's images in the LMDB item schema, the feature rows regenerated from its seed, and the reader's boxes"""
    z = np.load(GOLDEN)
    n = len([k for k in z.files if k.startswith("boxes_")])
    seed = int(z["seed"])
    items = [{"features": np.random.RandomState(seed + g).rand(z["boxes_%d" % g].shape[0], 2048).astype(np.float32), "boxes": z["boxes_%d" % g],
              "image_w": int(z["size_%d" % g][0]), "image_h": int(z["size_%d" % g][1])} for g in range(n)]
    return items, [z["loc_%d" % g] for g in range(n)]


def _small_store(seed=0, n_images=6, d_obj=16, d_ocr=12, with_questions=True, obj_counts=None, ocr_counts=None):
    """a store with narrow rows (the host twin does not care about the width) and one table of each kind"""
    from sam_textvqa_amd import store
    rng = np.random.RandomState(seed)
    obj_counts = obj_counts or [0, 1, 6, 9, 2, 4][:n_images]
    ocr_counts = ocr_counts or [3, 0, 4, 7, 1, 2][:n_images]

    def group(counts, d, extra=False):
        feats = [rng.randn(c, d).astype(np.float32) for c in counts]
        boxes = [rng.rand(c, 5).astype(np.float32) for c in counts]
        ex = {"ft_rows": [rng.randn(c, 300).astype(np.float32) for c in counts], "phoc_rows": [rng.rand(c, 604).astype(np.float32) for c in counts]} if extra else None
        return store.build_group_from_rows(feats, boxes, extra=ex), feats, boxes, ex

    obj, ocr = group(obj_counts, d_obj), group(ocr_counts, d_ocr, extra=True)
    ioq = torch.tensor([3, 0, 3, 5, 1, 2, 4, 2, 0][: 9 if n_images >= 6 else 4], dtype=torch.int32) % n_images if with_questions else None
    nq = ioq.numel() if with_questions else n_images
    image_tables = {"ocr_text": torch.from_numpy(rng.randint(0, 99, (n_images, 4, 3)).astype(np.int32)),
                    "ocr_text_len": torch.from_numpy(rng.randint(0, 4, (n_images, 4)).astype(np.int32))}
    question_tables = {"question_indices": torch.from_numpy(rng.randint(0, 30000, (nq, 20))), "train_loss_mask": torch.from_numpy(rng.rand(nq, 12).astype(np.float32))}
    s = store.build(obj[0], ocr[0], image_tables=image_tables, question_tables=question_tables, image_of_question=ioq)
    return s, obj, ocr


# ---------------------------------------------------------------------------------------------- the reader's boxes
def test_build_group_boxes_equal_the_readers_bit_for_bit():
    from sam_textvqa_amd import store
    items, want = _golden_items()
    assert sorted({w.shape[0] for w in want}) == [0, 1, 2, 7]
    for it, w in zip(items, want):
        got = store.reader_boxes(it["boxes"], it["image_w"], it["image_h"])
        assert got.dtype == np.float32 and got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32))
    g = store.build_group(items)
    counts = [w.shape[0] for w in want]
    assert g["row_off"].dtype == torch.int64 and g["row_off"].tolist() == [0] + list(np.cumsum(counts))
    assert g["box_rows"].dtype == torch.float32 and np.array_equal(g["box_rows"].numpy().view(np.uint32), np.concatenate(want).view(np.uint32))
    # only the real rows, untouched but for the dtype: no average row, no [0, 0, 1, 1, 1] box
    assert g["rows"].dtype == torch.float16 and tuple(g["rows"].shape) == (sum(counts), 2048)
    assert torch.equal(g["rows"], torch.from_numpy(np.concatenate([it["features"] for it in items])).to(torch.float16))
    assert torch.equal(store.build_group(items, dtype=torch.float32)["rows"], torch.from_numpy(np.concatenate([it["features"] for it in items])))
    # the operation order matters: the area from the normalised coordinates, or in float64, gives other bits somewhere in the fixture
    other = 0
    for it, w in zip(items, want):
        b = it["boxes"].astype(np.float64)
        area = ((b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0]) / (it["image_w"] * it["image_h"])).astype(np.float32)
        other += int((area.view(np.uint32) != w[:, 4].view(np.uint32)).sum())
    assert other > 0


# ---------------------------------------------------------------------------------------------- the host twin
@pytest.mark.parametrize("with_questions", [True, False])
def test_gather_host_equals_collate_ragged_of_the_looked_up_samples(with_questions):
    from sam_textvqa_amd import ragged, store
    s, (_, of, ob, _), (_, cf, cb, ex) = _small_store(with_questions=with_questions)
    idx = torch.tensor([2, 0, 5, 3, 3] if not with_questions else [0, 8, 2, 5, 3, 0], dtype=torch.int32)
    max_obj, max_ocr = 6, 4                                     # images 3 (9 objects, 7 OCR rows) are clamped
    imgs = [int(s["image_of_question"][q]) if with_questions else int(q) for q in idx]
    samples = [{"obj_features": torch.from_numpy(of[g]), "obj_bboxes": torch.from_numpy(ob[g]), "ocr_features": torch.from_numpy(cf[g]),
                "ocr_bboxes": torch.from_numpy(cb[g]), "ocr_fasttext": torch.from_numpy(ex["ft_rows"][g]), "ocr_phoc": torch.from_numpy(ex["phoc_rows"][g])} for g in imgs]
    want = ragged.collate_ragged(samples, max_obj_num=max_obj, max_ocr_num=max_ocr)
    got, status = store.gather_host(s, idx, max_obj_num=max_obj, max_ocr_num=max_ocr, check=True)
    assert status.dtype == torch.int32 and status.tolist() == [0] * len(idx)
    for cnt_key, _, parts in ragged.GROUPS:
        assert got[cnt_key].dtype == torch.int32 and torch.equal(got[cnt_key], want[cnt_key])
        total = int(want[cnt_key].sum())
        for row_key, _ in parts:
            assert got[row_key].dtype == want[row_key].dtype and got[row_key].shape == want[row_key].shape
            assert torch.equal(got[row_key][:total], want[row_key][:total]) and not got[row_key][total:].any()
    assert got["obj_count"].tolist() == [min(len(of[g]), max_obj) for g in imgs]
    for k in ("ocr_text", "ocr_text_len"):
        assert torch.equal(got[k], s["image_tables"][k][torch.tensor(imgs)])
    for k in ("question_indices", "train_loss_mask"):
        assert torch.equal(got[k], s["question_tables"][k][idx.long()])
    # the padded forms agree (rows past the total are never read); the text keys are dropped: a batch gives PHOC rows or text, not both
    drop = ("ocr_text", "ocr_text_len", "question_indices", "train_loss_mask")
    pg, pw = ragged.to_padded({k: v for k, v in got.items() if k not in drop}), ragged.to_padded(want)
    assert set(pg) == set(pw)
    for k in pw:
        assert torch.equal(pg[k], pw[k]), k
    # into=: the valid prefix lands in the caller's tensors, rows past the total keep what they held
    into = {k: torch.full_like(v, 7) for k, v in got.items()}
    ret, _ = store.gather_host(s, idx, into=into, max_obj_num=max_obj, max_ocr_num=max_ocr)
    assert ret is into
    total = int(want["ocr_count"].sum())
    assert torch.equal(into["ocr_rows"][:total], want["ocr_rows"][:total]) and bool((into["ocr_rows"][total:] == 7).all())
    assert torch.equal(into["question_indices"], got["question_indices"]) and torch.equal(into["obj_count"], want["obj_count"])


def test_gather_host_flags_bad_indices_and_leaves_the_rest_alone():
    from sam_textvqa_amd import store
    s, _, _ = _small_store()
    good, _ = store.gather_host(s, torch.tensor([4, 6], dtype=torch.int32), max_obj_num=6, max_ocr_num=4)
    s2 = dict(s, image_of_question=s["image_of_question"].clone())
    s2["image_of_question"][7] = 99                                                     # corrupted after build()
    got, status = store.gather_host(s2, torch.tensor([-1, 4, 9, 7, 6], dtype=torch.int32), max_obj_num=6, max_ocr_num=4)
    assert status.tolist() == [1, 0, 1, 1, 0]
    assert got["obj_count"].tolist() == [0, int(good["obj_count"][0]), 0, 0, int(good["obj_count"][1])]
    n = int(good["obj_count"].sum())
    assert torch.equal(got["obj_rows"][:n], good["obj_rows"][:n])
    assert not got["question_indices"][0].any() and not got["question_indices"][2].any() and not got["ocr_text"][3].any()
    assert torch.equal(got["question_indices"][3], s["question_tables"]["question_indices"][7])      # the question is fine, its image is not
    assert torch.equal(got["question_indices"][[1, 4]], good["question_indices"]) and torch.equal(got["ocr_text"][[1, 4]], good["ocr_text"])
    with pytest.raises(ValueError, match="sample 0 is flagged"):
        store.gather_host(s2, torch.tensor([-1, 4], dtype=torch.int32), max_obj_num=6, max_ocr_num=4, check=True)
    # a row range that leaves the store is cut, with bit 2
    assert store._resolve([0, 5], 0, 4, 3) == (0, 3, 2) and store._resolve([2, 9], 0, 4, 5) == (2, 3, 2) and store._resolve([-2, 9], 0, 4, 50) == (0, 2, 2)
    assert store._resolve([7, 9], 0, 4, 5) == (0, 0, 2) and store._resolve([3, 1], 0, 4, 5) == (0, 0, 0) and store._resolve([1, 9], 0, 4, 50) == (1, 4, 0)


# ---------------------------------------------------------------------------------------------- what build() refuses
def test_build_refuses_inconsistent_stores():
    from sam_textvqa_amd import store
    s, (obj, *_), (ocr, *_) = _small_store()
    assert s["n_images"] == 6 and s["n_questions"] == 9 and store.nbytes(s) > 0
    bad = dict(obj, row_off=obj["row_off"].clone())
    bad["row_off"][2] = bad["row_off"][3] + 1
    with pytest.raises(ValueError, match="never decrease"):
        store.build(bad, ocr)
    with pytest.raises(ValueError, match="ends at"):
        store.build(dict(obj, rows=obj["rows"][:-1], box_rows=obj["box_rows"][:-1]), ocr)
    with pytest.raises(ValueError, match="ends at"):
        store.build(obj, dict(ocr, row_off=ocr["row_off"] + torch.tensor([0] * 6 + [1])))
    with pytest.raises(ValueError, match="box_rows"):
        store.build(dict(obj, box_rows=obj["box_rows"][:-1]), ocr)
    for ioq in ([0, 6], [-1, 2]):
        with pytest.raises(ValueError, match="outside"):
            store.build(obj, ocr, image_of_question=torch.tensor(ioq, dtype=torch.int32))
    with pytest.raises(ValueError, match="image table 'a'"):
        store.build(obj, ocr, image_tables={"a": torch.zeros(5, 3)})
    with pytest.raises(ValueError, match="question table 'q'"):
        store.build(obj, ocr, question_tables={"q": torch.zeros(6, 3)}, image_of_question=torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="images"):
        store.build(obj, store.build_group_from_rows([np.zeros((1, 12), np.float32)], [np.zeros((1, 5), np.float32)]))
    with pytest.raises(ValueError, match="twice or name a ragged tensor"):
        store.build(obj, ocr, image_tables={"obj_rows": torch.zeros(6, 3)})
    with pytest.raises(ValueError):
        store.build_group_from_rows([np.zeros((2, 12), np.float32)], [np.zeros((3, 5), np.float32)])
    ok = store.build(obj, ocr, question_tables={"q": torch.zeros(6, 3)})              # without image_of_question: one row per image
    assert ok["image_of_question"] is None and ok["n_questions"] == 6


# ---------------------------------------------------------------------------------------------- registry and C ABI
def test_the_header_parses_into_the_open_table_and_the_library_holds_the_kernels():
    from sam_textvqa_amd import _build, _capi
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "store" in _build.ABI_ADDITIONS and _build.ABI_ADDITIONS["store"] in _build.public_headers()
    assert _capi.ADDITION_SIGNATURES["store"] == {"sam_store_gather_ragged": [vp, i, vp, i, vp, i, i64, i, vp, i, vp, vp, i, vp],
                                                   "sam_store_gather_fixed": [vp, i, vp, i, i, vp, i, vp, vp]}
    assert _capi.ADDITION_RESTYPES["store"] == {"sam_store_gather_ragged": i, "sam_store_gather_fixed": i}
    assert os.path.join(_build.CSRC, "store.hip") in _build.sources()
    lib = _capi.lib()                                           # builds store.hip for gfx950 with the rest when the tree changed
    assert lib.sam_build_digest().decode() == _build._digest()
    for name, sig in _capi.ADDITION_SIGNATURES["store"].items():
        assert getattr(lib, name).argtypes == sig and getattr(lib, name).restype is i


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi, ops
    fake = 1 << 20                                              # never dereferenced: the checks reject the call before any launch

    def parts(n=1, words=5, **kw):
        arr = (ctypes.c_int64 * (words * max(n, 1)))()
        for k in range(n):
            d = dict(src=fake, ld_src=64, dst=fake, ld_dst=64, row_bytes=64, key=0)
            d.update(kw)
            arr[k * words: k * words + words] = [d["src"], d["ld_src"], d["dst"], d["ld_dst"], d["row_bytes"], d["key"]][:words]
        return arr

    def ragged(idx=fake, b=2, image_of=fake, nq=5, row_off=fake, ni=3, total=10, n_max=4, p=None, n_parts=1, counts=fake, status=fake, cap=8):
        return _capi.call("sam_store_gather_ragged", idx, b, image_of, nq, row_off, ni, total, n_max, p if p is not None else parts(), n_parts, counts, status, cap, None)

    def fixed(idx=fake, b=2, image_of=fake, nq=5, ni=3, p=None, n_parts=1, status=fake):
        return _capi.call("sam_store_gather_fixed", idx, b, image_of, nq, ni, p if p is not None else parts(words=6), n_parts, status, None)

    for kw in (dict(idx=None), dict(row_off=None), dict(counts=None), dict(status=None)):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            ragged(**kw)
    for kw in (dict(b=0), dict(n_max=0), dict(cap=0), dict(b=1 << 16, n_max=1 << 15)):
        with pytest.raises(_capi.SamHipError, match="bad shape"):
            ragged(**kw)
    with pytest.raises(_capi.SamHipError, match="bad store"):
        ragged(total=-1)
    with pytest.raises(_capi.SamHipError, match="must equal n_images"):
        ragged(image_of=None)
    with pytest.raises(_capi.SamHipError, match="misaligned"):
        ragged(row_off=fake + 4)
    with pytest.raises(_capi.SamHipError, match="9 parts") as e:
        ragged(p=parts(9), n_parts=9)
    assert "rc=-2" in str(e.value)                              # SAM_ERR_UNSUPPORTED
    with pytest.raises(_capi.SamHipError, match="no parts"):
        ragged(n_parts=0)
    for kw in (dict(row_bytes=0), dict(ld_src=63), dict(ld_dst=8)):
        with pytest.raises(_capi.SamHipError, match="row_bytes"):
            ragged(p=parts(**kw))
    with pytest.raises(_capi.SamHipError, match="part 0: null pointer"):
        ragged(p=parts(src=0))
    for kw in (dict(idx=None), dict(status=None)):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            fixed(**kw)
    with pytest.raises(_capi.SamHipError, match="bad shape"):
        fixed(b=0)
    with pytest.raises(_capi.SamHipError, match="key 2"):
        fixed(p=parts(words=6, key=2))
    with pytest.raises(_capi.SamHipError, match="9 parts"):
        fixed(p=parts(9, words=6), n_parts=9)
    # the Python wrappers: CPU tensors are refused, there is no fallback
    idx, st = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_capi.SamHipError):
        ops.store_gather_ragged(idx, None, torch.zeros(3, dtype=torch.int64), 4, [(torch.zeros(4, 8), torch.zeros(8, 8))], torch.zeros(2, dtype=torch.int32), st)
    with pytest.raises(_capi.SamHipError):
        ops.store_gather_fixed(idx, None, 2, [(torch.zeros(2, 8), torch.zeros(2, 8), 0)], st)
