"""GPU: batches gathered from the resident feature store (csrc/store.hip, sam_textvqa_amd/store.py) on the MI355X -- the two
kernels against the host twin store.gather_host bit for bit (which tests/test_store_cpu.py pins to ragged.collate_ragged), every access path of the row
copy, the clamps, untouched rows past the total, bad indices, 64-bit source addressing and the batch end to end through ragged.to_padded.
No test captures a graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_MAX = 4
SENTINEL = 0x5A


def _sentinel_like(t, device=None):
    """a tensor of t's shape and dtype whose every byte is SENTINEL"""
    out = torch.empty_like(t, device=device)
    out.view(-1).view(torch.uint8).fill_(SENTINEL)
    return out


def _store(counts_obj, counts_ocr, image_of=None, seed=0):
    """obj rows 2048 fp16 (the c3 width: a 4 KB row), OCR rows 2048 fp16 + FastText 300 + PHOC 604, fp32 boxes; tables of both keys, one 3-dimensional"""
    from sam_textvqa_amd import store
    g = torch.Generator().manual_seed(seed)
    n = len(counts_obj)

    def group(counts, extra):
        feats = [torch.randn(c, 2048, generator=g) for c in counts]
        boxes = [torch.rand(c, 5, generator=g) for c in counts]
        ex = {"ft_rows": [torch.randn(c, 300, generator=g) for c in counts], "phoc_rows": [torch.rand(c, 604, generator=g) for c in counts]} if extra else None
        return store.build_group_from_rows(feats, boxes, extra=ex)

    nq = n if image_of is None else len(image_of)
    image_tables = {"ocr_text": torch.randint(1, 1 << 20, (n, N_MAX, 7), generator=g, dtype=torch.int32),          # 3-dimensional, 112-byte rows
                    "ocr_text_len": torch.randint(0, 8, (n, N_MAX), generator=g, dtype=torch.int32)}
    question_tables = {"question_indices": torch.randint(0, 30000, (nq, 20), generator=g), "answer_flag": torch.randint(0, 255, (nq, 3), generator=g).to(torch.uint8)}
    return store.build(group(counts_obj, False), group(counts_ocr, True), image_tables=image_tables, question_tables=question_tables,
                       image_of_question=None if image_of is None else torch.tensor(image_of, dtype=torch.int32))


def _gather_both(s_host, idx, s_dev=None, **kw):
    """store.gather on the GPU and store.gather_host, both into sentinel-filled destinations -> (device batch on the CPU, host batch, status pair)"""
    from sam_textvqa_amd import store
    idx = torch.tensor(idx, dtype=torch.int32)
    shape, _ = store.gather_host(s_host, idx.clamp(0, 0), max_obj_num=N_MAX, max_ocr_num=N_MAX)
    into_h = {k: _sentinel_like(v) for k, v in shape.items()}
    into_d = {k: _sentinel_like(v, device="cuda") for k, v in shape.items()}
    s_dev = s_dev if s_dev is not None else store.to(s_host, "cuda")
    got, st_d = store.gather(s_dev, idx.cuda(), into_d, max_obj_num=N_MAX, max_ocr_num=N_MAX, **kw)
    want, st_h = store.gather_host(s_host, idx, into=into_h, max_obj_num=N_MAX, max_ocr_num=N_MAX)
    assert got is into_d and st_d.dtype == torch.int32 and st_d.is_cuda
    return {k: v.cpu() for k, v in got.items()}, want, (st_d.cpu(), st_h)


def _assert_same_bytes(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].contiguous().view(-1).view(torch.uint8), want[k].contiguous().view(-1).view(torch.uint8)), k


COUNTS = [0, 1, N_MAX, N_MAX + 3, 2]                       # empty, one row, exactly the maximum, over it (clamped), two


@pytest.mark.parametrize("idx", [[1, 0, 2, 3, 4], [3, 3, 4, 0, 2]], ids=["each-count", "duplicated-image"])
def test_every_access_path_of_the_row_copy_and_rows_past_the_total(idx):
    """B = 5 on a 5-image store with the counts {0, 1, n_max, n_max + 3, 2} (five images: five distinct counts need them), once in an order that
    visits each and once with a duplicated image, through ops.store_gather_ragged with one part per path: 16-byte (4 KB fp16 rows; 8208-byte rows: the
    chunk loop runs three times; 53-byte rows at stride 64: a 5-byte tail), 4-byte (5 fp32; 22 bytes at stride 24: a 2-byte tail) and bytes (6-byte
    rows at source stride 9 from a misaligned base).  The destinations start as sentinel bytes: rows past the total and the bytes between strided
    rows must still hold them."""
    from sam_textvqa_amd import ops
    g = torch.Generator().manual_seed(5)
    off = [0] + list(np.cumsum(COUNTS))
    R, B, cap = off[-1], len(idx), len(idx) * N_MAX

    def strided_bytes(width, ld, shift=0):
        base = torch.randint(0, 256, (R * ld + shift,), generator=g, dtype=torch.uint8).cuda()
        return base, base[shift:].as_strided((R, width), (ld, 1))

    def strided_dst(width, ld):
        base = torch.full((cap * ld,), SENTINEL, dtype=torch.uint8, device="cuda")
        return base, base.as_strided((cap, width), (ld, 1))

    srcs = [torch.randn(R, 2048, generator=g).to(torch.float16).cuda(), torch.randn(R, 4104, generator=g).to(torch.float16).cuda(),
            strided_bytes(53, 64)[1], torch.rand(R, 5, generator=g).cuda(), strided_bytes(22, 24)[1], strided_bytes(6, 9, shift=1)[1]]
    assert srcs[5].data_ptr() % 2 == 1 and srcs[0].data_ptr() % 16 == 0 and srcs[3].data_ptr() % 16 == 0
    bases, dsts = [], []
    for k, src in enumerate(srcs):
        if src.dtype == torch.uint8:
            base, view = strided_dst(src.shape[1], {53: 64, 22: 24, 6: 6}[src.shape[1]])
        else:
            base = view = _sentinel_like(torch.empty(cap, src.shape[1], dtype=src.dtype), device="cuda")
        bases.append(base)
        dsts.append(view)
    counts = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    row_off = torch.tensor(off, dtype=torch.int64, device="cuda")
    ops.store_gather_ragged(torch.tensor(idx, dtype=torch.int32, device="cuda"), None, row_off, N_MAX, list(zip(srcs, dsts)), counts, status)
    kept = [min(COUNTS[g_], N_MAX) for g_ in idx]
    assert counts.tolist() == kept and status.tolist() == [0] * B
    pick = torch.tensor([off[g_] + i for g_, c in zip(idx, kept) for i in range(c)], device="cuda")
    total = pick.numel()
    assert 0 < total < cap
    for src, dst, base in zip(srcs, dsts, bases):
        assert torch.equal(dst[:total], src[pick]), (src.dtype, tuple(src.shape))
        assert bool((dst[total:].contiguous().view(-1).view(torch.uint8) == SENTINEL).all()), (src.dtype, tuple(src.shape))
        if base is not dst:                                               # the bytes between strided rows
            assert bool((base.view(cap, -1)[:, dst.shape[1]:] == SENTINEL).all()), tuple(src.shape)


@pytest.mark.parametrize("with_image_of", [False, True], ids=["image-indices", "question-indices"])
@pytest.mark.parametrize("case", ["B5", "B1", "B70"])
def test_gather_equals_the_host_twin_bit_for_bit(case, with_image_of):
    """both ragged groups and the fixed tables (both keys, a 3-dimensional table) against store.gather_host on sentinel-filled destinations: B = 5 with
    the counts of COUNTS and a duplicated image; B = 1; B = 70 with random counts, where the prefix loop crosses its 64-lane stride"""
    rng = np.random.RandomState(70)
    if case == "B70":
        counts_obj, counts_ocr = rng.randint(0, N_MAX + 4, 40).tolist(), rng.randint(0, N_MAX + 4, 40).tolist()
        image_of = rng.randint(0, 40, 90).tolist() if with_image_of else None
        idx = rng.randint(0, 90 if with_image_of else 40, 70).tolist()
    else:
        counts_obj, counts_ocr = COUNTS, COUNTS[::-1]
        image_of = [4, 3, 3, 0, 1, 2, 3] if with_image_of else None
        idx = ([1, 6, 3, 2, 5] if with_image_of else [3, 3, 4, 0, 2]) if case == "B5" else [1 if with_image_of else 3]
    s = _store(counts_obj, counts_ocr, image_of)
    got, want, (st_d, st_h) = _gather_both(s, idx)
    _assert_same_bytes(got, want)
    assert st_d.tolist() == st_h.tolist() == [0] * len(idx)
    imgs = [image_of[q] if with_image_of else q for q in idx]
    assert got["obj_count"].tolist() == [min(counts_obj[g], N_MAX) for g in imgs] and got["ocr_count"].tolist() == [min(counts_ocr[g], N_MAX) for g in imgs]
    total = int(got["obj_count"].sum())
    if total < len(idx) * N_MAX:                                          # rows past the total keep what they held
        assert bool((got["obj_rows"][total:].view(torch.uint8) == SENTINEL).all()) and bool((got["obj_box_rows"][total:].view(torch.uint8) == SENTINEL).all())
    assert torch.equal(got["ocr_text"], s["image_tables"]["ocr_text"][torch.tensor(imgs)])
    assert torch.equal(got["question_indices"], s["question_tables"]["question_indices"][torch.tensor(idx)])


def test_bad_indices_are_flagged_and_every_other_sample_is_unaffected():
    from sam_textvqa_amd import store
    image_of = [4, 3, 3, 0, 1, 2, 3]
    s = _store(COUNTS, COUNTS[::-1], image_of)
    s_dev = store.to(s, "cuda")
    good, _, _ = _gather_both(s, [1, 4, 5], s_dev=s_dev)
    bad_host = dict(s, image_of_question=s["image_of_question"].clone())
    bad_host["image_of_question"][2] = 5                                  # == n_images: corrupted after build(), on both sides
    bad_dev = dict(s_dev, image_of_question=bad_host["image_of_question"].cuda())
    idx = [-1, 1, 7, 4, 2, 5]                                             # -1 and n_questions; question 2's image is the corrupted entry
    got, want, (st_d, st_h) = _gather_both(bad_host, idx, s_dev=bad_dev)
    _assert_same_bytes(got, want)
    assert st_d.tolist() == st_h.tolist() == [1, 0, 1, 0, 1, 0]
    assert got["obj_count"].tolist() == [0, 4, 0, 1, 0, 4] and got["ocr_count"].tolist() == [0, 1, 0, 4, 0, 4]
    for k in ("obj_rows", "obj_box_rows", "ocr_rows", "ocr_ft_rows", "ocr_phoc_rows", "ocr_box_rows"):
        n = int(good[k[:3] + "_count"].sum())
        assert torch.equal(got[k][:n], good[k][:n]), k                    # the three good samples, back to back as if the bad ones were not there
    for k in ("ocr_text", "ocr_text_len", "question_indices", "answer_flag"):
        assert torch.equal(got[k][[1, 3, 5]], good[k]), k
        assert not got[k][0].any() and not got[k][2].any()                # zero rows, not the sentinel
    assert not got["ocr_text"][4].any() and torch.equal(got["question_indices"][4], s["question_tables"]["question_indices"][2])
    dev_idx = torch.tensor(idx, dtype=torch.int32, device="cuda")
    into = {k: torch.zeros_like(v, device="cuda") for k, v in want.items()}
    with pytest.raises(ValueError, match="sample 0 is flagged"):
        store.gather(bad_dev, dev_idx, into, max_obj_num=N_MAX, max_ocr_num=N_MAX, check=True)
    shape3, _ = store.gather_host(s, torch.tensor([1, 4, 5], dtype=torch.int32), max_obj_num=N_MAX, max_ocr_num=N_MAX)
    store.gather(s_dev, dev_idx[[1, 3, 5]].contiguous(), {k: torch.zeros_like(v, device="cuda") for k, v in shape3.items()}, max_obj_num=N_MAX, max_ocr_num=N_MAX,
                 check=True)                                              # clean indices pass the check
    sticky = torch.tensor([0, 2, 0, 0, 0, 0], dtype=torch.int32, device="cuda")          # status=: the bits are OR-ed into a resident tensor
    _, st = store.gather(bad_dev, dev_idx, into, max_obj_num=N_MAX, max_ocr_num=N_MAX, status=sticky)
    assert st is sticky and sticky.tolist() == [1, 2, 1, 0, 1, 0]


def test_a_corrupted_row_offset_is_cut_to_the_store_and_flagged():
    """row_off is device memory too: an end past the row count and a start below zero are cut to the rows the store holds (status bit 2) -- the
    kernel reads no row outside [0, total_rows)"""
    from sam_textvqa_amd import store
    s = _store(COUNTS, COUNTS[::-1])
    R = s["obj"]["rows"].shape[0]
    bad = dict(s, obj=dict(s["obj"], row_off=s["obj"]["row_off"].clone()))
    bad["obj"]["row_off"][5] = R + 1000                                   # image 4: [12, R + 1000) -> 2 rows left
    bad["obj"]["row_off"][0] = -3                                         # image 0: [-3, 0) -> nothing left
    got, want, (st_d, st_h) = _gather_both(bad, [4, 0, 2, 1])
    _assert_same_bytes(got, want)
    assert st_d.tolist() == st_h.tolist() == [2, 2, 0, 0] and got["obj_count"].tolist() == [R - 12, 0, 4, 1]


def test_source_addressing_is_64_bit():
    """a fp16 store of 1.1 M rows (4.5 GB, uninitialised but for two images): rows that straddle and rows that sit past byte offset 2^32"""
    from sam_textvqa_amd import ops
    R, n_max = 1_100_000, 12
    rows = torch.empty((R, 2048), dtype=torch.float16, device="cuda")
    boxes = torch.empty((R, 5), dtype=torch.float32, device="cuda")
    first = (1 << 32) // 4096 - 6                                         # image 1: ten rows, six below 2^32 bytes and four above
    off = [0, first, first + 10, R - 3, R]                                # image 3: the last three rows
    assert first * 4096 < 1 << 32 < (first + 10) * 4096 and rows.numel() * 2 > 1 << 32
    g = torch.Generator().manual_seed(64)
    known = torch.randn(13, 2048, generator=g).to(torch.float16).cuda()
    known_b = torch.rand(13, 5, generator=g).cuda()
    rows[first: first + 10], rows[R - 3:] = known[:10], known[10:]
    boxes[first: first + 10], boxes[R - 3:] = known_b[:10], known_b[10:]
    dst, dst_b = torch.zeros((2 * n_max, 2048), dtype=torch.float16, device="cuda"), torch.zeros((2 * n_max, 5), device="cuda")
    counts, status = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.store_gather_ragged(torch.tensor([3, 1], dtype=torch.int32, device="cuda"), None, torch.tensor(off, dtype=torch.int64, device="cuda"), n_max,
                            [(rows, dst), (boxes, dst_b)], counts, status)
    assert counts.tolist() == [3, 10] and status.tolist() == [0, 0]
    assert torch.equal(dst[:13], torch.cat([known[10:], known[:10]])) and torch.equal(dst_b[:13], torch.cat([known_b[10:], known_b[:10]]))
    assert not dst[13:].any() and not dst_b[13:].any()


def test_gathered_batch_equals_the_uploaded_collate_ragged_batch_end_to_end():
    """B = 3, 6 objects, 4 OCR rows: ragged.to_padded of the gathered batch == ragged.to_padded of collate_ragged + ragged.upload, on every key"""
    from sam_textvqa_amd import ragged, store
    g = torch.Generator().manual_seed(3)
    n_obj, n_ocr = [6, 9, 0, 3], [2, 4, 5, 0]                             # per image: over and under both maxima, and empty
    images = [{"obj_features": torch.randn(a, 2048, generator=g), "obj_bboxes": torch.rand(a, 5, generator=g), "ocr_features": torch.randn(c, 2048, generator=g),
               "ocr_bboxes": torch.rand(c, 5, generator=g), "ocr_fasttext": torch.randn(c, 300, generator=g), "ocr_phoc": torch.rand(c, 604, generator=g)}
              for a, c in zip(n_obj, n_ocr)]
    image_of = torch.tensor([1, 3, 1, 0, 2], dtype=torch.int32)
    qi = torch.randint(0, 30000, (5, 20), generator=g)
    obj = store.build_group_from_rows([im["obj_features"] for im in images], [im["obj_bboxes"] for im in images])
    ocr = store.build_group_from_rows([im["ocr_features"] for im in images], [im["ocr_bboxes"] for im in images],
                                      extra={"ft_rows": [im["ocr_fasttext"] for im in images], "phoc_rows": [im["ocr_phoc"] for im in images]})
    s = store.to(store.build(obj, ocr, question_tables={"question_indices": qi}, image_of_question=image_of), "cuda")
    idx = torch.tensor([2, 4, 3], dtype=torch.int32)
    host = ragged.collate_ragged([images[int(image_of[q])] for q in idx], max_obj_num=6, max_ocr_num=4)
    host["question_indices"] = qi[idx.long()]
    uploaded = ragged.upload(host, {k: torch.zeros_like(v, device="cuda") for k, v in host.items()})
    gathered, status = store.gather(s, idx.cuda(), {k: _sentinel_like(v, device="cuda") for k, v in host.items()}, max_obj_num=6, max_ocr_num=4, check=True)
    assert gathered["obj_count"].tolist() == [6, 0, 6] and gathered["ocr_count"].tolist() == [4, 4, 2] and not status.any()
    want, got = ragged.to_padded(uploaded), ragged.to_padded(gathered)
    assert set(got) == set(want) and {"pad_obj_features", "pad_obj_mask", "pad_obj_bboxes", "pad_ocr_features", "pad_ocr_mask", "pad_ocr_bboxes", "ocr_fasttext",
                                      "ocr_phoc", "question_indices"} <= set(got)
    for k in want:
        assert torch.equal(got[k], want[k]), k
