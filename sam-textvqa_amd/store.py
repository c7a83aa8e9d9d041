"""Region features resident in device memory; a batch is a list of indices.

The reference keeps the whole feature set in host memory (ImageFeaturesH5Reader(in_memory=True), sam/datasets/_image_features_reader.py:121-188) and
TextVQADataset.__getitem__ looks an image's rows up, drops the prepended average row and pads (textvqa_dataset.py:307-334).  Here the same set lives in
HBM as two CSR groups -- the real rows of all images back to back, fp16 by default, and an int64 row offset per image --

    group = {"rows": [R, D] dtype, "box_rows": fp32 [R, 5], "row_off": int64 [n_images + 1]}        (the OCR group may also hold "ft_rows" [R, 300] and
                                                                                                       "phoc_rows" [R, 604], rows aligned with "rows")

next to fixed-width per-image and per-question tensors (packed text, ids, answer tables) and the image of every question.  gather() then writes the
ragged batch that ragged.upload fills today -- obj_rows / obj_box_rows / obj_count, ocr_rows / ocr_box_rows / ocr_count (+ ocr_ft_rows / ocr_phoc_rows
when the store holds them) and every table key the destination holds -- in three launches (ops.store_gather_ragged per group, ops.store_gather_fixed),
with nothing read back by the host.  gather_host is its twin on CPU tensors: ragged.collate_ragged of the looked-up samples plus index selects.

Nothing is converted by the gather: the store is built in the dtype the batch ships."""
import numpy as np
import torch

from . import ragged as _ragged

BAD_INDEX, BAD_RANGE = 1, 2                     # status bits (include/sam_hip_store.h)
# (store key, batch key, sample key of collate_ragged) per group, in ragged.GROUPS' order
GROUP_ROWS = {"obj": (("rows", "obj_rows", "obj_features"), ("box_rows", "obj_box_rows", "obj_bboxes")),
              "ocr": (("rows", "ocr_rows", "ocr_features"), ("ft_rows", "ocr_ft_rows", "ocr_fasttext"), ("phoc_rows", "ocr_phoc_rows", "ocr_phoc"),
                      ("box_rows", "ocr_box_rows", "ocr_bboxes"))}
COUNT_KEYS = {"obj": "obj_count", "ocr": "ocr_count"}
MAX_PARTS = 8                                   # per launch


def reader_boxes(boxes, image_w, image_h):
    """pixel xyxy [n, 4] -> the reader's 5 columns, float32 [n, 5], in its operation order (_image_features_reader.py:155-169): the area column from the
    PIXEL coordinates over float32(float(w) * float(h)) first, then the four coordinates over float32(w) / float32(h)"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    loc = np.zeros((b.shape[0], 5), dtype=np.float32)
    loc[:, :4] = b
    w, h = float(int(image_w)), float(int(image_h))
    loc[:, 4] = (loc[:, 3] - loc[:, 1]) * (loc[:, 2] - loc[:, 0]) / np.float32(w * h)
    loc[:, 0] = loc[:, 0] / np.float32(w)
    loc[:, 1] = loc[:, 1] / np.float32(h)
    loc[:, 2] = loc[:, 2] / np.float32(w)
    loc[:, 3] = loc[:, 3] / np.float32(h)
    return loc


def build_group_from_rows(features_list, boxes5_list, dtype=torch.float16, extra=None):
    """per-image rows already in the reader's output form WITHOUT its prepended average row (features [n, D], boxes [n, 5]; n = 0 is legal) -> the CSR
    group on the CPU.  extra: {"ft_rows": [per-image [n, 300]], "phoc_rows": [per-image [n, 604]]}, stored as `dtype` too."""
    if len(features_list) != len(boxes5_list) or not features_list:
        raise ValueError("store: %d feature matrices and %d box matrices (need one of each per image, at least one image)" % (len(features_list), len(boxes5_list)))
    feats = [torch.as_tensor(np.asarray(f) if not torch.is_tensor(f) else f) for f in features_list]
    boxes = [torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b) for b in boxes5_list]
    D = max(int(f.shape[1]) for f in feats if f.dim() == 2) if any(f.dim() == 2 for f in feats) else 0
    for g, (f, b) in enumerate(zip(feats, boxes)):
        if f.dim() != 2 or f.shape[1] != D or D == 0 or b.dim() != 2 or b.shape[1] != 5 or b.shape[0] != f.shape[0]:
            raise ValueError("store: image %d has features %s and boxes %s; expected [n, %d] and [n, 5]" % (g, tuple(f.shape), tuple(b.shape), D))
    counts = torch.tensor([f.shape[0] for f in feats], dtype=torch.int64)
    group = {"rows": torch.cat(feats).to(dtype).contiguous(), "box_rows": torch.cat(boxes).to(torch.float32).contiguous(),
             "row_off": torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])}
    for key, per_image in (extra or {}).items():
        if key not in ("ft_rows", "phoc_rows") or len(per_image) != len(feats):
            raise ValueError("store: extra rows %r (ft_rows / phoc_rows, one matrix per image)" % key)
        mats = [torch.as_tensor(np.asarray(m) if not torch.is_tensor(m) else m) for m in per_image]
        if any(m.dim() != 2 or m.shape[0] != f.shape[0] or m.shape[1] != mats[0].shape[1] for m, f in zip(mats, feats)):
            raise ValueError("store: %s must give one [n, width] matrix per image, n as its features" % key)
        group[key] = torch.cat(mats).to(dtype).contiguous()
    return group


def build_group(items, dtype=torch.float16, extra=None):
    """items in the LMDB schema ({"features": [n, 2048], "boxes": [n, 4] pixel xyxy, "image_w", "image_h"}) -> the CSR group on the CPU.  Only the real
    rows are stored: the average row and the [0, 0, 1, 1, 1] box the reader prepends are what the dataset drops again (features[1:], num_boxes - 1).
    The 5-column boxes are computed once, here (reader_boxes)."""
    feats = [np.asarray(it["features"]).reshape(-1, 2048) for it in items]
    boxes = [reader_boxes(it["boxes"], it["image_w"], it["image_h"]) for it in items]
    return build_group_from_rows(feats, boxes, dtype=dtype, extra=extra)


def _check_group(name, g):
    for k in ("rows", "box_rows", "row_off"):
        if k not in g or not torch.is_tensor(g[k]):
            raise ValueError("store: the %s group lacks %s" % (name, k))
    off, R = g["row_off"], g["rows"].shape[0]
    if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 2:
        raise ValueError("store: %s row_off must be int64 [n_images + 1]" % name)
    if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()):
        raise ValueError("store: %s row_off must start at 0 and never decrease" % name)
    if int(off[-1]) != R:
        raise ValueError("store: %s row_off ends at %d but the group holds %d rows" % (name, int(off[-1]), R))
    if R == 0:
        raise ValueError("store: the %s group holds no row at all" % name)
    for k, _, _ in GROUP_ROWS[name]:
        if k in g and (g[k].dim() != 2 or g[k].shape[0] != R or g[k].shape[1] == 0):
            raise ValueError("store: %s %s is %s; expected [%d, width]" % (name, k, tuple(g[k].shape), R))
    if g["box_rows"].dtype != torch.float32 or g["box_rows"].shape[1] != 5:
        raise ValueError("store: %s box_rows must be fp32 [R, 5]" % name)
    return off.numel() - 1


def build(obj_group, ocr_group, image_tables=None, question_tables=None, image_of_question=None):
    """the store, validated on the host (ValueError): monotone row offsets that end at the row count, one image count, tables whose first dimension is
    the image / question count, image_of_question int32 [n_questions] in range.  Without image_of_question the samples are image indices and the
    question tables (if any) hold one row per image."""
    n_images = _check_group("obj", obj_group)
    if _check_group("ocr", ocr_group) != n_images:
        raise ValueError("store: the obj group holds %d images, the ocr group %d" % (n_images, ocr_group["row_off"].numel() - 1))
    image_tables, question_tables = dict(image_tables or {}), dict(question_tables or {})
    if image_of_question is not None:
        ioq = torch.as_tensor(image_of_question)
        if ioq.dim() != 1 or ioq.numel() == 0 or ioq.is_floating_point():
            raise ValueError("store: image_of_question must be an integer [n_questions] tensor")
        if int(ioq.min()) < 0 or int(ioq.max()) >= n_images:
            raise ValueError("store: image_of_question holds an image outside [0, %d)" % n_images)
        ioq = ioq.to(torch.int32).contiguous()
        n_questions = ioq.numel()
    else:
        ioq, n_questions = None, n_images
    both = set(image_tables) & set(question_tables)
    reserved = (set(image_tables) | set(question_tables)) & set(_ragged.RAGGED_KEYS)
    if both or reserved:
        raise ValueError("store: table keys %s are given twice or name a ragged tensor" % sorted(both | reserved))
    for tables, n, what in ((image_tables, n_images, "image"), (question_tables, n_questions, "question")):
        for k, t in tables.items():
            if not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] != n or t[:1].numel() == 0:
                raise ValueError("store: %s table %r must be a tensor of %d non-empty rows, got %s" % (what, k, n, tuple(t.shape) if torch.is_tensor(t) else type(t)))
    return {"obj": dict(obj_group), "ocr": dict(ocr_group), "image_tables": {k: t.contiguous() for k, t in image_tables.items()},
            "question_tables": {k: t.contiguous() for k, t in question_tables.items()}, "image_of_question": ioq, "n_images": n_images,
            "n_questions": n_questions}


def _map(s, fn):
    return {"obj": {k: fn(t) for k, t in s["obj"].items()}, "ocr": {k: fn(t) for k, t in s["ocr"].items()},
            "image_tables": {k: fn(t) for k, t in s["image_tables"].items()}, "question_tables": {k: fn(t) for k, t in s["question_tables"].items()},
            "image_of_question": None if s["image_of_question"] is None else fn(s["image_of_question"]), "n_images": s["n_images"],
            "n_questions": s["n_questions"]}


def to(s, device):
    """the store with every tensor on `device` (one copy each; the store then stays there)"""
    return _map(s, lambda t: t.to(device))


def nbytes(s):
    """bytes the store's tensors hold"""
    total = []
    _map(s, lambda t: total.append(t.numel() * t.element_size()))
    return sum(total)


def _row_parts(s, name, into):
    """[(store tensor, destination tensor)] of a group: every row key the destination holds; the store must hold it too"""
    parts = []
    for key, batch_key, _ in GROUP_ROWS[name]:
        if batch_key in into:
            if key not in s[name]:
                raise ValueError("store.gather: the destination holds %s but the store's %s group has no %s" % (batch_key, name, key))
            parts.append((s[name][key], into[batch_key]))
    if not parts or COUNT_KEYS[name] not in into:
        raise ValueError("store.gather: the destination holds no row matrix of the %s group, or lacks %s" % (name, COUNT_KEYS[name]))
    return parts


def _table_parts(s, into):
    parts = [(t, into[k], 0) for k, t in s["question_tables"].items() if torch.is_tensor(into.get(k))]
    return parts + [(t, into[k], 1) for k, t in s["image_tables"].items() if torch.is_tensor(into.get(k))]


def _check_into(parts, B, n_max, who):
    for src, dst in parts:
        if dst.shape[0] != B * n_max or dst.dtype != src.dtype or tuple(dst.shape[1:]) != tuple(src.shape[1:]):
            raise ValueError("%s: a destination is %s %s; expected [%d, %s] %s (B * max rows; the store's dtype: nothing is converted)" % (
                who, tuple(dst.shape), dst.dtype, B * n_max, ", ".join(str(d) for d in src.shape[1:]), src.dtype))


def gather(s, sample_idx, into, max_obj_num=100, max_ocr_num=50, check=False, status=None):
    """write the batch of sample_idx (int32 [B] on the store's device: question indices, or image indices for a store without image_of_question) into
    `into`, a dict of device tensors with the shapes of a collate_ragged batch (for instance Trainer.input_buffers()): the row matrices and counts of
    both groups and every table key `into` holds.  Three launches; rows past the total keep what they held (ragged.upload's contract).
    -> (into, status int32 [B]): bit 1 = index or image out of range (count 0 / zero rows), bit 2 = a row range outside the store (cut).  status=:
    a resident int32 [B] tensor the bits are OR-ed into instead of a fresh zero tensor.  check=True reads the status back and raises ValueError naming
    the first flagged sample; with check=False nothing synchronises."""
    from . import ops
    if not torch.is_tensor(sample_idx) or sample_idx.dtype != torch.int32 or sample_idx.dim() != 1 or sample_idx.numel() == 0:
        raise ValueError("store.gather: sample_idx must be a non-empty int32 [B] tensor")
    B = sample_idx.numel()
    if status is None:
        status = torch.zeros(B, dtype=torch.int32, device=sample_idx.device)
    for name, n_max in (("obj", int(max_obj_num)), ("ocr", int(max_ocr_num))):
        parts = _row_parts(s, name, into)
        _check_into(parts, B, n_max, "store.gather")
        ops.store_gather_ragged(sample_idx, s["image_of_question"], s[name]["row_off"], n_max, parts, into[COUNT_KEYS[name]], status)
    tables = _table_parts(s, into)
    for src, dst, _ in tables:
        if dst.shape[0] != B or dst.dtype != src.dtype or tuple(dst.shape[1:]) != tuple(src.shape[1:]):
            raise ValueError("store.gather: a table's destination is %s %s; expected [%d, %s] %s" % (tuple(dst.shape), dst.dtype, B,
                                                                                                  ", ".join(str(d) for d in src.shape[1:]), src.dtype))
    for at in range(0, len(tables), MAX_PARTS):
        ops.store_gather_fixed(sample_idx, s["image_of_question"], s["n_images"], tables[at: at + MAX_PARTS], status)
    if check:
        _raise_flagged(status)
    return into, status


def _raise_flagged(status):
    flagged = status.tolist()
    for b, f in enumerate(flagged):
        if f:
            raise ValueError("store.gather: sample %d is flagged (status %d: %s)" % (b, f, " + ".join(
                w for bit, w in ((BAD_INDEX, "index or image out of range"), (BAD_RANGE, "row range outside the store")) if f & bit)))


def _resolve(row_off, img, n_max, total):
    """the kernel's resolve_rows on Python integers: (lo, cnt, flags) with [lo, lo + cnt) inside [0, total]"""
    lo, hi = int(row_off[img]), int(row_off[img + 1])
    cnt = min(max(hi - lo, 0), n_max)
    if cnt == 0:
        return 0, 0, 0
    if lo > total:
        return 0, 0, BAD_RANGE
    if lo < 0:
        return 0, max(min(lo + cnt, total), 0), BAD_RANGE
    if cnt > total - lo:
        return lo, total - lo, BAD_RANGE
    return lo, cnt, 0


def gather_host(s, sample_idx, into=None, max_obj_num=100, max_ocr_num=50, check=False, status=None):
    """the host twin of gather on a CPU store, bit for bit: ragged.collate_ragged of the looked-up samples (the first max rows of each image, as
    _pad_features keeps them) copied into `into` the way ragged.upload copies -- the valid prefix of every row matrix, the counts -- plus an index
    select per table.  into=None: a fresh batch whose rows past the total are zero, with every row matrix and table the store holds."""
    idx = [int(q) for q in torch.as_tensor(sample_idx).tolist()]
    if not idx:
        raise ValueError("store.gather_host: sample_idx must not be empty")
    B, ioq = len(idx), s["image_of_question"]
    n_max = {"obj": int(max_obj_num), "ocr": int(max_ocr_num)}
    status = torch.zeros(B, dtype=torch.int32) if status is None else status
    q_ok = [0 <= q < s["n_questions"] for q in idx]
    imgs = [(int(ioq[q]) if ioq is not None else q) if ok else -1 for q, ok in zip(idx, q_ok)]
    imgs = [g if 0 <= g < s["n_images"] else -1 for g in imgs]
    samples = [{} for _ in idx]
    for b, g in enumerate(imgs):
        if g < 0:
            status[b] |= BAD_INDEX
        for name, rows in GROUP_ROWS.items():
            grp = s[name]
            lo, cnt, flags = _resolve(grp["row_off"], g, n_max[name], grp["rows"].shape[0]) if g >= 0 else (0, 0, 0)
            status[b] |= flags
            for key, _, sample_key in rows:               # (a row matrix the store lacks: a one-column placeholder, dropped again below)
                samples[b][sample_key] = grp[key][lo: lo + cnt] if key in grp else torch.zeros((cnt, 1), dtype=grp["rows"].dtype)
    dtypes = {s["obj"]["rows"].dtype, s["ocr"]["rows"].dtype}
    if len(dtypes) != 1:
        raise ValueError("store.gather_host: the two groups' rows must share a dtype (collate_ragged writes one feature_dtype)")
    host = _ragged.collate_ragged(samples, max_obj_num=n_max["obj"], max_ocr_num=n_max["ocr"], feature_dtype=dtypes.pop())
    for name, rows in GROUP_ROWS.items():
        for key, batch_key, _ in rows:
            if key not in s[name]:
                del host[batch_key]
    for tables, rows in ((s["question_tables"], [q if ok else -1 for q, ok in zip(idx, q_ok)]), (s["image_tables"], imgs)):
        pick = torch.tensor([max(r, 0) for r in rows], dtype=torch.int64)
        zero = torch.tensor([r < 0 for r in rows])
        for k, t in tables.items():
            sel = t.index_select(0, pick)
            sel[zero] = 0
            host[k] = sel
    if into is None:
        into = {k: (torch.zeros_like(v) if k in _ragged.RAGGED_KEYS else v) for k, v in host.items()}
    for name, rows in GROUP_ROWS.items():
        total = int(host[COUNT_KEYS[name]].sum())
        held = [(host[bk], into[bk]) for _, bk, _ in rows if bk in host and bk in into]
        if [bk for _, bk, _ in rows if bk in into and bk not in host]:
            raise ValueError("store.gather: the destination holds a row matrix of the %s group the store lacks" % name)
        _check_into(held, B, n_max[name], "store.gather_host")
        for src, dst in held:
            dst[:total].copy_(src[:total])
        into[COUNT_KEYS[name]].copy_(host[COUNT_KEYS[name]])
    for k in list(s["question_tables"]) + list(s["image_tables"]):
        if torch.is_tensor(into.get(k)) and into[k] is not host[k]:
            into[k].copy_(host[k])
    if check:
        _raise_flagged(status)
    return into, status
