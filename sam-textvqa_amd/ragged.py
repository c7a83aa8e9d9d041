"""Ragged region features: a batch that carries only the valid object / OCR rows, optionally as fp16, plus a row count per sample.

The reference zero-fills every sample to max_obj_num / max_ocr_num (sam/datasets/textvqa_dataset.py:285-305, _pad_features) and ships fp32: 1.41 MB per
sample at the c3 shapes, most of it padding and fp32 width.  Here the host side keeps the samples' valid rows back to back in fixed-capacity matrices
(capacity B * max rows, so the shapes -- and a captured training step -- never change) and the GPU expands them (ops.ragged_expand, csrc/ragged.hip):

    obj_rows [B * max_obj, 2048]   obj_box_rows [B * max_obj, 5]   obj_count int32 [B]
    ocr_rows [B * max_ocr, Df]     ocr_ft_rows [.., 300]   ocr_phoc_rows [.., 604]   ocr_box_rows [.., 5]   ocr_count int32 [B]

Sample b owns rows off[b] .. off[b] + count[b] - 1 of every matrix of its group, off = the exclusive prefix sum of the counts; rows past the total are
never read.  SAM4C.forward takes such a batch directly; to_padded / from_padded convert to and from the reference schema.

A batch may carry the OCR tokens' TEXT instead of ocr_phoc_rows (phoc.py): ocr_text int32 [B, max_ocr, Lw] / ocr_text_len int32
[B, max_ocr], indexed by slot (not back to back) and copied whole; the PHOC columns are then computed on the GPU.  Text next to ocr_phoc_rows is refused.
Likewise the QUESTION's text instead of question_indices / question_mask (wordpiece.py): question_text int32 [B, Lq] /
question_text_len int32 [B], one row per sample, carried by to_padded / from_padded / upload like every other non-ragged entry."""
import torch

from . import answers as _answers
from . import phoc as _phoc
from . import textprep as _textprep
from . import wordpiece as _wordpiece

OBJ_PARTS = (("obj_rows", "pad_obj_features"), ("obj_box_rows", "pad_obj_bboxes"))
OCR_PARTS = (("ocr_rows", "pad_ocr_features"), ("ocr_ft_rows", "ocr_fasttext"), ("ocr_phoc_rows", "ocr_phoc"), ("ocr_box_rows", "pad_ocr_bboxes"))
GROUPS = (("obj_count", "pad_obj_mask", OBJ_PARTS), ("ocr_count", "pad_ocr_mask", OCR_PARTS))
RAGGED_KEYS = tuple(k for cnt, _, parts in GROUPS for k in (cnt,) + tuple(r for r, _ in parts))
PADDED_KEYS = tuple(k for _, m, parts in GROUPS for k in (m,) + tuple(p for _, p in parts))
BOX_KEYS = ("obj_box_rows", "ocr_box_rows")
_SAMPLE_KEYS = {"obj_rows": "obj_features", "obj_box_rows": "obj_bboxes", "ocr_rows": "ocr_features", "ocr_ft_rows": "ocr_fasttext",
                "ocr_phoc_rows": "ocr_phoc", "ocr_box_rows": "ocr_bboxes"}


PHOC_PART = ("ocr_phoc_rows", "ocr_phoc")


def group_parts(batch_dict, parts):
    """the row matrices a batch carries for a group: without the PHOC part when it gives the tokens' text instead (packed, or raw: textprep.py)"""
    return tuple(p for p in parts if p != PHOC_PART) if (_phoc.has_text(batch_dict) or "ocr_raw" in batch_dict) else parts


def is_ragged(batch_dict):
    return "obj_count" in batch_dict or "ocr_count" in batch_dict


def check(batch_dict):
    """a ragged batch carries every ragged key (ocr_text / ocr_text_len in place of ocr_phoc_rows when it gives the tokens' text) and no padded feature tensor"""
    text = _phoc.check(batch_dict)                           # both text keys, and neither ocr_phoc_rows nor ocr_phoc next to them: ValueError
    missing = [k for k in RAGGED_KEYS if k not in batch_dict and not (text and k == PHOC_PART[0])]
    if missing:
        raise ValueError("ragged batch lacks %s" % ", ".join(missing))
    both = [k for k in ("pad_obj_features", "pad_ocr_features") if k in batch_dict]
    if both:
        raise ValueError("batch carries ragged rows (obj_count / ocr_count) and padded %s: give one form" % " / ".join(both))
    for cnt, _, parts in GROUPS:
        b = batch_dict[cnt].numel()
        rows = {batch_dict[r].shape[0] for r, _ in group_parts(batch_dict, parts)}
        if len(rows) != 1 or b == 0 or next(iter(rows)) % b or next(iter(rows)) == 0:
            raise ValueError("ragged batch: the row matrices of %s must share a capacity of B * max rows (B = %d, rows %s)" % (cnt, b, sorted(rows)))
    if text and tuple(batch_dict["ocr_text"].shape[:2]) != (batch_dict["ocr_count"].numel(), group_max(batch_dict, "ocr_count")):
        raise ValueError("ragged batch: ocr_text is %s, expected [B, max_ocr] = [%d, %d] slots" % (
            tuple(batch_dict["ocr_text"].shape), batch_dict["ocr_count"].numel(), group_max(batch_dict, "ocr_count")))


def group_max(batch_dict, count_key):
    """max rows per sample of a group: capacity / B"""
    parts = dict((c, p) for c, _, p in GROUPS)[count_key]
    return batch_dict[parts[0][0]].shape[0] // batch_dict[count_key].numel()


def collate_ragged(samples, max_obj_num=100, max_ocr_num=50, feature_dtype=torch.float16, pin_memory=False, spatial_from_boxes=False, spatial_distance_threshold=None,
                   max_chars=None, max_question_chars=None, raw_text=False, clean_answers=True, device_lower=False):
    """list of per-sample dicts of UNPADDED tensors (obj_features [n, 2048], obj_bboxes [n, 5], ocr_features [m, Df], ocr_fasttext [m, 300],
    ocr_phoc [m, 604], ocr_bboxes [m, 5]) -> the ragged CPU batch.  A sample over a maximum keeps its first `max` rows, as _pad_features does
    (min(num_boxes, max)); feature matrices are stored as feature_dtype, boxes stay fp32; rows past the total are left untouched.
    spatial_from_boxes / spatial_distance_threshold: set the batch's keys of those names (the model then derives the spatial allow bits from the boxes
    the expansion writes, and the batch ships no relation tensor); to_padded / from_padded carry them like every other non-ragged entry.
    A sample may give ocr_tokens (a list of str) instead of ocr_phoc -- every sample of the batch the same way: the batch then carries ocr_text /
    ocr_text_len (phoc.pack_ocr_text: the first max_ocr_num tokens, max_chars code points each, default the score table's width) and no ocr_phoc_rows.
    Such a sample may also give answers (its cleaned answers, a list of str) -- again the whole batch the same way: the batch then carries answer_text /
    answer_text_len (answers.pack_answer_text), from which answers.tables_from_text builds the answer table on the GPU.
    A sample may give question (a str) instead of question_indices / question_mask -- the whole batch the same way: the batch then carries question_text /
    question_text_len (wordpiece.pack_question_text, max_question_chars code points, default its own), from which SAM4C.forward writes the ids on the GPU.
    raw_text: ocr_tokens and answers are the RAW strings of the imdb, not cleaned ones, and travel as UTF-8 bytes (textprep.pack_utf8): the batch carries
    ocr_raw / ocr_raw_off and answer_raw / answer_raw_off instead of the four text keys, and textprep.materialize cleans and packs them on the GPU
    (clean_answers=False: the answers are packed for materialize(clean_answers=False)).  max_chars belongs to materialize then and is refused here.
    device_lower (with raw_text): nothing is lowered or normalised here -- the strings ship unlowered and a question ships as question_raw /
    question_raw_off (wordpiece.pack_question_utf8; max_question_chars is materialize's question_chars then and is refused here); the batch is for
    textprep.materialize(unicode=<table>), which lowers and normalises on the GPU from the resident Unicode table."""
    if device_lower and not raw_text:
        raise ValueError("collate_ragged: device_lower needs raw_text")
    if device_lower and max_question_chars is not None:
        raise ValueError("collate_ragged: with device_lower the capacity max_question_chars is textprep.materialize's question_chars")
    if not samples:
        raise ValueError("collate_ragged: no samples")
    B = len(samples)
    out = {}
    with_tokens = ["ocr_tokens" in s for s in samples]
    if raw_text and not any(with_tokens):
        raise ValueError("collate_ragged: raw_text needs ocr_tokens (and optionally answers) in every sample")
    if raw_text and max_chars is not None:
        raise ValueError("collate_ragged: with raw_text the capacity max_chars is textprep.materialize's ocr_chars")
    if any(with_tokens):
        if not all(with_tokens) or any("ocr_phoc" in s for s in samples):
            raise ValueError("collate_ragged: every sample gives either ocr_tokens or ocr_phoc, the whole batch the same way")
        if raw_text:
            packed = _textprep.pack_utf8([s["ocr_tokens"] for s in samples], max_ocr_num, pin_memory=pin_memory, host_lower=not device_lower)
            out.update(ocr_raw=packed["raw"], ocr_raw_off=packed["raw_off"])          # (ocr_count: the row count below, min(rows, max_ocr_num))
        else:
            out.update(_phoc.pack_ocr_text([s["ocr_tokens"] for s in samples], max_ocr_num, pin_memory=pin_memory,
                                           **({} if max_chars is None else {"max_chars": max_chars})))
    with_answers = ["answers" in s for s in samples]
    if any(with_answers):
        if not all(with_answers) or not all(with_tokens):
            raise ValueError("collate_ragged: every sample gives its answers (a list of str) next to ocr_tokens, the whole batch the same way, or none does")
        if raw_text:
            A = len(samples[0]["answers"])
            for b, s in enumerate(samples):
                if len(s["answers"]) != A or A < 1:
                    raise ValueError("sample %d: expected %d answers, got %d" % (b, A, len(s["answers"])))
            packed = _textprep.pack_utf8([s["answers"] for s in samples], A, pin_memory=pin_memory, lower=clean_answers, host_lower=not device_lower)
            out.update(answer_raw=packed["raw"], answer_raw_off=packed["raw_off"])
        else:
            out.update(_answers.pack_answer_text([s["answers"] for s in samples], num_answers=len(samples[0]["answers"]), pin_memory=pin_memory))
    with_question = ["question" in s for s in samples]
    if any(with_question):
        if not all(with_question) or any(k in s for s in samples for k in ("question_indices", "question_mask")):
            raise ValueError("collate_ragged: every sample gives either question (a str) or question_indices / question_mask, the whole batch the same way")
        if device_lower:
            out.update(_wordpiece.pack_question_utf8([s["question"] for s in samples], pin_memory=pin_memory))
        else:
            out.update(_wordpiece.pack_question_text([s["question"] for s in samples], pin_memory=pin_memory,
                                                     **({} if max_question_chars is None else {"max_chars": max_question_chars})))
    for cnt_key, _, parts in GROUPS:
        parts = group_parts(out, parts)
        n_max = max_obj_num if cnt_key == "obj_count" else max_ocr_num
        first = _SAMPLE_KEYS[parts[0][0]]
        counts = [min(int(s[first].shape[0]), n_max) for s in samples]
        for row_key, _ in parts:
            src = _SAMPLE_KEYS[row_key]
            width = int(samples[0][src].shape[1])
            dt = torch.float32 if row_key in BOX_KEYS else feature_dtype
            dst = torch.empty((B * n_max, width), dtype=dt, pin_memory=pin_memory)
            at = 0
            for s, c in zip(samples, counts):
                x = torch.as_tensor(s[src])
                if x.dim() != 2 or x.shape[1] != width or x.shape[0] < c:
                    raise ValueError("collate_ragged: %s of a sample is %s; expected [>= %d, %d]" % (src, tuple(x.shape), c, width))
                dst[at: at + c].copy_(x[:c])
                at += c
            out[row_key] = dst
        out[cnt_key] = torch.tensor(counts, dtype=torch.int32)
        if pin_memory:
            out[cnt_key] = out[cnt_key].pin_memory()
    if spatial_from_boxes:
        out["spatial_from_boxes"] = True
        if spatial_distance_threshold is not None:
            out["spatial_distance_threshold"] = float(spatial_distance_threshold)
    return out


def upload(host_batch, device_batch):
    """copy a collate_ragged batch into device tensors of the same shapes (for instance Trainer.input_buffers()): the valid prefix of every row matrix
    and the counts -- the host-to-device bytes are proportional to the valid rows; device rows past the total keep what they held.  Any other tensor
    the two dicts share (question_indices, ...) is copied whole.  Returns device_batch."""
    for cnt_key, _, parts in GROUPS:
        counts = host_batch[cnt_key]
        n_max = group_max(host_batch, cnt_key)
        total = int(counts.clamp(0, n_max).sum())
        for row_key, _ in group_parts(host_batch, parts):
            src, dst = host_batch[row_key], device_batch[row_key]
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("upload: %s is %s %s on the host and %s %s on the device" % (row_key, tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype))
            if total:
                dst[:total].copy_(src[:total], non_blocking=True)
        device_batch[cnt_key].copy_(counts, non_blocking=True)
    for k, v in host_batch.items():
        if k not in RAGGED_KEYS and torch.is_tensor(v) and torch.is_tensor(device_batch.get(k)):
            device_batch[k].copy_(v, non_blocking=True)
    return device_batch


def expand_rows_torch(rows, counts, n_max):
    """the torch twin of the kernel's fp32-copy form: rows [cap, D], counts [B] -> (padded fp32 [B, n_max, D], mask int64 [B, n_max]) with the kernel's
    clamps (counts into [0, n_max], source rows below cap)"""
    c = counts.long().clamp(0, n_max)
    off = torch.cumsum(c, 0) - c
    ar = torch.arange(n_max, device=rows.device)
    valid = ar[None, :] < c[:, None]
    idx = (off[:, None] + ar[None, :]).clamp(max=rows.shape[0] - 1)
    out = torch.where(valid[..., None], rows[idx].float(), torch.zeros((), dtype=torch.float32, device=rows.device))
    return out, valid.long()


def to_padded(batch_dict):
    """the reference-schema keys of a ragged batch (fp32 features and boxes, int64 masks) in a new dict next to the batch's other entries: on the GPU through
    the kernel's fp32-copy form, one launch per group; on CPU tensors through the torch twin.  A batch with the tokens' text keeps ocr_text / ocr_text_len
    (they are indexed by slot already) and gets no ocr_phoc: that is the padded form of such a batch, which SAM4C.forward takes"""
    check(batch_dict)
    out = {k: v for k, v in batch_dict.items() if k not in RAGGED_KEYS}
    for cnt_key, mask_key, parts in GROUPS:
        counts = batch_dict[cnt_key]
        B, n_max = counts.numel(), group_max(batch_dict, cnt_key)
        parts = group_parts(batch_dict, parts)
        if counts.is_cuda:
            from . import ops
            dev = counts.device
            mask = torch.empty((B, n_max), dtype=torch.int64, device=dev)
            launch = []
            for row_key, pad_key in parts:
                rows = batch_dict[row_key]
                out[pad_key] = torch.empty((B, n_max, rows.shape[1]), dtype=torch.float32, device=dev)
                launch.append((rows, out[pad_key].view(B * n_max, -1), 0, False, 0))
            ops.ragged_expand(counts.to(torch.int32).contiguous(), n_max, launch, mask=mask)
            out[mask_key] = mask
        else:
            for row_key, pad_key in parts:
                out[pad_key], out[mask_key] = expand_rows_torch(batch_dict[row_key], counts, n_max)
    return out


def from_padded(batch_dict, feature_dtype=torch.float16):
    """the inverse of to_padded (tests, synthetic batches): counts from the masks, which must be prefix masks (ValueError otherwise); feature matrices as
    feature_dtype, boxes fp32; rows past the total are zero.  Every other entry is carried over -- ocr_text / ocr_text_len among them (a batch with the
    tokens' text has no ocr_phoc and gets no ocr_phoc_rows)."""
    _phoc.check(batch_dict)
    out = {k: v for k, v in batch_dict.items() if k not in PADDED_KEYS}
    for cnt_key, mask_key, parts in GROUPS:
        parts = group_parts(batch_dict, parts)
        mask = batch_dict[mask_key].ne(0)
        B, n_max = mask.shape
        c = mask.sum(1)
        if not torch.equal(mask, torch.arange(n_max, device=mask.device)[None, :] < c[:, None]):
            raise ValueError("from_padded: %s is not a prefix mask (valid rows must come first in every sample)" % mask_key)
        for row_key, pad_key in parts:
            x = batch_dict[pad_key]
            if x.shape[:2] != mask.shape:
                raise ValueError("from_padded: %s is %s, %s is %s" % (pad_key, tuple(x.shape), mask_key, tuple(mask.shape)))
            dt = torch.float32 if row_key in BOX_KEYS else feature_dtype
            rows = torch.zeros((B * n_max, x.shape[2]), dtype=dt, device=x.device)
            valid = x[mask]                                       # sample-major, row-minor: already back to back
            rows[: valid.shape[0]] = valid.to(dt)
            out[row_key] = rows
        out[cnt_key] = c.to(torch.int32)
    return out


def materialize(batch_dict):
    """replace the ragged keys of batch_dict by their padded form, in place (what the decoding sessions read)"""
    padded = to_padded(batch_dict)
    for k in RAGGED_KEYS:
        batch_dict.pop(k, None)
    batch_dict.update(padded)
    return batch_dict
