"""The batch's raw strings to cleaned code-point tensors on the GPU (csrc/textprep.hip, include/sam_hip_textprep.h).

The reference cleans every OCR token and every answer with Processors.word_cleaner (sam/datasets/processors.py:746-755: lower, delete "," and "?",
"'s" -> " 's", strip) and the host packers (phoc.pack_ocr_text, answers.pack_answer_text) then fill zero-padded int32 arrays one character at a time.
Here the batch ships the strings as they sit in the imdb, as UTF-8 bytes with offsets:

    ocr_raw uint8 [nbytes]      ocr_raw_off int32 [B * No + 1]      ocr_count int32 [B]
    answer_raw uint8 [nbytes]   answer_raw_off int32 [B * A + 1]

and materialize() writes ocr_text / ocr_text_len and answer_text / answer_text_len on the GPU, one launch each, in exactly the layout the text kernels
read (PHOC, FastText, the answer and score tables).  It runs in front of answers.tables_from_text, metrics.score_tables_from_text, the model and the
trainer, which are unchanged; it is neither a node of the captured step nor a call inside Trainer.step / SAM4C.forward.

Who lowers what.  Without a Unicode table sam_text_from_utf8 lowers ASCII only, and pack_utf8 lowers a string that is not ASCII with str.lower()
before encoding it, so for every str s

    word_cleaner(s) == clean(utf8(s if s.isascii() else s.lower()), mode 15)

(on an ASCII string the device's lowering is str.lower(); on any other string the host has run word_cleaner's first statement and the device's
lowering finds nothing left to do).  With a table resident on the device (unicode_table.build / to) the strings ship as they are,
pack_utf8(host_lower=False), and sam_text_from_utf8_unicode lowers them as str.lower() does, U+0130 and the final sigma included:

    word_cleaner(s) == clean(utf8(s), mode 15, table)

and materialize(unicode=table) also turns question_raw / question_raw_off (wordpiece.pack_question_utf8) into question_text / question_text_len as
wordpiece.pack_question_text packs them, so no string of a sample is lowered or normalised on the host."""
import numpy as np
import torch

from . import batchtext as BT
from . import unicode_table as _unicode
from .wordindex import WHITESPACE    # the code points str.strip() removes; tests/golden/textprep.json pins the list as the generator enumerated it

LOWER, DELETE, POSSESSIVE, STRIP = 1, 2, 4, 8
WORD_CLEANER = LOWER | DELETE | POSSESSIVE | STRIP          # Processors.word_cleaner
WORD_CLEANER_LOWER = LOWER | STRIP                          # Processors.word_cleaner_lower
VERBATIM = 0                                                # the reference's clean_answers = False
MAX_CHARS = 128
STATUS_UTF8, STATUS_LONG, STATUS_OFFSETS = 1, 2, 4
STATUS_REASONS = ((STATUS_UTF8, "is not strict UTF-8"), (STATUS_LONG, "has more than L = %(L)d code points after cleaning"),
                  (STATUS_OFFSETS, "has offsets outside 0 <= raw_off[s] <= raw_off[s + 1] <= nbytes"))
OCR_RAW_KEYS = ("ocr_raw", "ocr_raw_off")
ANSWER_RAW_KEYS = ("answer_raw", "answer_raw_off")
QUESTION_RAW_KEYS = ("question_raw", "question_raw_off")


def pack_utf8(strings_per_sample, slots_per_sample, pin_memory=False, lower=True, host_lower=True):
    """list (one entry per sample) of lists of str -> {"raw": uint8 [nbytes], "raw_off": int32 [B * slots + 1], "count": int32 [B]} on the CPU.  A sample
    keeps its first slots_per_sample strings; the rest of its slots are empty; count = min(len, slots).  No per-character Python: str.encode, b"".join,
    numpy.frombuffer and a cumulative sum of the encoded lengths.  lower: the target mode has the LOWER bit, so a string that is not ASCII is lowered
    here with str.lower() (module docstring); pass False for mode 0.  host_lower=False ships every string as it is: the device lowers it from a Unicode
    table (text_from_utf8(unicode=...)).  A str holding a lone surrogate cannot be encoded: UnicodeEncodeError."""
    lower = lower and host_lower
    B, N = len(strings_per_sample), int(slots_per_sample)
    if B == 0:
        raise ValueError("pack_utf8: no samples")
    if N < 1:
        raise ValueError("pack_utf8: slots_per_sample = %d must be at least 1" % N)
    enc, counts = [], []
    for strings in strings_per_sample:
        strings = list(strings)[:N]
        counts.append(len(strings))
        enc.extend((s if (not lower or s.isascii()) else s.lower()).encode("utf-8") for s in strings)
        enc.extend([b""] * (N - len(strings)))
    off = np.zeros(B * N + 1, np.int64)
    np.cumsum(np.fromiter(map(len, enc), np.int64, count=B * N), out=off[1:])
    if off[-1] >= 1 << 31:
        raise ValueError("pack_utf8: %d bytes of text exceed the int32 offsets" % off[-1])
    out = {"raw": torch.from_numpy(np.frombuffer(b"".join(enc), np.uint8).copy()), "raw_off": torch.from_numpy(off.astype(np.int32)),
           "count": torch.tensor(counts, dtype=torch.int32)}
    return BT.pinned(out, pin_memory)


def _decode(b):
    """strict UTF-8, from the definition (Unicode table 3-7): bytes -> list of code points, or None where bytes.decode("utf-8") raises"""
    out, i, n = [], 0, len(b)
    while i < n:
        b0 = b[i]
        if b0 < 0x80:
            out.append(b0)
            i += 1
            continue
        if b0 < 0xC2 or b0 > 0xF4:                  # a continuation byte no lead asked for; C0 C1 overlong; F5.. above U+10FFFF
            return None
        tail = 1 if b0 < 0xE0 else (2 if b0 < 0xF0 else 3)
        if i + tail >= n:                           # the slot ends inside the sequence
            return None
        lo1 = 0xA0 if b0 == 0xE0 else (0x90 if b0 == 0xF0 else 0x80)
        hi1 = 0x9F if b0 == 0xED else (0x8F if b0 == 0xF4 else 0xBF)
        if not lo1 <= b[i + 1] <= hi1:
            return None
        v = (b0 & (0x1F, 0x0F, 0x07)[tail - 1]) << 6 | (b[i + 1] & 0x3F)
        for k in range(2, tail + 1):
            if b[i + k] & 0xC0 != 0x80:
                return None
            v = v << 6 | (b[i + k] & 0x3F)
        out.append(v)
        i += tail + 1
    return out


def _clean(cp, mode):
    """the four passes of the header on a list of code points, in order"""
    if mode & LOWER:
        cp = [c + 32 if 0x41 <= c <= 0x5A else c for c in cp]
    if mode & DELETE:
        cp = [c for c in cp if c not in (0x2C, 0x3F)]
    if mode & POSSESSIVE:
        out = []
        for i, c in enumerate(cp):
            if c == 0x27 and i + 1 < len(cp) and cp[i + 1] == 0x73:
                out.append(0x20)
            out.append(c)
        cp = out
    if mode & STRIP:
        lo, hi = 0, len(cp)
        while lo < hi and cp[lo] in WHITESPACE:
            lo += 1
        while hi > lo and cp[hi - 1] in WHITESPACE:
            hi -= 1
        cp = cp[lo:hi]
    return cp


def clean_host(raw, raw_off, L, mode, table=None):
    """host twin of sam_text_from_utf8, written from the header's definition: raw uint8 [nbytes], raw_off int32 [S + 1] (tensors or arrays) ->
    (text int32 [S, L], text_len int32 [S], status int32 [S]) as numpy arrays.  table: a unicode_table.build() table -- the twin of
    sam_text_from_utf8_unicode then: bit 1 of mode is unicode_table.lower_host of the whole slot, in front of the other three passes."""
    raw, off = BT.to_numpy(raw).astype(np.uint8, copy=False), BT.to_numpy(raw_off).astype(np.int64)
    L, mode, S, nbytes = int(L), int(mode), len(off) - 1, raw.size
    if S < 1 or not 1 <= L <= MAX_CHARS or not 0 <= mode <= 15:
        raise ValueError("clean_host: S = %d, L = %d, mode = %d" % (S, L, mode))
    text, ln, status = np.zeros((S, L), np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    data = raw.tobytes()
    for s in range(S):
        lo, hi = int(off[s]), int(off[s + 1])
        if lo < 0 or hi < lo or hi > nbytes:
            status[s] = STATUS_OFFSETS
            continue
        cp = _decode(data[lo:hi])
        if cp is None:
            status[s] = STATUS_UTF8
            continue
        if table is not None and mode & LOWER:
            cp = _clean(_unicode.lower_host(cp, table), mode & ~LOWER)
        else:
            cp = _clean(cp, mode)
        if len(cp) > L:
            status[s] = STATUS_LONG
            continue
        text[s, :len(cp)] = cp
        ln[s] = len(cp)
    return text, ln, status


def status_message(status, L, what="slot"):
    """the first flagged slot of a status vector (host list) and its bit, or None"""
    hit = BT.first_flagged(status, STATUS_REASONS, L=L)
    return hit and "%s %d %s (status bit %d)" % (what, hit[0], hit[2], hit[1])


def text_from_utf8(raw, raw_off, L, mode, out=None, check=True, unicode=None):
    """the launch: raw uint8 [nbytes] / raw_off int32 [S + 1] on the GPU -> (text int32 [S, L], text_len int32 [S]).  out: a dict with "text", "text_len"
    and "status" to write into (every element is written).  check=True reads status back and raises ValueError naming the first flagged slot and its
    bit; check=False never synchronises and returns (text, text_len, status): a flagged slot has an all-zero row and length 0.  unicode: a Unicode table
    on the GPU (unicode_table.to(unicode_table.build(), device)): bit 1 of mode is str.lower() of the whole slot then (sam_text_from_utf8_unicode)."""
    from . import ops
    out = ops.text_from_utf8(raw, raw_off, L, mode, out=out, unicode=unicode)
    if not check:
        return out["text"], out["text_len"], out["status"]
    msg = status_message(out["status"].tolist(), int(L))
    if msg is not None:
        raise ValueError("text_from_utf8: " + msg)
    return out["text"], out["text_len"]


def has_raw(batch_dict):
    return any(k in batch_dict for k in OCR_RAW_KEYS + ANSWER_RAW_KEYS + QUESTION_RAW_KEYS)


def check_question_raw(batch_dict, unicode):
    """a batch opts in with BOTH raw question keys, none of question_text / question_text_len / question_indices / question_mask, and a Unicode table to
    normalise from.  -> whether it opted in"""
    if not BT.check(BT.QUESTION_RAW, batch_dict):
        return False
    if unicode is None:
        raise ValueError("batch carries question_raw / question_raw_off: materialize needs unicode=<a table of unicode_table.build() on the GPU> to normalise them")
    return True


def check_raw(batch_dict):
    """a batch opts in per group with BOTH raw keys and neither text key of that group; the OCR group also needs ocr_count.  -> (ocr, answers) opted in"""
    for group in (BT.OCR_RAW, BT.ANSWER_RAW):               # each group's own keys and what excludes them first, then what either needs
        BT.check(group, batch_dict, kinds=("not",))
    return tuple(BT.check(group, batch_dict, kinds=("need", "any")) for group in (BT.OCR_RAW, BT.ANSWER_RAW))


def materialize(batch_dict, ocr_chars=64, answer_chars=128, clean_answers=True, check=True, unicode=None, question_chars=256):
    """replace the raw keys of batch_dict (on the GPU) by ocr_text / ocr_text_len [B, No, Lw = ocr_chars] and answer_text / answer_text_len
    [B, A, La = answer_chars], in place, one launch per group: OCR tokens through word_cleaner, answers through word_cleaner too, or verbatim with
    clean_answers=False (then pack them with pack_utf8(lower=False)).  ocr_count stays when the batch is ragged (it counts the OCR rows) and is removed
    otherwise (a padded batch has pad_ocr_mask).  A batch without raw keys is returned as it is.  Raw keys next to the corresponding text keys, or
    one raw key without the other: ValueError.  check=True reads the status words back and raises ValueError naming the first flagged slot; check=False
    never synchronises and returns (batch_dict, {"ocr": status, "answer": status}) with the status tensors of the groups it wrote.
    unicode: a Unicode table on the GPU.  The two groups are then lowered on the device as str.lower() lowers (pack them with host_lower=False, or not:
    lowering twice changes nothing), and question_raw / question_raw_off (wordpiece.pack_question_utf8) become question_text [B, question_chars] /
    question_text_len, one more launch, with status["question"].  Raw question keys without a table, or next to the question's text or ids: ValueError."""
    ocr, ans = check_raw(batch_dict)
    status = {}
    if check_question_raw(batch_dict, unicode):
        from . import wordpiece as _wordpiece
        text, ln, status["question"] = _wordpiece.question_text_from_utf8(batch_dict["question_raw"], batch_dict["question_raw_off"], unicode, max_chars=question_chars,
                                                                          check=False)
        batch_dict["question_text"], batch_dict["question_text_len"] = text, ln
        del batch_dict["question_raw"], batch_dict["question_raw_off"]
    if ocr or ans:
        B = batch_dict["ocr_count"].numel() if "ocr_count" in batch_dict else batch_dict["ocr_text"].shape[0]
        for name, on, L, mode in (("ocr", ocr, ocr_chars, WORD_CLEANER), ("answer", ans, answer_chars, WORD_CLEANER if clean_answers else VERBATIM)):
            if not on:
                continue
            raw, off = batch_dict[name + "_raw"], batch_dict[name + "_raw_off"]
            S = off.numel() - 1
            if B < 1 or S < B or S % B:
                raise ValueError("%s_raw_off holds %d slots for B = %d samples" % (name, S, B))
            text, ln, st = text_from_utf8(raw, off, L, mode, check=False, unicode=unicode)
            batch_dict[name + "_text"], batch_dict[name + "_text_len"], status[name] = text.view(B, S // B, int(L)), ln.view(B, S // B), st
            del batch_dict[name + "_raw"], batch_dict[name + "_raw_off"]
        if ocr and "obj_count" not in batch_dict:
            del batch_dict["ocr_count"]
    if check:
        for name, st in status.items():
            if name == "question":
                from . import wordpiece as _wordpiece
                msg = _wordpiece.question_status_message(st.tolist(), int(question_chars))
            else:
                msg = status_message(st.tolist(), int(ocr_chars if name == "ocr" else answer_chars), what=name + " slot")
            if msg is not None:
                raise ValueError("materialize: " + msg)
    return batch_dict if check else (batch_dict, status)
