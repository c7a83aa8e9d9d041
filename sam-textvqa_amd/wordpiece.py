"""BERT WordPiece ids of the questions from their text.

The reference's BertTokenizerProcessor (sam/datasets/processors.py:467-498) calls BertTokenizer.encode(question, add_special_tokens=True) of an uncased model
on the host, cuts the ids to max_length = 20 and pads with [PAD] = 0: question_indices / question_mask int64 [B, 20].  A batch may carry the question's code
points instead,

    question_text int32 [B, Lq]     question_text_len int32 [B]

and NO question_indices / question_mask: one launch (ops.wordpiece_from_text, csrc/wordpiece.hip) then writes the reference's tensors, inside SAM4C.forward
(set_question_vocab gives the model the vocabulary index) or through from_text here.  The work is split where Unicode tables are needed:

  pack_question_text   an ASCII question is packed raw.  A non-ASCII one first gets BasicTokenizer's table-driven steps: control characters dropped, Unicode
                       spaces mapped to U+0020, blanks around CJK ideographs, per word str.lower() and THEN NFD without combining marks (the order of the
                       reference's pytorch_transformers; later libraries strip first), and bit 30 on every non-ASCII punctuation character.
  the kernel           everything else, on code points: ASCII control characters, blanks, lower case and punctuation, the 100-character rule, greedy
                       longest-match WordPiece against the vocabulary index, [CLS] / [SEP], the cut to T (include/sam_hip_question.h states the rules).

With a Unicode table resident on the device (unicode_table.py) the packer's half runs there too: pack_question_utf8 ships the
questions as raw UTF-8 bytes and question_text_from_utf8 (sam_question_from_utf8, csrc/unicode_text.hip) writes what pack_question_text writes, bit for
bit; question_text_host is its twin.

encode_host is the kernel's host twin on the packed tensors.  Deviation from the library: the five special-token strings ([PAD] [UNK] [CLS] [SEP] [MASK])
written literally in a question are kept whole by the library and would be split at the brackets here -- pack_question_text refuses such a question."""
import unicodedata

import numpy as np
import torch

from . import batchtext as BT
from .wordindex import build_slots, table_size

QUESTION_TEXT_KEYS = ("question_text", "question_text_len")
QUESTION_KEYS = ("question_indices", "question_mask", "num_question_tokens")          # what the launch writes
MARKER = "_sam_question_from_text"                                                     # SAM4C.forward sets it beside the tensors it materialised
PAD_TOKEN, UNK_TOKEN, CLS_TOKEN, SEP_TOKEN, MASK_TOKEN = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
SPECIAL_TOKENS = (PAD_TOKEN, UNK_TOKEN, CLS_TOKEN, SEP_TOKEN, MASK_TOKEN)
MAX_QUESTION_CHARS = 1024          # the kernel's LDS staging
MAX_PIECE_CHARS = 64               # one candidate per lane
MAX_TOKENS = 64                    # one output column per lane
MAX_WORD_CHARS = 100               # WordpieceTokenizer.max_input_chars_per_word
PUNCT_FLAG = 1 << 30               # on a packed code point: "a punctuation character" (set by the packer for non-ASCII ones only)
_CP_MASK = PUNCT_FLAG - 1
_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
_WORD, _SINGLE, _SEP, _DROP = range(4)


def is_cjk(cp):
    """BertTokenizer's _is_chinese_char"""
    return any(lo <= cp <= hi for lo, hi in _CJK)


def normalize(question):
    """the table-driven half of BasicTokenizer(do_lower_case=True) for a non-ASCII question, up to but not including the split at punctuation: _clean_text,
    _tokenize_chinese_chars, whitespace_tokenize, and per word lower() then _run_strip_accents; the words joined with single blanks"""
    out = []
    for ch in question:
        cp = ord(ch)
        if ch in "\t\n\r":
            out.append(" ")
            continue
        cat = unicodedata.category(ch)
        if cp == 0 or cp == 0xFFFD or cat.startswith("C"):
            continue
        if cat == "Zs":
            out.append(" ")
        elif is_cjk(cp):
            out.extend((" ", ch, " "))
        else:
            out.append(ch)
    words = ("".join(c for c in unicodedata.normalize("NFD", w.lower()) if unicodedata.category(c) != "Mn") for w in "".join(out).split())
    return " ".join(w for w in words if w)


def pack_question_text(questions, max_chars=256, pin_memory=False):
    """list of str -> {"question_text": int32 [B, Lq], "question_text_len": int32 [B]} on the CPU, Lq = max_chars (1..1024).  An ASCII question is packed
    as it is; a non-ASCII one as normalize() leaves it, with PUNCT_FLAG on every code point >= 128 of a category P*.  ValueError naming the sample: a
    (normalised) question of more than max_chars code points -- nothing is truncated --, and a question that holds one of SPECIAL_TOKENS literally."""
    B, Lq = len(questions), int(max_chars)
    if B == 0:
        raise ValueError("pack_question_text: no samples")
    if not 1 <= Lq <= MAX_QUESTION_CHARS:
        raise ValueError("pack_question_text: max_chars = %d must be in [1, %d]" % (Lq, MAX_QUESTION_CHARS))

    def rows():
        for b, q in enumerate(questions):
            if not isinstance(q, str):
                raise ValueError("sample %d: the question must be a str, got %s" % (b, type(q).__name__))
            for tok in SPECIAL_TOKENS:
                if tok in q:
                    raise ValueError("sample %d: the question holds the special token %s literally; the tokenizer library keeps it whole, this path would split it: "
                                     "not supported" % (b, tok))
            yield b, q if q.isascii() else [ord(c) | (PUNCT_FLAG if ord(c) >= 128 and unicodedata.category(c).startswith("P") else 0) for c in normalize(q)]

    text, ln = BT.pack_rows((B, Lq), rows(), Lq, lambda b, q, n: "sample %d: the question has %d code points%s, over max_chars = %d" % (
        b, n, "" if isinstance(q, str) else " after normalisation", Lq))
    return BT.pinned({"question_text": torch.from_numpy(text), "question_text_len": torch.from_numpy(ln)}, pin_memory)


QUESTION_STATUS_REASONS = ((1, "is not strict UTF-8"), (2, "has more than max_chars = %(L)d code points after normalisation"),
                           (4, "has offsets outside 0 <= raw_off[b] <= raw_off[b + 1] <= nbytes"),
                           (8, "holds a special token ([PAD] [UNK] [CLS] [SEP] [MASK]) literally; the tokenizer library keeps it whole, this path would split it"),
                           (16, "holds a code point canonical reordering can move; normalise this question on the host (pack_question_text)"))


def pack_question_utf8(questions, pin_memory=False):
    """list of str -> {"question_raw": uint8 [nbytes], "question_raw_off": int32 [B + 1]} on the CPU: the questions as they are, as UTF-8 bytes back to
    back (textprep.pack_utf8 with one slot per sample and nothing lowered).  No per-character Python; everything pack_question_text refuses is reported
    by the launch's status instead."""
    for b, q in enumerate(questions):
        if not isinstance(q, str):
            raise ValueError("sample %d: the question must be a str, got %s" % (b, type(q).__name__))
    from . import textprep
    p = textprep.pack_utf8([[q] for q in questions], 1, pin_memory=pin_memory, host_lower=False)
    return {"question_raw": p["raw"], "question_raw_off": p["raw_off"]}


def question_status_message(status, max_chars):
    """the first flagged question of a status vector (host list) and its bit, or None"""
    hit = BT.first_flagged(status, QUESTION_STATUS_REASONS, L=max_chars)
    return hit and "sample %d: the question %s (status bit %d)" % (hit[0], hit[2], hit[1])


def question_text_host(raw, raw_off, table, max_chars=256):
    """host twin of sam_question_from_utf8 (include/sam_hip_unicode.h): raw uint8 [nbytes], raw_off int32 [B + 1] (tensors or arrays), table a
    unicode_table.build() table -> (question_text int32 [B, Lq], question_text_len int32 [B], status int32 [B]) as numpy arrays.  The first status
    that applies, in the order 4, 1, 8, 16, 2."""
    from . import textprep, unicode_table
    raw, off = BT.to_numpy(raw).astype(np.uint8, copy=False), BT.to_numpy(raw_off).astype(np.int64)
    Lq, B, nbytes = int(max_chars), len(off) - 1, raw.size
    if B < 1 or not 1 <= Lq <= MAX_QUESTION_CHARS:
        raise ValueError("question_text_host: B = %d, max_chars = %d must be in [1, %d]" % (B, Lq, MAX_QUESTION_CHARS))
    text, ln, status = np.zeros((B, Lq), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    data = raw.tobytes()
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if lo < 0 or hi < lo or hi > nbytes:
            status[b] = 4
            continue
        cps = textprep._decode(data[lo:hi])
        if cps is None:
            status[b] = 1
            continue
        if any(tok.encode() in data[lo:hi] for tok in SPECIAL_TOKENS):
            status[b] = 8
            continue
        if hi - lo != len(cps):                    # not ASCII
            cps = unicode_table.normalize_host(cps, table)
            if cps is None:
                status[b] = 16
                continue
        if len(cps) > Lq:
            status[b] = 2
            continue
        text[b, :len(cps)] = cps
        ln[b] = len(cps)
    return text, ln, status


def question_text_from_utf8(raw, raw_off, table, max_chars=256, check=True):
    """the launch: raw uint8 [nbytes] / raw_off int32 [B + 1] (pack_question_utf8) and a Unicode table, all on the GPU -> (question_text int32 [B, max_chars],
    question_text_len int32 [B]), bit for bit pack_question_text's.  check=True reads the status back and raises ValueError naming the first flagged
    sample and its bit; check=False never synchronises and returns (question_text, question_text_len, status): a flagged question has an all-zero row
    and length 0."""
    from . import ops
    if not 1 <= int(max_chars) <= MAX_QUESTION_CHARS:
        raise ValueError("question_text_from_utf8: max_chars = %d must be in [1, %d]" % (int(max_chars), MAX_QUESTION_CHARS))
    out = ops.question_from_utf8(raw, raw_off, int(max_chars), table)
    if not check:
        return out["question_text"], out["question_text_len"], out["status"]
    msg = question_status_message(out["status"].tolist(), int(max_chars))
    if msg is not None:
        raise ValueError("question_text_from_utf8: " + msg)
    return out["question_text"], out["question_text_len"]


def vocab_index(words, max_piece=32):
    """the lines of a BERT vocab.txt, in id order, as the kernel reads them -- the three tensors and the probe of answers.vocab_index: {"cp": int32 [V, Lv]
    exact code points (continuation pieces WITH their "##": a word-initial candidate never holds '#' next to another character, '#' being punctuation, so
    nothing is ambiguous), "len": int32 [V], "slots": int32 [T] (wordindex.build_slots: T the smallest power of two >= 2 V, -1 = empty, home slot
    wordindex.text_hash & (T - 1), linear probing, a contested slot goes to the lowest id), "V", "PAD", "UNK", "CLS", "SEP"} -- CPU tensors and ints; answers.index_to(index, device) moves the tensors.
    ValueError: a special token missing, [PAD] not id 0 (the reference asserts it), an entry listed twice, an entry of more than max_piece (<= 64) code points."""
    words = [w.rstrip("\n") for w in words]
    V, Lv = len(words), int(max_piece)
    if not 1 <= Lv <= MAX_PIECE_CHARS:
        raise ValueError("vocab_index: max_piece = %d must be in [1, %d]" % (Lv, MAX_PIECE_CHARS))
    ids = {}
    for i, w in enumerate(words):
        if w in ids:
            raise ValueError("vocab_index: entry %d (%r) is listed twice (first as %d)" % (i, w, ids[w]))
        ids[w] = i
    for tok in (PAD_TOKEN, UNK_TOKEN, CLS_TOKEN, SEP_TOKEN):
        if tok not in ids:
            raise ValueError("vocab_index: the vocabulary has no %s" % tok)
    if ids[PAD_TOKEN] != 0:
        raise ValueError("vocab_index: %s must be id 0 (it is %d)" % (PAD_TOKEN, ids[PAD_TOKEN]))
    cp, ln = BT.pack_rows((V, Lv), enumerate(words), Lv, lambda i, w, n: "vocab_index: entry %d (%r) has %d code points, over max_piece = %d" % (i, w, n, Lv))
    slots = build_slots(cp, ln, np.arange(V), table_size(V))
    return {"cp": torch.from_numpy(cp), "len": torch.from_numpy(ln), "slots": torch.from_numpy(slots), "V": V, "PAD": 0, "UNK": ids[UNK_TOKEN],
            "CLS": ids[CLS_TOKEN], "SEP": ids[SEP_TOKEN]}


def is_vocab_index(v):
    return isinstance(v, dict) and all(k in v for k in ("cp", "len", "slots", "V", "PAD", "UNK", "CLS", "SEP"))


def _classify(c, flagged):
    """(class, folded code point) of a masked code point: the kernel's classify"""
    if c >= 128:
        return (_SINGLE if flagged or is_cjk(c) else _WORD), c
    if c in (0x20, 0x09, 0x0A, 0x0D):
        return _SEP, c
    if c < 0x20 or c == 0x7F:
        return _DROP, c
    if 0x41 <= c <= 0x5A:
        return _WORD, c + 0x20
    if 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126:
        return _SINGLE, c
    return _WORD, c


def split_words(code_points):
    """packed code points (flag bits on) -> the words the kernel walks, each a list of folded code points"""
    words, cur = [], []
    for v in code_points:
        v = int(v) & 0xFFFFFFFF
        kind, c = _classify(v & _CP_MASK, bool(v & PUNCT_FLAG))
        if kind == _DROP:
            continue
        if kind == _WORD:
            cur.append(c)
            continue
        if cur:
            words.append(cur)
            cur = []
        if kind == _SINGLE:
            words.append([c])
    if cur:
        words.append(cur)
    return words


def _piece_table(index):
    cp, ln = index["cp"].cpu().numpy(), index["len"].cpu().numpy()
    return {tuple(cp[i, :ln[i]].tolist()): i for i in range(cp.shape[0])}


def word_pieces(word, table, Lv, unk):
    """WordpieceTokenizer.tokenize of one word (folded code points) -> ids: greedy longest match from the left, "##" in front of a continuation, candidates
    of more than Lv code points cannot match; a word of more than 100 code points, or with a position nothing matches, is the single id unk"""
    L = len(word)
    if L > MAX_WORD_CHARS:
        return [unk]
    out, s = [], 0
    while s < L:
        pre = (35, 35) if s > 0 else ()
        top = min(L, s + Lv - len(pre))
        for end in range(top, s, -1):
            i = table.get(pre + tuple(word[s:end]))
            if i is not None:
                out.append(i)
                s = end
                break
        else:
            return [unk]
    return out


def encode_host(question_text, question_text_len, index, T=20):
    """host twin of sam_wordpiece_from_text on the packed tensors -> {"question_indices": int64 [B, T], "question_mask": int64 [B, T],
    "num_question_tokens": int32 [B]} on the CPU: [CLS], the ids, [SEP], cut to T; [PAD] = 0 and mask 0 behind the count; lengths clamped to [0, Lq].
    Its lookups are exact matches in the index's word list (what the kernel's probe finds: answers.vocab_lookup_host is the probe's own twin)."""
    T = int(T)
    if not 1 <= T <= MAX_TOKENS:
        raise ValueError("encode_host: T = %d must be in [1, %d]" % (T, MAX_TOKENS))
    text, ln = BT.unpack(question_text, question_text_len)
    B = text.shape[0]
    table, Lv = _piece_table(index), index["cp"].shape[1]
    ids, mask, cnt = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64), np.zeros(B, np.int32)
    for b in range(B):
        row = [int(index["CLS"])]
        for w in split_words(text[b, :ln[b]]):
            if len(row) >= T:
                break
            row.extend(word_pieces(w, table, Lv, int(index["UNK"])))
        row = (row + [int(index["SEP"])])[:T]
        ids[b, :len(row)] = row
        mask[b, :len(row)] = 1
        cnt[b] = len(row)
    return {"question_indices": torch.from_numpy(ids), "question_mask": torch.from_numpy(mask), "num_question_tokens": torch.from_numpy(cnt)}


def encode_questions(questions, index, T=20, max_chars=256):
    """list of str -> encode_host of their packed text"""
    p = pack_question_text(questions, max_chars=max_chars)
    return encode_host(p["question_text"], p["question_text_len"], index, T)


def has_text(batch_dict):
    return BT.has_text(BT.QUESTION_TEXT, batch_dict)


def check(batch_dict):
    """a batch opts in with BOTH question-text keys and neither question_indices nor question_mask; -> whether it opted in"""
    return BT.check(BT.QUESTION_TEXT, batch_dict)


def strip_materialized(batch_dict):
    """drop what SAM4C.forward materialised from the question's text in an earlier call (the marker says so): the dict is again the batch its owner built"""
    if batch_dict.pop(MARKER, False):
        for k in QUESTION_KEYS:
            batch_dict.pop(k, None)


def outputs(B, T, device):
    """fresh output buffers of from_text"""
    return {"question_indices": torch.empty((B, T), dtype=torch.int64, device=device), "question_mask": torch.empty((B, T), dtype=torch.int64, device=device),
            "num_question_tokens": torch.empty((B,), dtype=torch.int32, device=device)}


def from_text(question_text, question_text_len, index, T=20, out=None):
    """the reference's question tensors of packed text on the GPU, one launch (csrc/wordpiece.hip): element for element encode_host.  index: vocab_index(...)
    with its tensors on the GPU (answers.index_to); out: buffers from outputs() (allocated here when None; every element is written).  Nothing is read by
    the host: capturable."""
    from . import ops
    if out is None:
        out = outputs(question_text.shape[0], int(T), question_text.device)
    ops.wordpiece_from_text(question_text.contiguous(), question_text_len.contiguous(), index, out["question_indices"], out["question_mask"], out["num_question_tokens"])
    return out
