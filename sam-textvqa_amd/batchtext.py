"""The batch's text, in its forms -- raw UTF-8 (*_raw / *_raw_off), packed code points (*_text / *_text_len), and the finished tensors (ids, PHOC, FastText,
answer table, score table) -- described once: which keys opt a batch in to a form, what may not sit beside them and what they need (the GROUPS below and
`check`), and the host-side handling every feature shares: tensor-or-array to numpy, strings into zero-padded int32 rows with a length array and back, the
pinned-memory tail, the first flagged entry of a status vector.  phoc.py, fasttext.py, wordpiece.py, answers.py, metrics.py and textprep.py keep their public
names and call these; tests/test_batchtext_cpu.py holds the groups against the modules' *_KEYS tuples and every message against
tests/golden/batch_text_rules.json.  Pure: numpy and torch, no GPU, no library."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------- helpers
def to_numpy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def code_points(s, mask=-1):
    """a str -> its code points; any other sequence of code points -> ints, each and-ed with `mask` (a packed code point's flag bits off)"""
    return [ord(c) for c in s] if isinstance(s, str) else [int(c) & mask for c in s]


def text_of(cps):
    return "".join(map(chr, cps))


def pack_rows(out, items, cap=None, over=None):
    """fill zero-padded int32 rows and their lengths.  out: the pair (text [..., W], len [...]) to write into, or the text's shape (both are allocated,
    all zero); items: (index, str or sequence of code points) -- index an int or a tuple, into the leading dimensions; cap: the caller's capacity --
    a row of more code points raises ValueError(over(index, row, its length)), the caller's message; None: the caller has checked.  -> (text, len).
    The items are walked once, in order (a generator's own refusals and the capacity's come in the order of the rows), then written in one scatter."""
    text, ln = out if isinstance(out[0], np.ndarray) else (np.zeros(out, np.int32), np.zeros(out[:-1], np.int32))
    where, rows = [], []
    for at, s in items:
        if cap is not None and len(s) > cap:
            raise ValueError(over(at, s, len(s)))
        where.append(at)
        rows.append(s)
    if rows:
        n = np.fromiter(map(len, rows), np.int64, len(rows))
        if all(isinstance(s, str) for s in rows):
            cps = np.frombuffer("".join(rows).encode("utf-32-le", "surrogatepass"), "<i4")          # ord() of every character, lone surrogates included
        else:
            cps = np.fromiter((c for s in rows for c in (map(ord, s) if isinstance(s, str) else s)), np.int64, int(n.sum()))
        row = np.ravel_multi_index(tuple(np.array(where).T.reshape(ln.ndim, -1)), ln.shape)
        assert text.flags.c_contiguous and ln.flags.c_contiguous                                  # (the reshapes below are views)
        ln.reshape(-1)[row] = n
        if cps.size:
            text.reshape(-1, text.shape[-1])[np.repeat(row, n), np.arange(cps.size) - np.repeat(np.cumsum(n) - n, n)] = cps
    return text, ln


def unpack(text, text_len):
    """the inverse's first half, as the kernels clamp: -> (text as numpy [..., W], lengths reshaped to text.shape[:-1] and clamped into [0, W])"""
    text = to_numpy(text)
    return text, np.clip(to_numpy(text_len).reshape(text.shape[:-1]), 0, text.shape[-1])


def map_slots(text, text_len, counts, dim, fn):
    """float32 [B, No, dim] of packed text [B, No, W]: fn(the slot's code points, cut to its clamped length) for the first counts[b] slots of sample b
    (clamped into [0, No]; None: all), zero rows behind them -- the frame of the per-token kernels' host twins"""
    text, ln = unpack(text, text_len)
    B, No = text.shape[:2]
    cnt = np.full(B, No) if counts is None else np.clip(to_numpy(counts), 0, No)
    out = np.zeros((B, No, dim), np.float32)
    for b in range(B):
        for i in range(int(cnt[b])):
            out[b, i] = fn(text[b, i, :ln[b, i]])
    return out


def strings(text, text_len):
    """rows [n, W] cut to lengths [n] -> list of n str"""
    return [text_of(row[:n]) for row, n in zip(to_numpy(text).tolist(), to_numpy(text_len).reshape(-1).tolist())]


def pinned(tensors, pin_memory):
    return {k: v.pin_memory() for k, v in tensors.items()} if pin_memory else tensors


def first_flagged(status, reasons, **params):
    """status: a host list of status words; reasons: ((bit, text), ...) in the order a word's bits are named -> (index, bit, text % params) of the first
    word with a listed bit, named by the first such bit, or None"""
    for i, st in enumerate(status):
        for bit, text in reasons:
            if st & bit:
                return i, bit, text % params


# ---------------------------------------------------------------------------------------------------------------- the key groups
class Group:
    """One form of one text: keys, the (data, lengths-or-offsets) pair that opts a batch in -- both or neither.
    shape: (the leading dimensions' names, the width's name, its maximum) of a packed pair: text int32 [*dims, width <= max], lengths int32 [*dims];
    checked: `check` enforces it (where not, the launch wrappers in ops.py are the first to look).
    rules, applied in order, each (kind, keys, clause):
      "not"   none of `keys` may sit beside the pair; the message lists the ones that do and ends in the clause
      "need"  every one of `keys` must; the message lists the missing ones, then the clause
      "pair"  "need", but `keys` is itself a pair: one of them without the other is reported as that
      "any"   at least one of `keys` must; the message names them all"""

    def __init__(self, keys, shape=None, checked=False, rules=()):
        self.keys, self.shape, self.checked, self.rules = tuple(keys), shape, checked, tuple(rules)
        self.label = " / ".join(self.keys)


def _whole(keys, batch_dict):
    have = [k for k in keys if k in batch_dict]
    if have and len(have) != len(keys):
        raise ValueError("batch carries %s without %s" % (" / ".join(have), " / ".join(k for k in keys if k not in batch_dict)))
    return bool(have)


def has_text(group, batch_dict):
    return any(k in batch_dict for k in group.keys)


def check(group, batch_dict, n_ocr=None, kinds=("not", "need", "pair", "any")):
    """walk a declaration: -> False for a batch with neither key of the pair; ValueError for one key without the other, for a broken rule (the first, in
    the declared order) and, in a `checked` group, for a pair that is not of the declared shape or -- n_ocr given -- holds another number of slots per
    sample; else True.  kinds: the rules to apply now (textprep.check_raw looks at both raw groups before it asks for what either needs)."""
    if not _whole(group.keys, batch_dict):
        return False
    for kind, keys, clause in (r for r in group.rules if r[0] in kinds):
        there = [k for k in keys if k in batch_dict]
        if kind == "pair":
            _whole(keys, batch_dict)
        if kind == "not":
            broken, what = there, "and %s: %s" % (" / ".join(there), clause)
        elif kind == "any":
            broken, what = not there, "without %s%s" % (" or ".join(keys), clause)
        else:
            broken, what = len(there) != len(keys), "without %s%s" % (" / ".join(k for k in keys if k not in there), clause)
        if broken:
            raise ValueError("batch carries %s %s" % (group.label, what))
    if group.checked:
        (text_key, len_key), (dims, width, limit) = group.keys, group.shape
        text, ln = batch_dict[text_key], batch_dict[len_key]
        rank = len(dims) + 1
        if text.dim() != rank or text.dtype != torch.int32 or ln.dtype != torch.int32 or tuple(ln.shape) != tuple(text.shape[:rank - 1]) or not 1 <= text.shape[rank - 1] <= limit:
            raise ValueError("%s must be int32 [%s, %s <= %d] and %s int32 [%s]; got %s %s and %s %s" % (
                text_key, ", ".join(dims), width, limit, len_key, ", ".join(dims), tuple(text.shape), text.dtype, tuple(ln.shape), ln.dtype))
        if n_ocr is not None and text.shape[1] != n_ocr:
            raise ValueError("%s holds %d slots per sample, the batch %d OCR rows" % (text_key, text.shape[1], n_ocr))
    return True


_QUESTION_TEXT, _OCR_TEXT, _ANSWER_TEXT = ("question_text", "question_text_len"), ("ocr_text", "ocr_text_len"), ("answer_text", "answer_text_len")
_QUESTION_IDS, _RAW_CLAUSE = ("question_indices", "question_mask"), "give the raw strings or their packed text, not both"

QUESTION_RAW = Group(("question_raw", "question_raw_off"), rules=[("not", _QUESTION_TEXT + _QUESTION_IDS, "give the raw question, its packed text or its ids, not more than one")])
QUESTION_TEXT = Group(_QUESTION_TEXT, (("B",), "Lq", 1024), True, [("not", _QUESTION_IDS, "give the question's text or its ids, not both")])
OCR_RAW = Group(("ocr_raw", "ocr_raw_off"), rules=[("not", _OCR_TEXT, _RAW_CLAUSE), ("need", ("ocr_count",), "")])
# one text, two readers: each refuses its own finished tensor beside the text and nothing else
OCR_TEXT_PHOC = Group(_OCR_TEXT, (("B", "No"), "Lw", 64), True, [("not", ("ocr_phoc", "ocr_phoc_rows"), "give the tokens' text or their PHOC, not both")])
OCR_TEXT_FASTTEXT = Group(_OCR_TEXT, (("B", "No"), "Lw", 64), True, [("not", ("ocr_fasttext", "ocr_ft_rows"), "give the tokens' text or their FastText vectors, not both")])
ANSWER_RAW = Group(("answer_raw", "answer_raw_off"), rules=[("not", _ANSWER_TEXT, _RAW_CLAUSE), ("any", ("ocr_count", "ocr_text"), " to take the batch size from")])
# again one text, two readers; they name the absent OCR text differently (a lone ocr_text is the answer table's "without ocr_text_len", the score
# table's "ocr_text without ocr_text_len") and the score table asks for it before it looks for a table beside the text
ANSWER_TEXT_TABLE = Group(_ANSWER_TEXT, (("B", "A"), "La", 128), False, [
    ("not", ("answer_table", "targets"), "give the answers' text, their table or the dense targets, only one of them"),
    ("need", _OCR_TEXT, ": the answers are matched against the OCR tokens' text")])
ANSWER_TEXT_SCORE = Group(_ANSWER_TEXT, (("B", "A"), "La", 128), False, [
    ("pair", _OCR_TEXT, ": the score table holds the OCR tokens' text"), ("not", ("score_table",), "give the answers' text or their score table, not both")])
GROUPS = {"question raw": QUESTION_RAW, "question text": QUESTION_TEXT, "OCR raw": OCR_RAW, "OCR text, PHOC": OCR_TEXT_PHOC, "OCR text, FastText": OCR_TEXT_FASTTEXT,
          "answer raw": ANSWER_RAW, "answer text, answer table": ANSWER_TEXT_TABLE, "answer text, score table": ANSWER_TEXT_SCORE}
