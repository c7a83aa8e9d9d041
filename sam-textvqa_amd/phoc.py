"""PHOC features of the OCR tokens from their text.

The reference builds the 604-column pyramidal histogram of characters per token on the host (sam/phoc/build_phoc.py + sam/phoc/cphoc.c behind PhocProcessor,
sam/datasets/processors.py:407-440), caches it and ships fp32 [50, 604] with every sample: 120 KB padded, 1208 B per valid row of a ragged fp16 batch.  PHOC is
a pure function of the token's characters, and those are at most 4 * Lw = 128 B per slot as code points:

    ocr_text int32 [B, No, Lw]     ocr_text_len int32 [B, No]

A batch that carries these two keys and NO ocr_phoc (padded form) / ocr_phoc_rows (ragged form) has its PHOC computed on the GPU, one launch
(ops.phoc_from_text, csrc/phoc.hip).  A batch with a score table (metrics.collate_score_tables) already holds exactly these tensors and may pass
score_table["ocr"] / score_table["ocr_len"] as the two keys: the score table's text is lowered, which PHOC's folding does anyway, its NO_GLUE flag bit is
masked off, and its "<pad>" slots lie at or past the sample's OCR count, where the rows are zero whatever the text holds.

Folding (build_phoc): token.lower(), then only a-z 0-9 are kept.  Per code point that is: ASCII A-Z to lower case, plus exactly the non-ASCII code points
whose str.lower() contains a kept character (FOLD_TABLE: enumerated over all code points, re-derived by tests/test_phoc_cpu.py); everything else is dropped.
str.lower() is context-free except for the final sigma, which is dropped either way.

The region test is the reference's fp32 sequence, NOT the exact rational one (see _region_hit): the two differ for everyday tokens, first at the middle
letter of "the".  phoc_host is the host twin of the kernel, in the role metrics.score_answers_host plays for the metrics."""
import numpy as np
import torch

from . import batchtext as BT
from . import metrics

PHOC_DIM = 604
ALPHABET = "abcdefghijklmnopqrstuvwxyz0123456789"
# the 50 bigrams in column order (data: the name list of tests/golden/phoc.npz, which the generator reads out of the reference's compiled module's rows)
BIGRAMS = ("th", "he", "in", "er", "an", "re", "es", "on", "st", "nt", "en", "at", "ed", "nd", "to", "or", "ea", "ti", "ar", "te", "ng", "al", "it", "as", "is",
           "ha", "et", "se", "ou", "of", "le", "sa", "ve", "ro", "ra", "ri", "hi", "ne", "me", "de", "co", "ta", "ec", "si", "ll", "so", "na", "li", "la", "el")
# non-ASCII code point -> the kept character its str.lower() contains (U+0130 lowers to "i" + a combining dot, U+212A KELVIN SIGN to "k")
FOLD_TABLE = {0x0130: "i", 0x212A: "k"}
UNIGRAM_LEVELS = (2, 3, 4, 5)
UNIGRAM_COLUMNS = 36 * sum(UNIGRAM_LEVELS)           # 504: the bigram block starts here
MAX_CHARS = 64                                       # one code point per lane of the kernel

_CHAR_INDEX = {c: i for i, c in enumerate(ALPHABET)}
_BIGRAM_INDEX = {(_CHAR_INDEX[b[0]], _CHAR_INDEX[b[1]]): k for k, b in enumerate(BIGRAMS)}
_CP_MASK = metrics.NO_GLUE - 1                       # the score table's flag bit (and anything above it) is not part of the code point


def fold(token):
    """alphabet indices (a-z -> 0..25, 0-9 -> 26..35) of the characters build_phoc keeps of `token`: a str, or a sequence of code points"""
    out = []
    for cp in BT.code_points(token, _CP_MASK):
        if 0x41 <= cp <= 0x5A:
            cp += 0x20
        ch = FOLD_TABLE.get(cp) if cp >= 0x80 else chr(cp)
        if ch in _CHAR_INDEX:
            out.append(_CHAR_INDEX[ch])
    return out


def _region_hit(lo, hi, n, region, level):
    """cphoc.c's overlap test of the occupancy [lo / n, hi / n] against [region / level, (region + 1) / level], operation by operation in fp32: four
    quotients, max, min, one subtraction each for numerator and denominator, ONE division, compared with 0.5.  Do not simplify it to integers or exact
    fractions: the result differs (tests/test_phoc_cpu.py keeps an exact variant to show it).  lo / hi: int arrays; -> bool array"""
    f = np.float32
    n = f(n)
    occ0, occ1 = lo.astype(f) / n, hi.astype(f) / n
    reg0, reg1 = f(region) / f(level), f(region + 1) / f(level)
    ov0, ov1 = np.maximum(occ0, reg0), np.minimum(occ1, reg1)
    return (ov1 - ov0) / (occ1 - occ0) >= f(0.5)


def phoc_row(chars, region_hit=_region_hit):
    """one PHOC row (float32 [604]) of the folded characters `chars` (alphabet indices)"""
    row = np.zeros(PHOC_DIM, np.float32)
    n = len(chars)
    if n == 0:
        return row
    ch = np.asarray(chars, np.int64)
    index = np.arange(n)
    base = 0
    for level in UNIGRAM_LEVELS:
        for region in range(level):
            hit = region_hit(index, index + 1, n, region, level)
            row[(base + region) * 36 + ch[hit]] = 1.0
        base += level
    if n > 1:
        at = np.array([i for i in range(n - 1) if (chars[i], chars[i + 1]) in _BIGRAM_INDEX], np.int64)
        if at.size:
            bg = np.array([_BIGRAM_INDEX[(chars[i], chars[i + 1])] for i in at], np.int64)
            for region in range(2):
                hit = region_hit(at, at + 2, n, region, 2)
                row[UNIGRAM_COLUMNS + region * 50 + bg[hit]] = 1.0
    return row


def phoc_host(tokens):
    """numpy float32 [len(tokens), 604]: build_phoc of every token (str, or a sequence of code points), the kernel's host twin"""
    out = np.zeros((len(tokens), PHOC_DIM), np.float32)
    for i, t in enumerate(tokens):
        out[i] = phoc_row(fold(t))
    return out


def phoc_host_text(ocr_text, ocr_text_len, counts=None):
    """the kernel's output for packed text, on the host: float32 [B, No, 604] with the kernel's clamps (lengths into [0, Lw], counts into [0, No])"""
    return BT.map_slots(ocr_text, ocr_text_len, counts, PHOC_DIM, lambda cps: phoc_row(fold(cps)))


def pack_ocr_text(tokens_per_sample, max_ocr_tokens=50, max_chars=metrics.DEFAULT_SCORE_CAPS.Lw, pin_memory=False):
    """list (one entry per sample) of lists of str -> {"ocr_text": int32 [B, No, Lw], "ocr_text_len": int32 [B, No]} on the CPU, No = max_ocr_tokens,
    Lw = max_chars (at most 64).  A sample keeps its first max_ocr_tokens tokens, as _pad_features / PhocProcessor do; the slots behind them are empty.
    A token of more than max_chars code points raises ValueError naming the sample and the token: nothing is truncated, because PHOC depends on the
    token's length.  A batch with a score table may pass score_table["ocr"] / score_table["ocr_len"] as these two keys instead (module docstring)."""
    B, No, Lw = len(tokens_per_sample), int(max_ocr_tokens), int(max_chars)
    if B == 0:
        raise ValueError("pack_ocr_text: no samples")
    if not 1 <= Lw <= MAX_CHARS:
        raise ValueError("pack_ocr_text: max_chars = %d must be in [1, %d]" % (Lw, MAX_CHARS))
    text, ln = BT.pack_rows((B, No, Lw), (((b, i), t) for b, tokens in enumerate(tokens_per_sample) for i, t in enumerate(list(tokens)[:No])), Lw,
                           lambda at, t, n: "sample %d: OCR token %d (%r) has %d code points, over max_chars = %d" % (at + (t, n, Lw)))
    return BT.pinned({"ocr_text": torch.from_numpy(text), "ocr_text_len": torch.from_numpy(ln)}, pin_memory)


TEXT_KEYS = ("ocr_text", "ocr_text_len")


def has_text(batch_dict):
    return BT.has_text(BT.OCR_TEXT_PHOC, batch_dict)


def check(batch_dict, n_ocr=None):
    """a batch opts in with BOTH text keys and no PHOC tensor of either form; -> whether it opted in"""
    return BT.check(BT.OCR_TEXT_PHOC, batch_dict, n_ocr)


def phoc_from_text(ocr_text, ocr_text_len, counts=None, dtype=torch.float32):
    """the GPU [B, No, 604] 0/1 tensor (fp32 or bf16) of packed text, one launch; counts int32 [B] (optional): slots at or past it are zero rows"""
    from . import ops
    B, No = ocr_text.shape[:2]
    out = torch.empty((B, No, PHOC_DIM), dtype=dtype, device=ocr_text.device)
    ops.phoc_from_text(ocr_text.contiguous(), ocr_text_len.contiguous(), counts, out.view(B * No, PHOC_DIM))
    return out
