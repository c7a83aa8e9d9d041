"""The Unicode character table the text kernels read on the device (csrc/text.h UniTable, include/sam_hip_unicode.h).

build() derives everything from this interpreter's own str.lower(), str.isspace() and unicodedata at run time -- no data file is committed, so the table
and the Python functions it stands for (str.lower, wordpiece.normalize) come from one Unicode version and cannot disagree.

Layout, three int32 tensors:

    block [8704]              stage one: block[cp >> 7] = the record block of code point cp (identical blocks are stored once)
    rec   [n_blocks, 128, 2]  stage two: the record of cp is the word pair rec[block[cp >> 7], cp & 127]
    pool  [n_pool]            results of more than one code point, back to back

    word 0   bits 0..20   x: str.lower() of the character is chr(cp ^ x); with LOWER_POOL x is the pool offset of its two code points (U+0130)
             bits 21..29  flags: DROP (normalize drops it: cp 0, U+FFFD, every category C* but tab, newline and return), SEP (normalize splits there:
                          tab, newline, return, Zs, and what str.split() splits at besides: U+2028, U+2029), CJK (wordpiece.is_cjk, and neither of the
                          two before), PUNCT (>= 128 and category P*), SIGMA_C / SIGMA_I (cased and not case-ignorable / case-ignorable, as str.lower()'s
                          final-sigma rule sees them; neither bit: neither), HOST (not Mn but a non-zero combining class: canonical reordering can move
                          it, the question has to be normalised on the host), LOWER_POOL, HANGUL (a precomposed syllable: the composite is arithmetic)
    word 1   the question composite  c -> NFD(c.lower()) without category Mn:
             bits 21..22  n, its code points (0..3)
             bits 0..20   n = 1: x, the result is chr(cp ^ x);  n >= 2: the pool offset of the n code points
             bit 30       n = 1: wordpiece.PUNCT_FLAG of the RESULT (the packer flags the normalised text: U+037E becomes ';', ASCII, unflagged)
             (pool entries of a composite carry their PUNCT_FLAG themselves)

Storing x = cp ^ target rather than the target makes the blocks of unassigned, private-use, CJK and Hangul code points identical, so two stages shrink
1 114 112 records to a few hundred blocks.  U+03A3 is the one character whose lowering depends on its neighbours: its record holds U+03C3 and both
twins and both kernels apply the final-sigma rule from the two SIGMA bits (lower_host states it).

lower_host and normalize_host walk these arrays exactly as the kernels do; tests pin them to str.lower() and wordpiece.normalize over the whole code
space, and the kernels to them bit for bit."""
import unicodedata

import numpy as np
import torch

from .wordpiece import PUNCT_FLAG, is_cjk

BLOCK_SHIFT, BLOCK = 7, 128
N_STAGE1 = 0x110000 >> BLOCK_SHIFT
CP_MASK = (1 << 21) - 1
DROP, SEP, CJK, PUNCT, SIGMA_C, SIGMA_I, HOST, LOWER_POOL, HANGUL = (1 << (21 + i) for i in range(9))
COUNT_SHIFT = 21
SIGMA, SMALL_SIGMA, FINAL_SIGMA = 0x3A3, 0x3C3, 0x3C2
HANGUL_BASE, HANGUL_COUNT = 0xAC00, 11172
KEYS = ("block", "rec", "pool")


def _punct(cp):
    return PUNCT_FLAG if cp >= 128 and unicodedata.category(chr(cp))[0] == "P" else 0


def build():
    """-> {"block": int32 [8704], "rec": int32 [n_blocks, 128, 2], "pool": int32 [n_pool]} on the CPU (module docstring).  About two seconds."""
    w0, w1, pool = np.zeros(0x110000, np.int64), np.zeros(0x110000, np.int64), []
    w0[:] = DROP                                                  # Cn, Co, Cs: dropped, lowered to themselves, neither cased nor case-ignorable
    w1[:] = 1 << COUNT_SHIFT
    category, combining, nfd = unicodedata.category, unicodedata.combining, unicodedata.normalize
    for cp in range(0x110000):
        ch = chr(cp)
        cat = category(ch)
        if cat in ("Cn", "Co", "Cs"):
            continue
        if ch in "\t\n\r":
            flags = SEP
        elif cp == 0 or cp == 0xFFFD or cat[0] == "C":
            flags = DROP
        elif cat == "Zs" or ch.isspace():                         # "".join(out).split() splits wherever str.isspace() holds
            flags = SEP
        elif is_cjk(cp):
            flags = CJK
        else:
            flags = 0
        if cp >= 128 and cat[0] == "P":
            flags |= PUNCT
        if ("AΣ" + ch).lower()[1] == "σ":               # a cased, not case-ignorable character behind the sigma: not final
            flags |= SIGMA_C
        elif ("AΣ" + ch + "A").lower()[1] == "σ":       # skipped on the way to the "A": case-ignorable
            flags |= SIGMA_I
        if cat != "Mn" and combining(ch):
            flags |= HOST
        low = ch.lower()
        if len(low) == 1:
            x = cp ^ ord(low)
        else:
            if len(low) != 2:
                raise ValueError("unicode_table.build: str.lower() of U+%04X has %d code points; the kernels take two" % (cp, len(low)))
            flags |= LOWER_POOL
            x = len(pool)
            pool.extend(ord(c) for c in low)
        if HANGUL_BASE <= cp < HANGUL_BASE + HANGUL_COUNT:
            flags |= HANGUL
            comp = None
        else:
            comp = [ord(c) for c in nfd("NFD", low) if category(c) != "Mn"]
        w0[cp] = flags | x
        if comp is None or comp == [cp]:
            continue
        if len(comp) > 3:
            raise ValueError("unicode_table.build: the composite of U+%04X has %d code points; the kernels take three" % (cp, len(comp)))
        if len(comp) == 1:
            w1[cp] = (1 << COUNT_SHIFT) | (cp ^ comp[0]) | _punct(comp[0])
        else:
            w1[cp] = (len(comp) << COUNT_SHIFT) | len(pool)
            pool.extend(c | _punct(c) for c in comp)
    for cp in np.nonzero((w1 == 1 << COUNT_SHIFT) & (w0 & PUNCT != 0))[0]:          # the characters that stay themselves: the result's flag is their own
        w1[cp] |= PUNCT_FLAG
    if len(pool) > CP_MASK:
        raise ValueError("unicode_table.build: the pool outgrew its 21-bit offsets")
    rec = np.stack([w0, w1], axis=1).astype(np.int32).reshape(N_STAGE1, BLOCK * 2)
    uniq, inverse = np.unique(rec, axis=0, return_inverse=True)
    return {"block": torch.from_numpy(inverse.reshape(-1).astype(np.int32)), "rec": torch.from_numpy(uniq.reshape(-1, BLOCK, 2).copy()),
            "pool": torch.tensor(pool or [0], dtype=torch.int32)}


def is_table(v):
    return isinstance(v, dict) and all(torch.is_tensor(v.get(k)) and v[k].dtype == torch.int32 for k in KEYS) and v["block"].numel() == N_STAGE1 and \
        v["rec"].dim() == 3 and tuple(v["rec"].shape[1:]) == (BLOCK, 2)


def to(table, device):
    """the table with its three tensors on `device`, contiguous"""
    if not is_table(table):
        raise ValueError("unicode_table.to: not a table of unicode_table.build()")
    return {k: table[k].to(device).contiguous() for k in KEYS}


def nbytes(table):
    """the resident size"""
    return sum(table[k].numel() * 4 for k in KEYS)


def _lists(table):
    """the three arrays as Python lists (kept beside the tensors: the twins index them a million times in the tests)"""
    host = table.get("_lists")
    if host is None:
        host = table["_lists"] = tuple(table[k].detach().cpu().reshape(-1).tolist() for k in KEYS)
    return host


def lower_host(code_points, table):
    """str.lower() of a whole string as sam_text_from_utf8_unicode computes it: list of code points -> list of code points.  One walk from left to right
    with the kernel's carried state: whether the last character outside class I was of class C (prev_cased), and at most one sigma whose successor has
    not been seen yet (pend, its output position).  U+03A3 becomes the final sigma U+03C2 iff the nearest character outside class I before it is of
    class C and the nearest one behind it is not (or there is none)."""
    block, rec, pool = _lists(table)
    out, prev_cased, pend = [], False, -1
    for cp in code_points:
        w = rec[((block[cp >> BLOCK_SHIFT] << BLOCK_SHIFT) | (cp & (BLOCK - 1))) * 2]
        was = prev_cased
        if not w & SIGMA_I:
            prev_cased = bool(w & SIGMA_C)
            if pend >= 0:
                if not prev_cased:
                    out[pend] = FINAL_SIGMA
                pend = -1
        if cp == SIGMA:
            if was:
                pend = len(out)
            out.append(SMALL_SIGMA)
        elif w & LOWER_POOL:
            out.extend(pool[(w & CP_MASK): (w & CP_MASK) + 2])
        else:
            out.append(cp ^ (w & CP_MASK))
    if pend >= 0:
        out[pend] = FINAL_SIGMA
    return out


def normalize_host(code_points, table):
    """wordpiece.normalize of a string, as packed code points (PUNCT_FLAG on), as sam_question_from_utf8 computes it; None when the string holds a HOST
    code point.  One walk: dropped characters vanish before anything else sees them; a separator or a CJK ideograph ends the word (and the sigma
    context with it); every other character is replaced by its composite; a blank goes in front of the first code point a word emits when an earlier
    word emitted one."""
    block, rec, pool = _lists(table)
    out, brk, prev_cased, pend = [], False, False, -1
    for cp in code_points:
        i = ((block[cp >> BLOCK_SHIFT] << BLOCK_SHIFT) | (cp & (BLOCK - 1))) * 2
        w0, w1 = rec[i], rec[i + 1]
        if w0 & HOST:
            return None
        if w0 & DROP:
            continue
        was = prev_cased
        if w0 & (SEP | CJK):
            if pend >= 0:
                out[pend] = FINAL_SIGMA
            prev_cased, pend, brk = False, -1, True
            if w0 & SEP:
                continue
        elif not w0 & SIGMA_I:
            prev_cased = bool(w0 & SIGMA_C)
            if pend >= 0:
                if not prev_cased:
                    out[pend] = FINAL_SIGMA
                pend = -1
        n = (w1 >> COUNT_SHIFT) & 3
        if cp == SIGMA:
            vals = [SMALL_SIGMA]
        elif w0 & HANGUL:
            s = cp - HANGUL_BASE
            vals = [0x1100 + s // 588, 0x1161 + s % 588 // 28] + ([0x11A7 + s % 28] if s % 28 else [])
        elif n == 1:
            vals = [(cp ^ (w1 & CP_MASK)) | (w1 & PUNCT_FLAG)]
        else:
            vals = pool[(w1 & CP_MASK): (w1 & CP_MASK) + n]
        if vals:
            if brk and out:
                out.append(0x20)
            brk = False
            if cp == SIGMA and was:
                pend = len(out)
            out.extend(vals)
        if w0 & CJK:
            brk = True
    if pend >= 0:
        out[pend] = FINAL_SIGMA
    return out
