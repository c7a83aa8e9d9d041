"""CPU (no GPU needed): the resident Unicode table and its host twins (sam_textvqa_amd/unicode_table.py, include/sam_hip_unicode.h).
lower_host against str.lower() and normalize_host against wordpiece.normalize over the whole code space and on context strings; the text twin
clean_host(table=...) against the reference's cleaners on tests/golden/textprep.json; the question twin against pack_question_text on
tests/golden/wordpiece.json and a seeded fuzz; then the key and argument checks of materialize, collate_ragged and the two C entry points."""
import functools
import json
import os
import random
import unicodedata

import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi
from sam_textvqa_amd import ragged as R
from sam_textvqa_amd import textprep as T
from sam_textvqa_amd import unicode_table as U
from sam_textvqa_amd import wordpiece as W

HERE = os.path.dirname(os.path.abspath(__file__))
CONTEXT = [0x3A3, 0x41, 0x61, 0x27, 0x2E, 0x3A, 0x20, 0x301, 0x345, 0xAD, 0x3B1, 0x31, 0x130, 0x2B0]       # Σ A a ' . : space U+0301 U+0345 U+00AD α 1 U+0130 U+02B0


@functools.lru_cache(maxsize=None)
def table():
    return U.build()


@functools.lru_cache(maxsize=None)
def assigned():
    return [c for c in range(0x110000) if unicodedata.category(chr(c)) not in ("Cn", "Cs", "Co")]


def context_strings(n, seed=0):
    """seeded random strings of 1..8 characters, 80 % from CONTEXT and 20 % from all assigned code points"""
    rng, pool = random.Random(seed), assigned()
    return ["".join(chr(rng.choice(CONTEXT) if rng.random() < 0.8 else rng.choice(pool)) for _ in range(rng.randint(1, 8))) for _ in range(n)]


def packed(s):
    """what pack_question_text writes for normalize's output"""
    return [ord(c) | (W.PUNCT_FLAG if ord(c) >= 128 and unicodedata.category(c).startswith("P") else 0) for c in s]


def fuzz_questions(n, seed=1):
    """questions mixing ASCII, accented Latin, Greek with Σ, CJK, Hangul, U+2028, control and unassigned characters (none of the HOST code points)"""
    rng = random.Random(seed)
    words = ["what", "IS", "the", "Café", "ÉCOLE", "straße", "STRAẞE", "ΟΔΟΣ", "ΣΟΦΟΣ", "Σ", "aΣ", "İstanbul", "naïve", "Ångström", "ǅ", "中文", "東京タワー", "豈", "한국어", "값",
             "Москва", "don't", "«quoted»", "¿qué?", "́̂", "é", "x­y", "a\U000E0001b", "", "͸", "Σa", "AΣ́", "50£", "№5", "…", "—"]
    seps = [" ", " ", " ", "  ", "\t", "\n", " ", " ", " ", "　", "\u000B", "\u0085", "", "​"]
    out = []
    for _ in range(n):
        q = "".join(rng.choice(words) + rng.choice(seps) for _ in range(rng.randint(0, 9)))
        out.append(q if rng.random() < 0.8 else q.encode("ascii", "ignore").decode())
    return out


def test_table_layout_and_surface():
    t = table()
    assert U.is_table(t) and not U.is_table({"block": t["block"]}) and not U.is_table(None)
    assert t["block"].numel() == 8704 and t["rec"].shape[1:] == (128, 2) and int(t["block"].max()) == t["rec"].shape[0] - 1 and int(t["block"].min()) == 0
    assert U.nbytes(t) < 1 << 20                                      # resident size: well under a megabyte
    w0 = t["rec"][t["block"].long()].reshape(-1, 2)[:, 0].numpy()
    assert int((w0 & U.SIGMA_C != 0).sum()) > 1000 and int((w0 & U.SIGMA_I != 0).sum()) > 1000 and not (w0 & U.SIGMA_C != 0)[(w0 & U.SIGMA_I) != 0].any()
    host = [cp for cp in np.nonzero(w0 & U.HOST)[0]]
    assert host == [c for c in range(0x110000) if unicodedata.combining(chr(c)) and unicodedata.category(chr(c)) != "Mn"] and 0x302E in host and len(host) < 64
    # the separator class is normalize's behaviour, not Zs: it also splits at U+2028 / U+2029, and drops U+000B / U+000C before the split
    for cp, flag in ((0x2028, U.SEP), (0x2029, U.SEP), (0x0B, U.DROP), (0x0C, U.DROP), (0x85, U.DROP), (0x09, U.SEP), (0xA0, U.SEP), (0x4E2D, U.CJK), (0xFFFD, U.DROP),
                     (0, U.DROP), (0xE000, U.DROP), (0x378, U.DROP), (0xBF, U.PUNCT), (0xAC00, U.HANGUL), (0x130, U.LOWER_POOL)):
        assert w0[cp] & flag, hex(cp)
    moved = U.to(t, "cpu")
    assert set(moved) == set(U.KEYS) and all(torch.equal(moved[k], t[k]) for k in U.KEYS)
    with pytest.raises(ValueError):
        U.to({"block": t["block"]}, "cpu")


def test_lower_host_is_str_lower_for_every_code_point():
    t = table()
    bad = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000 and
           (U.lower_host([cp], t) != [ord(c) for c in chr(cp).lower()] or U.lower_host([0x41, cp], t) != [ord(c) for c in ("A" + chr(cp)).lower()])]
    assert bad == []


def test_normalize_host_is_normalize_for_every_code_point():
    t = table()
    bad, host = [], []
    for cp in range(0x110000):
        if 0xD800 <= cp < 0xE000:
            continue
        for s in (chr(cp), "a" + chr(cp) + "b"):
            got = U.normalize_host([ord(c) for c in s], t)
            if got is None:
                host.append(cp)
            elif got != packed(W.normalize(s)):
                bad.append(cp)
    assert bad == []
    assert sorted(set(host)) == [c for c in range(0x110000) if unicodedata.combining(chr(c)) and unicodedata.category(chr(c)) != "Mn"] and len(host) == 2 * len(set(host))


def test_lowering_contexts():
    t = table()
    strings = context_strings(100000)
    assert sum("Σ" in s for s in strings) > 20000
    bad = [s for s in strings if U.lower_host([ord(c) for c in s], t) != [ord(c) for c in s.lower()]]
    assert bad == []
    for s in ("ΟΔΟΣ", "ΟΔΟΣ ΣΟΦΟΣ", "AΣ́", "AΣ́A", "Σ", "'Σ", "A'Σ'", "AΣΣ", "AΣ" + "́" * 70, "AΣ" + "́" * 70 + "a", "İİ", "STRAẞE"):
        assert U.lower_host([ord(c) for c in s], t) == [ord(c) for c in s.lower()], s


def test_normalize_contexts():
    """a dropped character between Σ and a letter, a word of marks only, CJK and Hangul next to words, the sigma context ending at the word"""
    t = table()
    for s in ("AΣa", "AΣ", "AΣ b", "AΣ中a", "a ́̂ b", "́ a", "a ́", "中文", "a中b", "한국어 값", "AΣ a", "ΟΔΟΣ?", "¿ΟΔΟΣ?", "x\u000By", " a  b ",
              ";", "İi", "ǅ", "豈"):
        assert U.normalize_host([ord(c) for c in s], t) == packed(W.normalize(s)), s
    rng = random.Random(3)
    alphabet = CONTEXT + [0xE000, 0x4E2D, 0xAC01, 0x2028, 0x0B, 0xC9, 0xBF, 0x1E9E]
    for _ in range(20000):
        s = "".join(chr(rng.choice(alphabet)) for _ in range(rng.randint(1, 8)))
        assert U.normalize_host([ord(c) for c in s], t) == packed(W.normalize(s)), s


def golden_textprep():
    with open(os.path.join(HERE, "golden", "textprep.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("mode,key", [(T.WORD_CLEANER, "word_cleaner"), (T.WORD_CLEANER_LOWER, "word_cleaner_lower"), (T.VERBATIM, "s")])
def test_text_twin_with_a_table_equals_the_reference_cleaner_and_the_host_lowered_route(mode, key):
    cases = golden_textprep()
    strings = [c["s"] for c in cases]
    assert any(not s.isascii() and s.lower() != s for s in strings)
    p = T.pack_utf8([strings], len(strings), lower=mode != T.VERBATIM, host_lower=False)
    assert p["raw"].numpy().tobytes() == "".join(strings).encode()                       # shipped as they are
    text, ln, status = T.clean_host(p["raw"], p["raw_off"], T.MAX_CHARS, mode, table=table())
    assert not status.any()
    for i, c in enumerate(cases):
        assert text[i, :ln[i]].tolist() == [ord(x) for x in c[key]] and not text[i, ln[i]:].any(), c["s"]
    q = T.pack_utf8([strings], len(strings), lower=mode != T.VERBATIM)
    for got, want in zip((text, ln, status), T.clean_host(q["raw"], q["raw_off"], T.MAX_CHARS, mode)):
        np.testing.assert_array_equal(got, want)


@functools.lru_cache(maxsize=None)
def golden_wordpiece():
    with open(os.path.join(HERE, "golden", "wordpiece.json"), encoding="utf-8") as f:
        g = json.load(f)
    return W.vocab_index(g["vocab"]), g["questions"], g["ids_T20"]


def test_question_twin_equals_the_packer_on_golden_and_fuzz():
    index, questions, ids = golden_wordpiece()
    fuzz = fuzz_questions(3000)
    assert any("Σ" in q for q in fuzz) and any(q.isascii() and q for q in fuzz) and any(" " in q for q in fuzz)
    for qs in (questions, fuzz):
        p = W.pack_question_utf8(qs)
        assert p["question_raw_off"].numel() == len(qs) + 1 and p["question_raw"].numpy().tobytes() == "".join(qs).encode()
        text, ln, status = W.question_text_host(p["question_raw"], p["question_raw_off"], table(), max_chars=1024)
        want = W.pack_question_text(qs, max_chars=1024)
        assert not status.any()
        np.testing.assert_array_equal(text, want["question_text"].numpy())
        np.testing.assert_array_equal(ln, want["question_text_len"].numpy())
    text, ln, _ = W.question_text_host(*W.pack_question_utf8(questions).values(), table(), max_chars=1024)
    enc = W.encode_host(text, ln, index, T=20)
    for b, row in enumerate(ids):
        assert enc["question_indices"][b, :len(row)].tolist() == row and int(enc["num_question_tokens"][b]) == len(row), questions[b]


def test_question_twin_status_bits():
    qs = ["ok", "café [SEP] x", "a\u302eb", "é" * 9, "x" * 9, "[MASK]", "[MASK", "é" * 8, "a\u302e [CLS]"]
    p = W.pack_question_utf8(qs)
    text, ln, status = W.question_text_host(p["question_raw"], p["question_raw_off"], table(), max_chars=8)
    assert status.tolist() == [0, 8, 16, 2, 2, 8, 0, 0, 8]
    assert ln.tolist() == [2, 0, 0, 0, 0, 0, 5, 8, 0] and not text[status != 0].any()
    raw = np.frombuffer(b"ab\xc3(cd\xe9", np.uint8)
    _, _, status = W.question_text_host(raw, np.array([0, 2, 4, 6, 7, 5, 9], np.int32), table(), max_chars=8)
    assert status.tolist() == [0, 1, 0, 1, 4, 4]
    for st, word in ((1, "UTF-8"), (2, "max_chars = 8"), (4, "offsets"), (8, "special token"), (16, "on the host")):
        msg = W.question_status_message([0, st], 8)
        assert msg.startswith("sample 1") and word in msg and "status bit %d" % st in msg
    assert W.question_status_message([0, 0], 8) is None
    with pytest.raises(ValueError, match="max_chars"):
        W.question_text_host(p["question_raw"], p["question_raw_off"], table(), max_chars=1025)
    with pytest.raises(ValueError, match="max_chars"):
        W.question_text_from_utf8(p["question_raw"], p["question_raw_off"], table(), max_chars=0)
    with pytest.raises(ValueError, match="sample 1.*str"):
        W.pack_question_utf8(["a", 3])


def test_key_checks_of_materialize():
    p = W.pack_question_utf8(["Café?", "what"])
    t = table()
    assert T.has_raw(dict(p)) and T.QUESTION_RAW_KEYS == ("question_raw", "question_raw_off")
    with pytest.raises(ValueError, match="needs unicode"):
        T.materialize(dict(p))
    with pytest.raises(ValueError, match="question_raw without question_raw_off"):
        T.materialize({"question_raw": p["question_raw"]}, unicode=t)
    for k in ("question_text", "question_text_len", "question_indices", "question_mask"):
        with pytest.raises(ValueError, match="question_raw / question_raw_off and %s" % k):
            T.materialize(dict(p, **{k: torch.zeros(2, 4, dtype=torch.int32)}), unicode=t)
    with pytest.raises(_capi.SamHipError):                                 # the table and the bytes must live on the GPU: no CPU path
        T.materialize(dict(p), unicode=t)
    plain = {"pad_obj_mask": torch.ones(2, 3)}
    assert T.materialize(plain, unicode=t) is plain and not T.has_raw(plain)


def test_collate_ragged_device_lower():
    from tests.test_textprep_cpu import ragged_samples
    tokens, answers = [["CAFÉ", "STRAẞE,"], ["ΟΔΟΣ's", "x", "İ"]], [["Été?"] * 2, ["ΣΟΦΟΣ"] * 2]
    samples = ragged_samples(tokens, answers)
    for s, q in zip(samples, ("What's ÉCRIT?", "plain")):
        s["question"] = q
    batch = R.collate_ragged(samples, max_obj_num=4, max_ocr_num=3, raw_text=True, device_lower=True)
    assert {"question_raw", "question_raw_off", "ocr_raw", "answer_raw"} <= set(batch) and not {"question_text", "question_text_len"} & set(batch)
    assert batch["ocr_raw"].numpy().tobytes() == "".join(tokens[0] + [""] + tokens[1]).encode() and batch["answer_raw"].numpy().tobytes() == "Été?Été?ΣΟΦΟΣΣΟΦΟΣ".encode()
    assert batch["question_raw"].numpy().tobytes() == "What's ÉCRIT?plain".encode()
    host = R.collate_ragged(samples, max_obj_num=4, max_ocr_num=3, raw_text=True)
    assert "question_text" in host and "question_raw" not in host and host["ocr_raw"].numpy().tobytes() == "".join(t if t.isascii() else t.lower() for t in tokens[0] + [""] + tokens[1]).encode()
    t = table()
    for name, mode in (("ocr", 15), ("answer", 15)):
        for got, want in zip(T.clean_host(batch[name + "_raw"], batch[name + "_raw_off"], 32, mode, table=t), T.clean_host(host[name + "_raw"], host[name + "_raw_off"], 32, mode)):
            np.testing.assert_array_equal(got, want)
    text, ln, status = W.question_text_host(batch["question_raw"], batch["question_raw_off"], t)
    assert not status.any() and np.array_equal(text, host["question_text"].numpy()) and np.array_equal(ln, host["question_text_len"].numpy())
    with pytest.raises(ValueError, match="device_lower needs raw_text"):
        R.collate_ragged(samples, max_obj_num=4, max_ocr_num=3, device_lower=True)
    with pytest.raises(ValueError, match="max_question_chars"):
        R.collate_ragged(samples, max_obj_num=4, max_ocr_num=3, raw_text=True, device_lower=True, max_question_chars=64)


def test_header_adds_two_status_returning_functions_to_a_table_of_its_own():
    from ctypes import c_int, c_int64, c_void_p as vp
    tab = [vp, c_int, vp, c_int, vp, c_int]
    assert _capi.HEADER_SIGNATURES["unicode"] == {"sam_text_from_utf8_unicode": [vp, c_int64, vp, c_int, c_int, c_int] + tab + [vp, vp, vp, vp],
                                                  "sam_question_from_utf8": [vp, c_int64, vp, c_int, c_int] + tab + [vp, vp, vp, vp]}
    assert set(_capi.HEADER_RESTYPES["unicode"].values()) == {c_int} and not set(_capi.HEADER_SIGNATURES["unicode"]) & (set(_capi.SIGNATURES) | _capi.NO_STATUS)
    for name, other in _capi.HEADER_SIGNATURES.items():                  # every other header of the registry
        assert name == "unicode" or not set(other) & set(_capi.HEADER_SIGNATURES["unicode"])
    import sam_textvqa_amd._build as b
    assert b.HEADERS["unicode"].endswith("sam_hip_unicode.h") and os.path.exists(b.HEADERS["unicode"])


# one good argument list per entry point (fake, aligned, non-null device addresses: a rejected call reads none of them); each case breaks one thing
P = 0x1000
TABLE_OK = dict(block=P, n_stage1=8704, rec=P, n_blocks=245, pool=P, n_pool=97)
TEXT_OK = dict(raw=P, nbytes=10, raw_off=P, S=2, L=8, mode=15, **TABLE_OK, text=P, text_len=P, status=P, stream=None)
QUESTION_OK = dict(raw=P, nbytes=10, raw_off=P, S=2, L=8, **TABLE_OK, text=P, text_len=P, status=P, stream=None)
COMMON_BAD = [("S", 0, "S=0" ), ("nbytes", -1, "nbytes"), ("nbytes", 1 << 31, "nbytes"), ("raw", None, "null raw"), ("raw_off", None, "null"), ("text", None, "null"),
              ("text_len", None, "null"), ("status", None, "null"), ("raw_off", P + 2, "misaligned"), ("block", None, "null table"), ("rec", None, "null table"),
              ("pool", None, "null table"), ("n_stage1", 8703, "8704"), ("n_blocks", 0, "out of range"), ("n_pool", 0, "out of range"), ("rec", P + 4, "misaligned table")]


@pytest.mark.parametrize("name,ok,bad", [
    ("sam_text_from_utf8_unicode", TEXT_OK, COMMON_BAD + [("L", 0, "L=0"), ("L", 129, "L=129"), ("mode", 16, "mode=16"), ("mode", -1, "mode=-1")]),
    ("sam_question_from_utf8", QUESTION_OK, [(k, v, w.replace("S=0", "B=0")) for k, v, w in COMMON_BAD] + [("L", 0, "Lq=0"), ("L", 1025, "Lq=1025")])])
def test_argument_rejections_come_before_any_device_call(name, ok, bad):
    fn = getattr(_capi.lib(), name)
    for key, value, word in bad:
        args = list(dict(ok, **{key: value}).values())
        assert fn(*args) == _capi.CONSTANTS["SAM_ERR_ARG"] == -1, (name, key, value)
        msg = _capi.lib().sam_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, msg
        with pytest.raises(_capi.SamHipError, match=name):
            _capi.call(name, *args)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_ops_wrappers_reject_cpu_tensors():
    from sam_textvqa_amd import ops
    p = W.pack_question_utf8(["Café"])
    with pytest.raises(_capi.SamHipError, match="GPU"):
        ops.question_from_utf8(p["question_raw"], p["question_raw_off"], 8, table())
    with pytest.raises(_capi.SamHipError, match="GPU"):
        ops.text_from_utf8(p["question_raw"], p["question_raw_off"], 8, 15, unicode=table())
