"""CPU (no GPU needed): the batch's raw strings to cleaned code points (sam_textvqa_amd/textprep.py, include/sam_hip_textprep.h).
The host twin clean_host on pack_utf8's bytes against the golden the reference's word_cleaner / word_cleaner_lower wrote (tests/golden/textprep.json),
against the host packers on a synthetic batch, and the status bits against bytes.decode; then the refusals of materialize and collate_ragged."""
import json
import os
from ctypes import c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi
from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import phoc as P
from sam_textvqa_amd import ragged as R
from sam_textvqa_amd import textprep as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textprep.json")
_cache = {}


def load_golden():
    if not _cache:
        with open(GOLDEN) as f:
            _cache.update(json.load(f))
    return _cache


def word_cleaner(w):
    """the definition the issue and the header give (Python's chained replace), for strings the golden does not hold"""
    return w.lower().replace(",", "").replace("?", "").replace("'s", " 's").strip()


def padded(strings, L):
    """what the host packers write for one row per string: (int32 [S, L], int32 [S])"""
    text, ln = np.zeros((len(strings), L), np.int32), np.zeros(len(strings), np.int32)
    for i, s in enumerate(strings):
        text[i, :len(s)] = [ord(c) for c in s]
        ln[i] = len(s)
    return text, ln


def raw_batch(B, seed=0, n_ocr=50):
    """metrics.make_score_text's samples with the dirt the cleaner removes put back: (raw answers, raw tokens) per sample"""
    _, answers, tokens = M.make_score_text(B, num_vocab=120, n_ocr=n_ocr, seed=seed, rich=True)
    rng = np.random.RandomState(seed + 7)

    def dirty(s):
        k = rng.randint(6)
        return (s.upper(), "  " + s + "\t", s + "?", s.replace(" ", ", "), s.capitalize() + ",", s)[k]
    return [[dirty(a) for a in ans] for ans in answers], [[dirty(t) for t in tok] for tok in tokens]


def test_whitespace_list_is_the_golden_and_the_interpreters():
    ws = load_golden()["whitespace"]
    assert sorted(T.WHITESPACE) == ws == sorted(A.WHITESPACE)
    assert ws == [c for c in range(0x110000) if chr(c).isspace()]


def test_golden_covers_what_it_should():
    g = load_golden()
    strings = {c["s"] for c in g["cases"]}
    assert len(strings) == len(g["cases"]) >= 300
    assert {"'s", "'S", "'?s", "',s", "''s", "'ss", "'", "s'", "", "İ", "ẞ", "K", "ΟΔΟΣ"} <= strings
    for w in g["whitespace"]:
        assert any(s.startswith(chr(w)) and s.endswith(chr(w)) and chr(w) in s[1:-1] for s in strings), hex(w)
    assert {len(chr(c).encode()) for s in strings for c in map(ord, s)} == {1, 2, 3, 4}
    assert any(c["word_cleaner"] == "" and c["s"] != "" for c in g["cases"])


@pytest.mark.parametrize("mode,key", [(T.WORD_CLEANER, "word_cleaner"), (T.WORD_CLEANER_LOWER, "word_cleaner_lower"), (T.VERBATIM, "s")])
def test_twin_equals_the_reference_cleaner(mode, key):
    cases = load_golden()["cases"]
    L = T.MAX_CHARS
    p = T.pack_utf8([[c["s"] for c in cases]], len(cases), lower=mode != T.VERBATIM)
    text, ln, status = T.clean_host(p["raw"], p["raw_off"], L, mode)
    want_text, want_len = padded([c[key] for c in cases], L)
    assert not status.any()
    np.testing.assert_array_equal(ln, want_len)
    np.testing.assert_array_equal(text, want_text)                    # padding included
    assert text.dtype == ln.dtype == status.dtype == np.int32


def test_pack_utf8_layout():
    p = T.pack_utf8([["ab", "", "é"], [], ["x", "y", "z", "dropped"], ["İZ", "QQ"]], 3)
    assert p["raw"].dtype == torch.uint8 and p["raw_off"].dtype == torch.int32 and p["count"].dtype == torch.int32
    assert p["count"].tolist() == [3, 0, 3, 2]
    want = [b"ab", b"", "é".encode(), b"", b"", b"", b"x", b"y", b"z", "İZ".lower().encode(), b"QQ", b""]        # only the non-ASCII string is lowered
    assert bytes(p["raw"].numpy()) == b"".join(want)
    assert p["raw_off"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    q = T.pack_utf8([["İZ"]], 1, lower=False)
    assert bytes(q["raw"].numpy()) == "İZ".encode()
    with pytest.raises(ValueError, match="no samples"):
        T.pack_utf8([], 3)
    with pytest.raises(ValueError, match="slots_per_sample"):
        T.pack_utf8([["a"]], 0)


def test_synthetic_batch_equals_the_host_packers_key_by_key():
    B, No, A_, Lw = 5, 50, 10, M.DEFAULT_SCORE_CAPS.Lw          # (the packers' default widths: Lw = 32 for the score table, La = 128)
    raw_answers, raw_tokens = raw_batch(B)
    want = dict(P.pack_ocr_text([[word_cleaner(t) for t in tok] for tok in raw_tokens], No))
    want.update(A.pack_answer_text([[word_cleaner(a) for a in ans] for ans in raw_answers], A_))
    po, pa = T.pack_utf8(raw_tokens, No), T.pack_utf8(raw_answers, A_)
    ot, ol, os_ = T.clean_host(po["raw"], po["raw_off"], Lw, T.WORD_CLEANER)
    at, al, as_ = T.clean_host(pa["raw"], pa["raw_off"], 128, T.WORD_CLEANER)
    assert not os_.any() and not as_.any()
    got = {"ocr_text": ot.reshape(B, No, Lw), "ocr_text_len": ol.reshape(B, No), "answer_text": at.reshape(B, A_, 128), "answer_text_len": al.reshape(B, A_)}
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].numpy().dtype, k
        np.testing.assert_array_equal(got[k], want[k].numpy(), err_msg=k)
    assert torch.equal(po["count"], M.ocr_counts(raw_tokens, No))
    # clean_answers = False: the answers' exact code points
    pv = T.pack_utf8(raw_answers, A_, lower=False)
    vt, vl, vs = T.clean_host(pv["raw"], pv["raw_off"], 128, T.VERBATIM)
    verb = A.pack_answer_text(raw_answers, A_)
    np.testing.assert_array_equal(vt.reshape(B, A_, 128), verb["answer_text"].numpy())
    np.testing.assert_array_equal(vl.reshape(B, A_), verb["answer_text_len"].numpy())


def decodes(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


INVALID = {
    "truncated 2": b"a\xc3", "truncated 3": b"\xe4\xb8", "truncated 4": b"\xf0\x9f\x98", "truncated mid": b"\xe4\xb8x", "stray continuation": b"a\x80b",
    "stray after complete": b"\xc3\xa9\xa9", "leading continuation": b"\xbf", "overlong 2 (C0)": b"\xc0\xaf", "overlong 2 (C1)": b"\xc1\xbf",
    "overlong 3": b"\xe0\x9f\xbf", "overlong 4": b"\xf0\x8f\xbf\xbf", "surrogate low": b"\xed\xa0\x80", "surrogate high": b"\xed\xbf\xbf",
    "above 10FFFF (F4 90)": b"\xf4\x90\x80\x80", "above 10FFFF (F5)": b"\xf5\x80\x80\x80", "FE": b"\xfe", "FF": b"\xff",
}
VALID_EDGES = [b"", b"\x00", b"\x7f", b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xef\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf"]


def random_byte_slots(n, seed):
    """n byte strings: uniform bytes, bytes biased to UTF-8 structure, valid text cut at a random byte, and valid text with one byte replaced"""
    rng = np.random.RandomState(seed)
    structure = np.array([0x41, 0x73, 0x27, 0x20, 0x80, 0xBF, 0x9F, 0xA0, 0x90, 0x8F, 0xC2, 0xDF, 0xE0, 0xE1, 0xED, 0xEF, 0xF0, 0xF1, 0xF4, 0xC0, 0xC1, 0xF5, 0xFF], np.uint8)
    texts = [c["s"].encode() for c in load_golden()["cases"] if c["s"]]
    out = []
    for i in range(n):
        k, ln = i % 4, rng.randint(0, 12)
        if k == 0:
            out.append(rng.randint(0, 256, ln).astype(np.uint8).tobytes())
        elif k == 1:
            out.append(structure[rng.randint(0, len(structure), ln)].tobytes())
        else:
            t = bytearray(texts[rng.randint(len(texts))])
            if k == 2:
                t = t[:rng.randint(0, len(t) + 1)]
            else:
                t[rng.randint(len(t))] = rng.randint(256)
            out.append(bytes(t))
    return out


def pack_bytes(slots):
    off = np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int32)
    return np.frombuffer(b"".join(slots), np.uint8), off


def test_status_utf8_is_exactly_where_bytes_decode_raises():
    slots = list(INVALID.values()) + VALID_EDGES + random_byte_slots(4000, 3)
    assert not any(decodes(b) for b in INVALID.values()) and all(decodes(b) for b in VALID_EDGES)
    raw, off = pack_bytes(slots)
    for mode in (0, 15):
        text, ln, status = T.clean_host(raw, off, 64, mode)
        ok = np.array([decodes(b) for b in slots])
        assert 0.2 < ok.mean() < 0.8                                      # both outcomes well represented
        np.testing.assert_array_equal(status == T.STATUS_UTF8, ~ok)
        assert not status[ok].any() and not text[~ok].any() and not ln[~ok].any()
        if mode == 0:
            for i in np.flatnonzero(ok):
                assert text[i, :ln[i]].tolist() == [ord(c) for c in slots[i].decode()] and not text[i, ln[i]:].any()


def test_status_long_and_offsets():
    L = 8
    slots = [b"a" * L, b"a" * (L + 1), b"  " + b"a" * L + b" \t ", b"x's" + b"a" * (L - 3), b"," * 5 + b"a" * L + b"?", "é".encode() * L, "é".encode() * (L + 1)]
    raw, off = pack_bytes(slots)
    text, ln, status = T.clean_host(raw, off, L, 15)
    assert status.tolist() == [0, T.STATUS_LONG, 0, T.STATUS_LONG, 0, 0, T.STATUS_LONG]          # (slot 3: L raw code points, L + 1 after the possessive)
    assert ln.tolist() == [L, 0, L, 0, L, L, 0] and not text[status != 0].any()
    assert T.clean_host(raw, off, L, 0)[2].tolist() == [0, T.STATUS_LONG, T.STATUS_LONG, 0, T.STATUS_LONG, 0, T.STATUS_LONG]
    # offsets: decreasing, negative, past the end -- flagged, their neighbours served
    bad = np.array([0, 3, 2, 5, 5, len(raw) + 1, len(raw)], np.int32)
    st = T.clean_host(raw, bad, L, 0)[2]
    assert st.tolist() == [0, T.STATUS_OFFSETS, 0, 0, T.STATUS_OFFSETS, T.STATUS_OFFSETS]
    assert T.clean_host(raw, np.array([-1, 2], np.int32), L, 0)[2].tolist() == [T.STATUS_OFFSETS]
    assert T.status_message([0, 2, 1], 8) == "slot 1 has more than L = 8 code points after cleaning (status bit 2)"
    assert T.status_message([0, 0], 8) is None
    with pytest.raises(ValueError):
        T.clean_host(raw, off, 129, 0)
    with pytest.raises(ValueError):
        T.clean_host(raw, off, 8, 16)


def test_materialize_refusals():
    p = T.pack_utf8([["a"], ["b"]], 2)
    full = dict(ocr_raw=p["raw"], ocr_raw_off=p["raw_off"], ocr_count=p["count"])
    plain = {"question_indices": torch.zeros(2, 20)}
    assert T.materialize(plain) is plain and set(plain) == {"question_indices"}          # no raw keys: as before
    for drop in ("ocr_raw", "ocr_raw_off"):
        with pytest.raises(ValueError, match="without"):
            T.materialize({k: v for k, v in full.items() if k != drop})
    with pytest.raises(ValueError, match="without ocr_count"):
        T.materialize({k: v for k, v in full.items() if k != "ocr_count"})
    for k in ("ocr_text", "ocr_text_len"):
        with pytest.raises(ValueError, match="not both"):
            T.materialize(dict(full, **{k: torch.zeros(2, 2, 64, dtype=torch.int32)}))
    ans = dict(answer_raw=p["raw"], answer_raw_off=p["raw_off"])
    with pytest.raises(ValueError, match="not both"):
        T.materialize(dict(full, answer_text_len=torch.zeros(2, 2, dtype=torch.int32), **ans))
    with pytest.raises(ValueError, match="without answer_raw_off"):
        T.materialize(dict(full, answer_raw=p["raw"]))
    with pytest.raises(ValueError, match="batch size"):
        T.materialize(dict(ans))
    with pytest.raises(ValueError, match="slots for B"):
        T.materialize(dict(full, ocr_count=torch.zeros(3, dtype=torch.int32)))
    assert T.has_raw(full) and T.has_raw(ans) and not T.has_raw(plain)


def ragged_samples(tokens, answers=None):
    g = torch.Generator().manual_seed(0)
    out = []
    for i, tok in enumerate(tokens):
        m = len(tok)
        s = dict(obj_features=torch.randn(3, 2048, generator=g), obj_bboxes=torch.rand(3, 5, generator=g), ocr_features=torch.randn(m, 16, generator=g),
                 ocr_fasttext=torch.randn(m, 300, generator=g), ocr_bboxes=torch.rand(m, 5, generator=g), ocr_tokens=tok)
        if answers is not None:
            s["answers"] = answers[i]
        out.append(s)
    return out


def test_collate_ragged_raw_text():
    raw_answers, raw_tokens = raw_batch(3, seed=2, n_ocr=9)
    raw_tokens[1] = raw_tokens[1] + ["Extra", "TOKENS,", "past", "the", "maximum?", "x", "y", "z", "w"]
    batch = R.collate_ragged(ragged_samples(raw_tokens, raw_answers), max_obj_num=4, max_ocr_num=6, raw_text=True)
    assert not {"ocr_text", "ocr_text_len", "answer_text", "answer_text_len", "ocr_phoc_rows"} & set(batch)
    want = R.collate_ragged(ragged_samples([[word_cleaner(t) for t in tok] for tok in raw_tokens], [[word_cleaner(a) for a in ans] for ans in raw_answers]),
                            max_obj_num=4, max_ocr_num=6)
    assert torch.equal(batch["ocr_count"], want["ocr_count"]) and batch["ocr_raw_off"].numel() == 3 * 6 + 1 and batch["answer_raw_off"].numel() == 3 * 10 + 1
    ot, ol, _ = T.clean_host(batch["ocr_raw"], batch["ocr_raw_off"], want["ocr_text"].shape[2], 15)
    at, al, _ = T.clean_host(batch["answer_raw"], batch["answer_raw_off"], 128, 15)
    for k, got in (("ocr_text", ot), ("ocr_text_len", ol), ("answer_text", at), ("answer_text_len", al)):
        np.testing.assert_array_equal(got.reshape(want[k].shape), want[k].numpy(), err_msg=k)
    for k in set(want) - {"ocr_text", "ocr_text_len", "answer_text", "answer_text_len"}:
        n = int(batch["obj_count" if k.startswith("obj") else "ocr_count"].sum()) if k.endswith("_rows") else None      # (rows past the total are not written)
        assert torch.equal(batch[k][:n], want[k][:n]), k
    # the default is unchanged
    assert set(R.collate_ragged(ragged_samples(raw_tokens), max_obj_num=4, max_ocr_num=6)) == set(want) - {"answer_text", "answer_text_len"}
    # refusals
    no_tokens = [{k: v for k, v in s.items() if k != "ocr_tokens"} for s in ragged_samples(raw_tokens)]
    for s in no_tokens:
        s["ocr_phoc"] = torch.zeros(s["ocr_features"].shape[0], 604)
    with pytest.raises(ValueError, match="raw_text needs ocr_tokens"):
        R.collate_ragged(no_tokens, max_obj_num=4, max_ocr_num=6, raw_text=True)
    with pytest.raises(ValueError, match="max_chars"):
        R.collate_ragged(ragged_samples(raw_tokens), max_obj_num=4, max_ocr_num=6, raw_text=True, max_chars=32)
    short = ragged_samples(raw_tokens, [raw_answers[0], raw_answers[1][:9], raw_answers[2]])
    with pytest.raises(ValueError, match="sample 1: expected 10 answers, got 9"):
        R.collate_ragged(short, max_obj_num=4, max_ocr_num=6, raw_text=True)
    mixed = ragged_samples(raw_tokens, raw_answers)
    del mixed[2]["answers"]
    with pytest.raises(ValueError, match="whole batch the same way"):
        R.collate_ragged(mixed, max_obj_num=4, max_ocr_num=6, raw_text=True)


def test_header_adds_one_status_returning_function_to_a_table_of_its_own():
    sig = [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    assert _capi.HEADER_SIGNATURES["textprep"] == {"sam_text_from_utf8": sig} and _capi.HEADER_RESTYPES["textprep"] == {"sam_text_from_utf8": c_int}
    assert "sam_text_from_utf8" not in _capi.SIGNATURES
    for name, other in _capi.HEADER_SIGNATURES.items():                  # every other header of the registry
        assert name == "textprep" or "sam_text_from_utf8" not in other
    assert "sam_text_from_utf8" not in _capi.NO_STATUS and c_int32 is c_int
