"""GPU: the two kernels that read the resident Unicode table (csrc/textprep.hip sam_text_from_utf8_unicode, csrc/unicode_text.hip
sam_question_from_utf8) against their host twins textprep.clean_host(table=...) and wordpiece.question_text_host, bit for bit in text
(padding included), lengths and status -- the twins themselves are held against str.lower() and wordpiece.normalize by tests/test_unicode_text_cpu.py.
One code point per slot over the whole code space; context strings; sequences, U+0130, undecided sigmas, special tokens and mark-only words across the
64-byte chunks; slot counts and capacities at their limits; every status bit between clean neighbours, with guard words; ASCII equivalence with
sam_text_from_utf8; materialize(unicode=...) end to end."""
import functools
import unicodedata

import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi
from sam_textvqa_amd import ops
from sam_textvqa_amd import textprep as T
from sam_textvqa_amd import unicode_table as U
from sam_textvqa_amd import wordpiece as W
from tests.test_textprep_cpu import load_golden, pack_bytes
from tests.test_unicode_text_cpu import context_strings, fuzz_questions, golden_wordpiece, table

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A
HOST_CODE_POINTS = [c for c in range(0x110000) if unicodedata.combining(chr(c)) and unicodedata.category(chr(c)) != "Mn"]      # what normalize_host refuses


@functools.lru_cache(maxsize=None)
def device_table():
    return U.to(table(), "cuda")


def gpu(a):
    return torch.from_numpy(np.array(a)).cuda()          # (copies: frombuffer arrays are read-only)


def compare(keys, got, want, slots, what):
    for k, g, w in zip(keys, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, bad[:4].tolist(), slots[bad[0][0]][:80], g[bad[0][0]].tolist()[:12], w[bad[0][0]].tolist()[:12])


def check_text(slots, L, mode, what=""):
    """one launch of sam_text_from_utf8_unicode over `slots` (a list of bytes) equals the twin in all three outputs; -> the twin's (text, len, status)"""
    raw, off = pack_bytes(slots)
    out = ops.text_from_utf8(gpu(raw), gpu(off), L, mode, unicode=device_table())
    want = T.clean_host(raw, off, L, mode, table=table())
    compare(ops.TEXT_FROM_UTF8_KEYS, [out[k].cpu().numpy() for k in ops.TEXT_FROM_UTF8_KEYS], want, slots, what)
    return want


def check_question(slots, Lq, what=""):
    """the same for sam_question_from_utf8 and wordpiece.question_text_host"""
    raw, off = pack_bytes(slots)
    out = ops.question_from_utf8(gpu(raw), gpu(off), Lq, device_table())
    want = W.question_text_host(raw, off, table(), max_chars=Lq)
    compare(ops.QUESTION_FROM_UTF8_KEYS, [out[k].cpu().numpy() for k in ops.QUESTION_FROM_UTF8_KEYS], want, slots, what)
    return want


def test_every_code_point_one_per_slot():
    """S = 1 112 064 slots of L = Lq = 4: every code point outside the surrogates through both kernels.  The expected rows come straight from the twins'
    per-character walks (lower_host, normalize_host); decoding is the byte arithmetic below."""
    t = table()
    cps = np.array([c for c in range(0x110000) if not 0xD800 <= c < 0xE000], np.int64)
    S = cps.size
    raw = np.frombuffer("".join(map(chr, cps.tolist())).encode(), np.uint8)
    off = np.concatenate([[0], np.cumsum(1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000))]).astype(np.int32)
    assert off[-1] == raw.size and S > 1100000
    pad = ([0, 0, 0, 0], [0, 0, 0], [0, 0], [0], [])
    rows_t, rows_q = [], []                                         # (lists first: a million numpy row assignments cost more than the twins)
    for cp in cps.tolist():
        low = U.lower_host((cp,), t)
        rows_t.append(low + pad[len(low)])
        q = [cp] if cp < 0x80 else U.normalize_host((cp,), t)
        rows_q.append(pad[0] if q is None else q + pad[len(q)])
    want_t, want_q = np.array(rows_t, np.int32), np.array(rows_q, np.int32)
    want_tl, want_ql = (want_t != 0).sum(1).astype(np.int32), (want_q != 0).sum(1).astype(np.int32)
    want_tl[0] = want_ql[0] = 1                                     # U+0000 is the one code point whose row is its own padding
    want_qs = np.where((want_ql == 0) & np.isin(cps, HOST_CODE_POINTS), 16, 0).astype(np.int32)
    g_raw, g_off = gpu(raw), gpu(off)
    out = ops.text_from_utf8(g_raw, g_off, 4, T.LOWER, unicode=device_table())
    assert np.array_equal(out["text"].cpu().numpy(), want_t) and np.array_equal(out["text_len"].cpu().numpy(), want_tl) and not out["status"].any()
    out = ops.question_from_utf8(g_raw, g_off, 4, device_table())
    assert np.array_equal(out["status"].cpu().numpy(), want_qs) and 0 < (want_qs == 16).sum() < 64
    assert np.array_equal(out["question_text"].cpu().numpy(), want_q) and np.array_equal(out["question_text_len"].cpu().numpy(), want_ql)


def test_context_strings():
    slots = [s.encode() for s in context_strings(20000, seed=5)]
    for mode in (15, 1):
        assert not check_text(slots, 16, mode, "contexts")[2].any()
    st = check_question(slots, 16, "contexts")[2]
    assert set(st.tolist()) <= {0, 16} and (st == 0).mean() > 0.9


def test_golden_and_fuzz():
    cases = load_golden()["cases"]
    slots = [c["s"].encode() for c in cases]                       # unlowered, as they sit in the imdb
    text, ln, st = check_text(slots, 128, 15, "golden")
    assert not st.any()
    for i, c in enumerate(cases):
        assert "".join(map(chr, text[i, :ln[i]])) == c["word_cleaner"], c["s"]
    check_text(slots, 128, 9, "golden")
    _, questions, _ = golden_wordpiece()
    for qs in (questions, fuzz_questions(2000, seed=9)):
        text, ln, st = check_question([q.encode() for q in qs], 1024, "questions")
        want = W.pack_question_text(qs, max_chars=1024)
        assert not st.any() and np.array_equal(text, want["question_text"].numpy()) and np.array_equal(ln, want["question_text_len"].numpy())


def boundary_strings():
    out = []
    for n in list(range(58, 67)) + list(range(122, 131)):          # raw lengths 62..67 and 126..131 and around: the sequence straddles byte 64 / 128
        for ch in ("é", "中", "\U0001D11E", "İ", "Σ", "É", "한", "豈", "́", " ", "¿"):
            out += ["x" * n + ch + "yz", "A" * n + ch, ch * (n // 2)]
    for pre in ("A", "A" * 23, "A" * 62, "A" * 63, "1", ""):      # the decision falls in a later chunk (40 marks are 80 bytes)
        for post in ("a", "", "1", " ", "Σ", "中", "́a", "Σa"):
            out += [pre + "Σ" + "́" * 40 + post, pre + "Σ" + "́" * 100 + post, pre + "Σ" + "\u00ad" * 31 + post]
    return out


def test_chunk_boundaries_text():
    slots = [s.encode() for s in boundary_strings()]
    lens = {len(b) for b in slots}
    assert set(range(62, 68)) | set(range(126, 132)) <= lens
    for L, mode in ((128, 15), (128, 1), (64, 9)):
        st = check_text(slots, L, mode, "boundaries")[2]
        assert (st == 0).any() and (st == T.STATUS_LONG).any()
    # U+0130 is the last character that still fits L (its two code points end at L), and the first that does not
    for L, n in ((8, 6), (128, 126), (65, 63), (2, 0)):
        text, ln, st = check_text([("x" * n + "İ").encode(), ("x" * (n + 1) + "İ").encode(), ("x" * n + "İ ").encode(), (" " + "x" * n + "İ").encode()], L, 15, "U+0130 at L")
        assert st.tolist() == [0, T.STATUS_LONG, 0, 0] and ln.tolist() == [L, 0, L, L] and text[0, L - 2:].tolist() == [0x69, 0x307]


def test_chunk_boundaries_question():
    strings = boundary_strings()
    strings += ["é" + "x" * n + tok + "y" for n in range(56, 64) for tok in W.SPECIAL_TOKENS]            # a special-token string straddles byte 64
    strings += ["é" + "x" * n + tok for n in (57, 58) for tok in ("[SEP", "[MASK", "[mask]", "[", "[PAD")]      # ... and what only looks like one, at the slot's end
    strings += ["a " + "́̂" * k + " b" for k in (1, 16, 31, 32, 33, 70)] + ["́" * 40, "́" * 40 + " a", "a " + "́" * 40, "中" + "́" * 33 + "文 " + "́" * 64 + "x"]
    strings += ["ab " * 21 + "é", " " * 64 + "é", "é" + " " * 70 + "a", "A\U000E0001" * 20 + "Σ" + "\U000E0001" * 20 + "a", "AΣ" + "\u00ad" * 30 + "a", "AΣ" + "\u00ad" * 30 + " a"]
    slots = [s.encode() for s in strings]
    st = check_question(slots, 1024, "boundaries")[2]
    assert (st == 8).sum() == 8 * len(W.SPECIAL_TOKENS) and (st == 0).sum() > 100
    st = check_question(slots, 64, "boundaries, Lq = 64")[2]
    assert (st == 2).any() and (st == 0).any()


@pytest.mark.parametrize("S", [1, 3, 64, 65])
def test_slot_counts_and_capacities(S):
    pool = [s for s in boundary_strings() if s][::7] + context_strings(200, seed=S) + ["", "a", "İ", "Σ", "AΣ", "中", "한", "́"]
    rng = np.random.RandomState(S)
    slots = [pool[i].encode() for i in rng.randint(0, len(pool), S)]
    for L in (1, 128):
        check_text(slots, L, 15, "S=%d L=%d" % (S, L))
    for Lq in (1, 1024):
        check_question(slots, Lq, "B=%d Lq=%d" % (S, Lq))
    long_q = "Ünï " * 255 + "Σοφός"                                 # 1025 code points after normalisation: flagged; its first 1023 characters pass
    check_question([long_q.encode(), long_q[:1023].encode(), ("é" * 1024).encode(), ("é" * 1025).encode(), b"a" * 1024, b"a" * 1025] * ((S + 5) // 6), 1024, "Lq limit")


def test_every_status_bit_between_clean_neighbours_with_guard_words():
    clean = "Café ΑΣ.".encode()                                      # (ends in an ASCII byte: the slot with bad offsets below hands it to its neighbour)
    t = device_table()
    # text: 1 not UTF-8 (a cut sequence; a stray continuation byte), 2 too long, 4 bad offsets
    slots = [clean, b"ab\xc3", clean, b"\x80ab", clean, ("İ" * 9).encode(), clean, b"zz", clean]
    raw, off = pack_bytes(slots)
    off = off.copy()
    off[8] = off[7] - 1                                             # slot 7 ends before it begins; slot 8 then starts there: both ranges stay inside raw
    L, S = 16, len(slots)
    big = torch.full((S * L + 64,), POISON, dtype=torch.int32, device="cuda")
    out = {"text": big[:S * L], "text_len": torch.full((S + 64,), POISON, dtype=torch.int32, device="cuda")[:S], "status": torch.empty(S, dtype=torch.int32, device="cuda")}
    ops.text_from_utf8(gpu(raw), gpu(off), L, 15, out=out, unicode=t)
    want = T.clean_host(raw, off, L, 15, table=table())
    assert want[2].tolist() == [0, 1, 0, 1, 0, 2, 0, 4, 0] and out["status"].cpu().tolist() == want[2].tolist()
    assert np.array_equal(out["text"].cpu().numpy().reshape(S, L), want[0]) and np.array_equal(out["text_len"].cpu().numpy(), want[1])
    assert (big[S * L:] == POISON).all() and "".join(map(chr, want[0][0, :want[1][0]])) == "café ας."
    # question: the same three, 8 a special token, 16 a code point for the host
    slots = [clean, b"ab\xc3", clean, "é[CLS]".encode(), clean, "a\u302eb".encode(), clean, "é" * 17, clean, b"zz", clean]
    slots = [s if isinstance(s, bytes) else s.encode() for s in slots]
    raw, off = pack_bytes(slots)
    off = off.copy()
    off[10] = off[9] - 1
    Lq, B = 16, len(slots)
    big = torch.full((B * Lq + 64,), POISON, dtype=torch.int32, device="cuda")
    out = {"question_text": big[:B * Lq], "question_text_len": torch.empty(B, dtype=torch.int32, device="cuda"), "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    ops.question_from_utf8(gpu(raw), gpu(off), Lq, t, out=out)
    want = W.question_text_host(raw, off, table(), max_chars=Lq)
    assert want[2].tolist() == [0, 1, 0, 8, 0, 16, 0, 2, 0, 4, 0] and out["status"].cpu().tolist() == want[2].tolist()
    assert np.array_equal(out["question_text"].cpu().numpy().reshape(B, Lq), want[0]) and np.array_equal(out["question_text_len"].cpu().numpy(), want[1])
    assert (big[B * Lq:] == POISON).all() and "".join(map(chr, want[0][0, :want[1][0]])) == "cafe ας."


def test_ascii_input_equals_the_ascii_entry_point_for_every_mode():
    rng = np.random.RandomState(4)
    alphabet = np.frombuffer(b"aAsSzZ',? \t\n.:x1", np.uint8)
    slots = [c["s"].encode() for c in load_golden()["cases"] if c["s"].isascii()] + [alphabet[rng.randint(0, alphabet.size, rng.randint(0, 140))].tobytes() for _ in range(300)]
    raw, off = pack_bytes(slots)
    g_raw, g_off = gpu(raw), gpu(off)
    for mode in range(16):
        a, b = ops.text_from_utf8(g_raw, g_off, 128, mode), ops.text_from_utf8(g_raw, g_off, 128, mode, unicode=device_table())
        for k in ops.TEXT_FROM_UTF8_KEYS:
            assert torch.equal(a[k], b[k]), (mode, k)


def test_both_op_routes_and_the_argument_errors(monkeypatch):
    slots = [s.encode() for s in ("Café Σ", "İ's", "ΟΔΟΣ 中")]
    raw, off = pack_bytes(slots)
    g_raw, g_off, t = gpu(raw), gpu(off), device_table()
    res = []
    for on in ("1", "0"):                                            # the torch ops, then the ctypes route
        monkeypatch.setenv("SAM_COARSE_OPS", on)
        res.append((ops.text_from_utf8(g_raw, g_off, 16, 15, unicode=t), ops.question_from_utf8(g_raw, g_off, 16, t)))
    for a, b in zip(res[0], res[1]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(_capi.SamHipError):
        ops.question_from_utf8(g_raw, g_off, 1025, t)
    with pytest.raises(_capi.SamHipError):
        ops.text_from_utf8(g_raw, g_off, 129, 15, unicode=t)
    with pytest.raises(_capi.SamHipError):
        ops.question_from_utf8(g_raw, g_off, 16, dict(t, block=t["block"][:-1].contiguous()))
    with pytest.raises(ValueError, match="sample 1.*status bit 8"):
        W.question_text_from_utf8(*[gpu(v.numpy()) for v in W.pack_question_utf8(["fine", "é [SEP]"]).values()], t)


def test_materialize_end_to_end():
    index, questions, ids = golden_wordpiece()
    B = 6
    tokens = [["CAFÉ", "STRAẞE,", "ΟΔΟΣ's", "İstanbul?", "£5"], ["Москва", "ΣΟΦΟΣ", "東京"], [], ["plain", "Ascii's"], ["Ǆ"], ["  ÉTÉ  "]]
    answers = [["Été, SÛR?", "ΟΔΟΣ"], ["İ", "ok"], ["Ж's", ""], ["x", "Y"], ["ΑΣ ΑΣ", "ß"], ["ÀÉ", "ς"]]
    qs = [q for q in questions if not q.isascii()][:3] + questions[:2] + ["Τι ΕΙΝΑΙ ΑΥΤΟΣ ο ΔΡΟΜΟΣ; 東京 Café"]
    t = device_table()
    po, pa, pq = T.pack_utf8(tokens, 5, host_lower=False), T.pack_utf8(answers, 2, host_lower=False), W.pack_question_utf8(qs)
    batch = {"ocr_raw": po["raw"].cuda(), "ocr_raw_off": po["raw_off"].cuda(), "ocr_count": po["count"].cuda(), "answer_raw": pa["raw"].cuda(),
             "answer_raw_off": pa["raw_off"].cuda(), "question_raw": pq["question_raw"].cuda(), "question_raw_off": pq["question_raw_off"].cuda()}
    assert T.has_raw(batch)
    got = T.materialize(dict(batch), ocr_chars=32, answer_chars=64, unicode=t, question_chars=256)
    assert not T.has_raw(got)
    # the host route: pack_utf8 with host lowering through the ASCII launch, and pack_question_text
    ho, ha = T.pack_utf8(tokens, 5), T.pack_utf8(answers, 2)
    host = T.materialize({"ocr_raw": ho["raw"].cuda(), "ocr_raw_off": ho["raw_off"].cuda(), "ocr_count": ho["count"].cuda(), "answer_raw": ha["raw"].cuda(),
                          "answer_raw_off": ha["raw_off"].cuda()}, ocr_chars=32, answer_chars=64)
    host.update({k: v.cuda() for k, v in W.pack_question_text(qs, max_chars=256).items()})
    for k in ("ocr_text", "ocr_text_len", "answer_text", "answer_text_len", "question_text", "question_text_len"):
        assert torch.equal(got[k], host[k]), k
    assert got["ocr_text"].shape == (B, 5, 32) and got["question_text"].shape == (B, 256)
    # and the reference's cleaner, directly
    for b in range(B):
        for i, s in enumerate(tokens[b]):
            n = int(got["ocr_text_len"][b, i])
            assert "".join(map(chr, got["ocr_text"][b, i, :n].tolist())) == s.lower().replace(",", "").replace("?", "").replace("'s", " 's").strip()
    # WordPiece ids from the materialised question text: the golden ids
    qg = [q.encode() for q in questions]
    raw, off = pack_bytes(qg)
    text, ln = W.question_text_from_utf8(gpu(raw), gpu(off), t, max_chars=1024)
    from sam_textvqa_amd import answers as A
    enc = {k: v.cpu() for k, v in W.from_text(text, ln, A.index_to(index, "cuda"), T=20).items()}
    for b, row in enumerate(ids):
        assert enc["question_indices"][b, :len(row)].tolist() == row and int(enc["num_question_tokens"][b]) == len(row), questions[b]
    # check=False returns the status tensors, the question's too
    _, status = T.materialize(dict(batch), ocr_chars=32, answer_chars=64, unicode=t, check=False)
    assert set(status) == {"ocr", "answer", "question"} and not any(bool(s.any()) for s in status.values())
    with pytest.raises(ValueError, match="materialize: sample 0.*status bit 2"):
        T.materialize(dict(batch), ocr_chars=32, answer_chars=64, unicode=t, question_chars=4)
