"""GPU: raw UTF-8 strings to cleaned code points (csrc/textprep.hip, sam_text_from_utf8) against its host twin textprep.clean_host, bit
for bit in text (padding included), text_len and status -- the twin itself is held against the reference-written golden and bytes.decode by
tests/test_textprep_cpu.py.  The shapes are the smallest at which the kernel can go wrong: slot counts and capacities around the wave width, raw lengths
around the 64-byte chunk, code points / possessives / white space across chunk boundaries, slots that end inside a sequence next to slots that begin
with continuation bytes; then guard words, both op routes, and materialize in front of the answer tables, the score tables and PHOC."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi
from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops
from sam_textvqa_amd import phoc as P
from sam_textvqa_amd import textprep as T
from tests.test_textprep_cpu import load_golden, pack_bytes, random_byte_slots, raw_batch, word_cleaner

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A


def launch(raw, off, L, mode):
    out = ops.text_from_utf8(torch.from_numpy(np.array(raw)).cuda(), torch.from_numpy(np.array(off)).cuda(), L, mode)          # (copies: frombuffer arrays are read-only)
    return tuple(out[k].cpu().numpy() for k in ops.TEXT_FROM_UTF8_KEYS)


def check(slots, L, mode, what=""):
    """one launch over `slots` (a list of bytes) equals the twin in all three outputs; -> the status vector"""
    raw, off = pack_bytes(slots)
    got, want = launch(raw, off, L, mode), T.clean_host(raw, off, L, mode)
    for k, g, w in zip(ops.TEXT_FROM_UTF8_KEYS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, L, mode, bad[:4].tolist(), slots[bad[0][0]][:80], g[bad[0][0]].tolist()[:12], w[bad[0][0]].tolist()[:12])
    return want[2]


@pytest.mark.parametrize("mode", [15, 9, 0, 6])
def test_golden_strings(mode):
    slots = [(c["s"] if mode == 0 else (c["s"] if c["s"].isascii() else c["s"].lower())).encode() for c in load_golden()["cases"]]
    st = check(slots, 128, mode, "golden")
    assert not st.any()
    if mode in (15, 9):                                # and the reference's own words, without the twin in between
        key = "word_cleaner" if mode == 15 else "word_cleaner_lower"
        raw, off = pack_bytes(slots)
        text, ln, _ = launch(raw, off, 128, mode)
        for i, c in enumerate(load_golden()["cases"]):
            assert "".join(map(chr, text[i, :ln[i]])) == c[key], c["s"]
    assert (check(slots, 8, mode, "golden, L = 8") == T.STATUS_LONG).any()


@pytest.mark.parametrize("S", [1, 63, 64, 65])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 128])
def test_slot_counts_and_capacities(S, L):
    rng = np.random.RandomState(S * 131 + L)
    alphabet = list("aAsS',? \t") + ["é", "中", "\U0001f600", "　"]
    slots = []
    for s in range(S):
        n = (0, 1, L - 1, L, L + 1, L + 2)[s % 6] if s < 12 else rng.randint(0, L + 3)
        slots.append("".join(alphabet[i] for i in rng.randint(0, len(alphabet), max(n, 0))).encode())
    slots[S // 2] = b"a" * L                            # exactly L: passes
    for mode in (15, 0):
        st = check(slots, L, mode, "S=%d" % S)
        assert st[S // 2] == 0
    if S > 1:
        grown = list(slots)
        grown[0], grown[-1] = b"a" * (L + 1), (b"x's" + b"a" * L)[:L]          # L + 1: flagged; L raw code points growing past L through the possessive
        st = check(grown, L, 15, "grown")
        assert st[0] == T.STATUS_LONG and (st[-1] == T.STATUS_LONG or L < 3)


def test_empty_slots_first_last_adjacent_and_between_full_ones():
    full = b"Joe's, bar?" * 5
    for slots in ([b"", full, full], [full, full, b""], [full, b"", b"", full], [full, b"", full], [b""], [b"", b""], [b"", b"", full, b"", b""]):
        for mode in (15, 0):
            st = check(slots, 64, mode, "empties")
            assert not st.any()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 1000])
def test_raw_lengths_around_the_chunk(n):
    body = ("It's Joe's, isn't it? " * 60).encode()[:n]
    multi = ("é中\U0001f600's " * 200).encode()
    multi = multi[:n] if multi[:n].decode(errors="ignore").encode() == multi[:n] else multi[:n].decode(errors="ignore").encode()
    deleted = (b",?" * n)[:n - 2] + b"ok"               # n bytes, two code points left
    slots = [body, multi, deleted, b"a" * n, b" " * n, b"'" * n, (b"'s" * n)[:n]]
    for L in (128, 64):
        for mode in (15, 9, 0):
            check(slots, L, mode, "n=%d" % n)


def test_code_points_across_every_chunk_boundary_at_every_byte_split():
    slots = []
    for boundary in (64, 128):
        for ch in ("é", "中", "\U0001f600", "　"):
            e = ch.encode()
            for split in range(0, len(e) + 1):          # `split` bytes of the code point sit in front of the boundary
                slots.append(b"a" * (boundary - split) + e + b"z")
                slots.append(b" " * (boundary - split) + e + b" ")
                slots.append(b"a" * (boundary - split) + e)          # ... and the slot ends with it
                slots.append(b"a" * (boundary - split) + e[:-1])     # ... or inside it: flagged
    st = check(slots, 128, 15, "straddle")
    assert (st == T.STATUS_UTF8).sum() == len(slots) // 4 and (st == 0).sum() * 4 >= len(slots)
    check(slots, 128, 0, "straddle verbatim")


def test_possessive_across_the_chunk_boundary():
    slots = []
    for boundary in (64, 128):
        a = b"x" * (boundary - 1)
        slots += [a + b"'s", a + b"'S", a + b"'", a + b"'x", a + b"'?s", a + b"',?,s z", a[:-1] + b"'?s", a[:-1] + b"'?" + b",s",
                  a + b"'" + b"?" * 64 + b"s", a + b"'" + b"?" * 130 + b"s", a + b"'" + b"?" * 64, a + b"'" + b"?" * 64 + b"x", a + b"''s", a[:-1] + b"''s",
                  a + b"'" + b"," * 63 + b"'s", b" " * (boundary - 1) + b"'s", b" " * (boundary - 1) + b"'" + b"?" * 70 + b"s ", b"," * (boundary - 1) + b"'s",
                  a + b"'\xc5\x9b", a + b"'s's's", b"'s" * boundary]
    for L in (128, 67):
        for mode in (15, 4, 6, 12):
            check(slots, L, mode, "possessive")
    st = check([b"x" * 63 + b"'s"], 66, 15)
    assert st.tolist() == [0]
    assert check([b"x" * 63 + b"'s"], 65, 15).tolist() == [T.STATUS_LONG]


def test_more_than_one_chunk_of_leading_and_trailing_white_space():
    ws = "".join(chr(c) for c in load_golden()["whitespace"])
    slots = [b" " * 150 + b"ab's" + b" " * 200, (ws * 6 + "x y" + ws * 6).encode(), ("　" * 50 + "Q" + "　" * 50).encode(), b"\t" * 64 + b"a" + b"\n" * 64,
             b" " * 64, b" " * 129, b" " * 63 + b"a", b"a" + b" " * 63, b"a" + b" " * 63 + b"b", b"a" + b" " * 200 + b"b" + b" " * 200, b" " * 128 + b"'s" + b" " * 128,
             b"a" * 128 + b" " * 300]
    for mode in (15, 9, 8):
        st = check(slots, 128, mode, "white space")
        assert st[-1] == 0                               # trailing blanks past the capacity are not an overflow
    check(slots, 128, 0, "white space kept")
    for c in load_golden()["whitespace"]:                # every white-space code point, at both ends and in the middle
        w = chr(c)
        assert not check([(w + "Ab" + w + "Cd" + w).encode(), (w * 70 + "x" + w * 70).encode()], 16, 15, hex(c)).any()


def test_a_truncated_lead_is_not_completed_by_the_neighbours_bytes():
    slots = [b"ab\xe4", b"\xb8\xadxy", b"ok", b"\xf0\x9f", b"\x98\x80", b"\xc3", b"\xa9", b"fine"]
    st = check(slots, 16, 15, "neighbours")
    assert st.tolist() == [1, 1, 0, 1, 1, 1, 1, 0]
    assert b"".join(slots[:2]).decode() == "ab中xy"      # the bytes would decode if the boundary were ignored
    long = [b"a" * 63 + b"\xe4", b"\xb8\xad" + b"b" * 70, b"a" * 127 + b"\xf0\x9f\x98", b"\x80"]
    assert check(long, 128, 0, "neighbours, at the chunk's end").tolist() == [1, 1, 1, 1]


def test_fuzz():
    rng = np.random.RandomState(11)
    slots = random_byte_slots(3000, 5)
    texts = [c["s"] for c in load_golden()["cases"] if c["s"]]
    for i in range(1000):
        t = "".join(texts[j] for j in rng.randint(0, len(texts), rng.randint(1, 12))).encode()
        if i % 3 == 0:
            t = bytearray(t)
            t[rng.randint(len(t))] = rng.randint(256)
        slots.append(bytes(t))
    order = rng.permutation(len(slots))
    slots = [slots[i] for i in order]
    st = check(slots, 64, 15, "fuzz")
    assert min((st == 0).sum(), (st == 1).sum()) > 500 and (st == 2).sum() > 20
    check(slots, 128, 0, "fuzz verbatim")


def test_guard_words_and_poisoned_outputs():
    slots = [c["s"].encode() for c in load_golden()["cases"][:70]] + [b"\xff", b"a" * 200]
    raw, off = pack_bytes(slots)
    S, L, G = len(slots), 65, 16
    buf = torch.full((G + S * L + G + S + G + S + G,), POISON, dtype=torch.int32, device="cuda")
    a = G
    views = {}
    for k, n in (("text", S * L), ("text_len", S), ("status", S)):
        views[k] = buf[a: a + n]
        a += n + G
    out = ops.text_from_utf8(torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(off).cuda(), L, 15, out=views)
    want = T.clean_host(raw, off, L, 15)
    for k, w in zip(ops.TEXT_FROM_UTF8_KEYS, want):
        np.testing.assert_array_equal(out[k].cpu().numpy().reshape(w.shape), w, err_msg=k)          # (no poison survives: it is no expected value)
    host = buf.cpu().numpy()
    guards = np.ones(host.size, bool)
    a = G
    for n in (S * L, S, S):
        guards[a: a + n] = False
        a += n + G
    assert guards.sum() == 4 * G and (host[guards] == POISON).all()


def test_bad_offsets_flag_the_slot_and_bad_arguments_fail_the_call():
    raw = np.frombuffer(b"hello world", np.uint8)
    off = np.array([0, 5, 3, 11, 11, 12, 11], np.int32)
    text, ln, st = launch(raw, off, 8, 0)
    w = T.clean_host(raw, off, 8, 0)
    assert st.tolist() == w[2].tolist() == [0, 4, 0, 0, 4, 4] and np.array_equal(text, w[0]) and np.array_equal(ln, w[1])
    assert launch(raw, np.array([-3, 4], np.int32), 8, 0)[2].tolist() == [4]
    assert launch(np.zeros(0, np.uint8), np.array([0, 0, 0], np.int32), 8, 15)[2].tolist() == [0, 0]          # no bytes at all
    g_raw, g_off = torch.from_numpy(raw.copy()).cuda(), torch.tensor([0, 11], dtype=torch.int32, device="cuda")
    out = {k: torch.empty(256, dtype=torch.int32, device="cuda") for k in ops.TEXT_FROM_UTF8_KEYS}
    for L, mode in ((0, 0), (129, 0), (8, 16), (8, -1)):
        with pytest.raises(_capi.SamHipError):
            ops.text_from_utf8(g_raw, g_off, L, mode)
        with pytest.raises(_capi.SamHipError):           # the launcher's own checks, behind the wrapper's
            _capi.call("sam_text_from_utf8", _capi.ptr(g_raw), 11, _capi.ptr(g_off), 1, L, mode, _capi.ptr(out["text"]), _capi.ptr(out["text_len"]),
                       _capi.ptr(out["status"]), _capi.stream_handle())
    with pytest.raises(_capi.SamHipError):
        _capi.call("sam_text_from_utf8", _capi.ptr(g_raw), -1, _capi.ptr(g_off), 1, 8, 0, _capi.ptr(out["text"]), _capi.ptr(out["text_len"]), _capi.ptr(out["status"]),
                   _capi.stream_handle())
    with pytest.raises(_capi.SamHipError):
        ops.text_from_utf8(g_raw.cpu(), g_off, 8, 0)


def test_both_op_routes_agree(monkeypatch):
    slots = random_byte_slots(300, 9) + [c["s"].encode() for c in load_golden()["cases"]]
    raw, off = pack_bytes(slots)
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("SAM_COARSE_OPS", route)
        out[route] = launch(raw, off, 64, 15)
    direct = {k: torch.full(n, POISON, dtype=torch.int32, device="cuda") for k, n in (("text", (len(slots), 64)), ("text_len", (len(slots),)), ("status", (len(slots),)))}
    torch.ops.sam_hip.text_from_utf8(torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(off).cuda(), 64, 15, direct["text"], direct["text_len"], direct["status"])
    for i, k in enumerate(ops.TEXT_FROM_UTF8_KEYS):
        np.testing.assert_array_equal(out["1"][i], out["0"][i], err_msg=k)
        np.testing.assert_array_equal(out["1"][i], direct[k].cpu().numpy(), err_msg=k)


def test_check_names_the_first_flagged_slot():
    raw, off = pack_bytes([b"fine", b"a" * 9, b"\xff"])
    g_raw, g_off = torch.from_numpy(raw.copy()).cuda(), torch.from_numpy(off).cuda()
    with pytest.raises(ValueError, match=r"slot 1 has more than L = 8 code points after cleaning \(status bit 2\)"):
        T.text_from_utf8(g_raw, g_off, 8, 15)
    text, ln, st = T.text_from_utf8(g_raw, g_off, 8, 15, check=False)
    assert st.tolist() == [0, 2, 1] and ln.tolist() == [4, 0, 0] and not text[1:].any().item()
    text, ln = T.text_from_utf8(g_raw[:4], g_off[:2], 8, 15)
    assert text.tolist() == [[102, 105, 110, 101, 0, 0, 0, 0]] and ln.tolist() == [4]


def test_materialize_in_front_of_the_text_kernels():
    B, No, A_, Lw = 3, 50, 10, M.DEFAULT_SCORE_CAPS.Lw
    voc, _, _ = M.make_score_text(B, num_vocab=120, n_ocr=No, seed=0, rich=True)
    raw_answers, raw_tokens = raw_batch(B)
    host = dict(P.pack_ocr_text([[word_cleaner(t) for t in tok] for tok in raw_tokens], No))
    host.update(A.pack_answer_text([[word_cleaner(a) for a in ans] for ans in raw_answers], A_))
    host = {k: v.cuda() for k, v in host.items()}
    po, pa = T.pack_utf8(raw_tokens, No), T.pack_utf8(raw_answers, A_)
    counts = po["count"].cuda()
    batch = {"ocr_raw": po["raw"].cuda(), "ocr_raw_off": po["raw_off"].cuda(), "ocr_count": counts, "answer_raw": pa["raw"].cuda(), "answer_raw_off": pa["raw_off"].cuda(),
             "question_id": torch.arange(B)}
    assert T.materialize(batch, ocr_chars=Lw) is batch
    assert set(batch) == {"ocr_text", "ocr_text_len", "answer_text", "answer_text_len", "question_id"}          # raw keys gone; not a ragged batch: no ocr_count
    for k in host:
        assert batch[k].dtype == host[k].dtype and batch[k].shape == host[k].shape and torch.equal(batch[k], host[k]), k
    index = A.index_to(A.vocab_index(voc), "cuda")
    (ta, sa), (tb, sb) = A.tables_from_text(batch, index, check=False), A.tables_from_text(host, index, check=False)
    assert torch.equal(sa, sb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    (ta, sa), (tb, sb) = M.score_tables_from_text(batch, counts=counts, check=False), M.score_tables_from_text(host, counts=counts, check=False)
    assert torch.equal(sa, sb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert torch.equal(P.phoc_from_text(batch["ocr_text"], batch["ocr_text_len"], counts), P.phoc_from_text(host["ocr_text"], host["ocr_text_len"], counts))
    # a ragged batch keeps ocr_count; check=False hands the status words back; a flagged slot is named
    rb = {"ocr_raw": po["raw"].cuda(), "ocr_raw_off": po["raw_off"].cuda(), "ocr_count": counts, "obj_count": counts}
    rb2, st = T.materialize(rb, ocr_chars=Lw, check=False)
    assert rb2 is rb and "ocr_count" in rb and set(st) == {"ocr"} and not st["ocr"].any().item() and torch.equal(rb["ocr_text"], host["ocr_text"])
    with pytest.raises(ValueError, match=r"materialize: ocr slot \d+ has more than L = 2 code points"):
        T.materialize({"ocr_raw": po["raw"].cuda(), "ocr_raw_off": po["raw_off"].cuda(), "ocr_count": counts}, ocr_chars=2)
    # clean_answers = False: the answers' exact code points
    pv = T.pack_utf8(raw_answers, A_, lower=False)
    vb = T.materialize({"answer_raw": pv["raw"].cuda(), "answer_raw_off": pv["raw_off"].cuda(), "ocr_text": host["ocr_text"], "ocr_text_len": host["ocr_text_len"]},
                       clean_answers=False)
    verb = A.pack_answer_text(raw_answers, A_)
    assert torch.equal(vb["answer_text"].cpu(), verb["answer_text"]) and torch.equal(vb["answer_text_len"].cpu(), verb["answer_text_len"])
