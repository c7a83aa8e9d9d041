"""CPU: the host side of the answer tables built from text (answers.pack_answer_text / vocab_index / vocab_lookup_host / tables_from_text_host, DESIGN.md
§3.15) -- the twin on packed text against build_answer_table + collate_answer_tables, the hash index against word2idx_dict, the splitter's whitespace set
against str.isspace over all code points, the packer's errors, the binding of include/sam_hip_answers.h and the entry point's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import phoc as P
from tests.test_answers_cpu import golden

SPECIALS = [A.PAD_TOKEN, A.BOS_TOKEN, A.EOS_TOKEN, A.UNK_TOKEN]


# ---------------------------------------------------------------------------------------------- shared with tests/test_answer_text_gpu.py
def pack(answers, tokens, No=50, Lw=32, La=128, A_=10):
    bd = A.pack_answer_text(answers, num_answers=A_, max_chars=La)
    bd.update(P.pack_ocr_text(tokens, max_ocr_tokens=No, max_chars=Lw))
    return bd


def host_tables(answers, tokens, voc, caps=A.DEFAULT_CAPS, No=50, A_=10, max_match_num=20):
    """(table, status) straight from the strings: build_answer_table + collate_answer_tables per sample, the status bit and zero rows where they raise"""
    caps = A.AnswerTableCaps(*caps)
    out = A._zero_tables(len(answers), caps)
    status = torch.zeros(len(answers), dtype=torch.int32)
    for b, (ans, tok) in enumerate(zip(answers, tokens)):
        try:
            one = A.collate_answer_tables([A.build_answer_table(ans, tok, voc, num_answers=A_, max_ocr_tokens=No, max_copy_steps=caps.L,
                                                                max_match_num=max_match_num)], caps)
        except A.AnswerTableError as e:
            status[b] = e.status
            continue
        for k in A.TABLE_KEYS:
            out[k][b] = one[k][0]
    return out, status


def golden_batch():
    """every case of tests/golden/answers.json, then the two on which the reference asserts"""
    meta, _ = golden()
    cases = meta["cases"] + meta["failing"]
    return A.AnswerVocab(meta["vocab"]), [c["answers"] for c in cases], [c["context_tokens"] for c in cases], len(meta["cases"])


def special_vocab():
    return A.AnswerVocab(SPECIALS + ["stop", "sign", "go", "a", "one", "two", "the", "tok"])          # 12 words


def special_batch():
    """B = 16 samples over the 12-word vocabulary, one per corner of the host rules (the names say which)"""
    S = {}
    S["vocab_and_three_slots"] = (["stop"] * 6 + ["stop sign"] * 4, ["stop", "x", "stop", "y", "stop", "sign"])
    S["product_24_is_cut"] = (["go tok"] * 10, ["go"] * 5 + ["tok"] * 3)                                  # (1 + 5) * (1 + 3)
    S["product_exactly_20"] = (["go tok"] * 7 + ["tok"] * 3, ["go"] * 4 + ["tok"] * 3)                    # (1 + 4) * (1 + 3)
    S["thirteen_words"] = ([" ".join(["one", "two"] * 6 + ["one"])] * 5 + ["one two"] * 5, ["two", "q"])
    S["sixty_four_words"] = ([" ".join(["a", "b"] * 32)] * 9 + ["b"], ["a", "b", "a"])                    # counts 3, 1, 3, ...: the product saturates
    S["ten_identical"] = (["the sign"] * 10, ["sign"])
    S["ten_distinct"] = (["stop", "sign", "go", "a", "one", "two", "the", "tok", "go stop", "nothing"], ["go", "the"])
    S["empty_and_blank_answers"] = (["", "  \t ", "go", "", "　", "go", "go", " go ", "\n", "go"], ["go"])
    S["other_whitespace"] = (["stop sign", "stop\tsign", " stop sign　", "\x1cstop\x1fsign", "stop sign", "stop​sign", "stop\x85sign",
                              "stop sign ", "stop sign ", "stop  sign"], ["sign", "stop​sign"])
    S["astral_code_points"] = (["stop \U0001F600", "\U0001F600", "\U00010000\U0010FFFF", "stop \U0001F601"] + ["\U0001F600 stop"] * 6,
                               ["\U0001F600", "\U00010000\U0010FFFF", "\U0001F600"])
    S["case_differs"] = (["Stop", "stop", "STOP", "Stop stop", "stop Stop"] * 2, ["Stop", "sTop"])
    S["unmatched_last_word"] = (["stop nowhere"] * 6 + ["go stop"] * 4, ["stop", "go"])
    S["no_ocr_tokens"] = (["stop", "go sign", "nowhere", "the the the", "stop"] * 2, [])
    S["unk_and_pad_at_step_0"] = (["<unk> go", "<pad>", "</s>", "<s> go", "go"] * 2, ["<pad>", "<unk>", "go"])
    S["fifty_tokens"] = (["tok go", "go tok", "t49", "t49 t0 t25", "tok"] * 2, ["t%d" % i for i in range(48)] + ["tok", "t49"])
    S["every_word_everywhere"] = (["a a a", "a a", "a", "a a a a"] * 2 + ["a one", "one a"], ["a"] * 7 + ["one"] * 2)
    assert len(S) == 16
    names = list(S)
    return special_vocab(), names, [S[n][0] for n in names], [S[n][1] for n in names]


def tiny_batch():
    """the smallest shapes at which the indexing can still go wrong: B = 1, A = 2, La = 9, No = 3, Lw = 5"""
    voc = A.AnswerVocab(SPECIALS + ["go", "big"])
    return voc, [["go big go", "big"]], [["go", "big", "go"]], dict(No=3, Lw=5, La=9, A_=2), A.AnswerTableCaps(40, 3, 8, 16)


def colliding_vocab():
    """V = 7, T = 16, with at least two words sharing a home slot (found by search): the probe has to walk"""
    for i in range(1000):
        words = SPECIALS + ["c%d" % i, "c%d" % (i + 1), "c%d" % (i + 2)]
        homes = [A.text_hash([ord(c) for c in w]) & 15 for w in words]
        if len(set(homes)) < len(homes) and len(set(homes[4:])) < 3:
            return A.AnswerVocab(words)
    raise AssertionError("no colliding triple among 1000 candidates")


def big_vocab(n=5000):
    return A.AnswerVocab(SPECIALS + ["w%d" % i for i in range(n - 4)])


def text_samples(batch_size, num_vocab=5000, n_ocr=50, seed=0):
    """answers.make_answer_tables' synthetic samples, as strings: (vocabulary, answers per sample, tokens per sample)"""
    rng = np.random.RandomState(seed)
    voc = big_vocab(num_vocab)
    answers, tokens = [], []
    for _ in range(batch_size):
        n_tok = rng.randint(1, n_ocr + 1)
        pool = ["w%d" % i for i in rng.randint(0, num_vocab - 4, 8)] + ["oov%d" % i for i in rng.randint(0, 40, 8)]
        toks = [pool[i] for i in rng.randint(0, len(pool), n_tok)]
        cands = []
        for _ in range(4):
            src = toks if rng.rand() < 0.6 else ["w%d" % i for i in rng.randint(0, num_vocab - 4, 3)]
            cands.append(" ".join(src[i] for i in rng.randint(0, len(src), rng.randint(1, 4))))
        cands.append("unmatched%d" % rng.randint(1000))
        answers.append([cands[i] for i in rng.choice(len(cands), 10, p=[0.4, 0.25, 0.15, 0.1, 0.1])])
        tokens.append(toks)
    return voc, answers, tokens


STATUS_CAPS = A.AnswerTableCaps(200, 12, 6, 7)


def status_batch():
    """one sample per status bit between clean neighbours, at capacities G = 6, E = 7; -> (voc, names, answers, tokens, expected status)"""
    clean = (["go tok"] * 10, ["tok"])                                      # groups go, tok, V+0, EOS; target indices 2 + 2 + 1
    S = [("clean0", clean, 0),
         ("seven_groups", (["go tok"] * 10, ["tok"] * 4), A.STATUS_GROUPS),                                  # go, tok, 4 slots, EOS
         ("clean1", clean, 0),
         ("eight_target_indices", (["go tok"] * 10, ["tok"] * 2), A.STATUS_EXTRA),                            # 5 groups; 3 + 2 + 2 + 1
         ("pad_slot_scored", (["go <pad>"] * 10, ["go", "<pad>"]), A.STATUS_PAD_SLOT),
         ("clean2", clean, 0),
         ("unk_scored", (["go <unk>"] * 10, ["go"]), A.STATUS_UNK_TARGET),
         ("pad_before_too_many_groups", (["go <pad>"] * 10, ["go", "<pad>", "go", "go", "go", "go"]), A.STATUS_PAD_SLOT),
         ("unk_then_pad", (["go <unk> <pad>"] * 10, ["<pad>"]), A.STATUS_UNK_TARGET),
         ("pad_then_unk", (["go <pad>"] * 5 + ["go <unk>"] * 5, ["<pad>"]), A.STATUS_PAD_SLOT),        # (the slot is first met before <unk> is)
         ("clean3", clean, 0)]
    return special_vocab(), [s[0] for s in S], [s[1][0] for s in S], [s[1][1] for s in S], torch.tensor([s[2] for s in S], dtype=torch.int32)


def assert_tables_equal(got, want, what=""):
    for k in A.TABLE_KEYS:
        assert got[k].dtype == want[k].dtype and tuple(got[k].shape) == tuple(want[k].shape), (what, k)
        assert torch.equal(got[k].cpu(), want[k].cpu()), (what, k)


def twin(bd, voc, caps=A.DEFAULT_CAPS):
    return A.tables_from_text_host(bd["answer_text"], bd["answer_text_len"], bd["ocr_text"], bd["ocr_text_len"], voc, caps)


# ---------------------------------------------------------------------------------------------- the host twin
def test_twin_on_the_packed_golden_cases_equals_the_host_functions():
    voc, answers, tokens, n_clean = golden_batch()
    table, status = twin(pack(answers, tokens), voc)
    want, want_status = host_tables(answers, tokens, voc)
    assert_tables_equal(table, want)
    assert torch.equal(status, want_status)
    assert status[:n_clean].eq(0).all() and status[n_clean:].tolist() == [A.STATUS_UNK_TARGET, A.STATUS_PAD_SLOT]
    for k in A.TABLE_KEYS:
        assert not table[k][n_clean:].any(), k                                             # the cases on which the reference asserts: zero rows
    assert table["meta"][:n_clean, 0].sum() > 0
    meta, _ = golden()
    assert table["dims"].tolist() == [meta["W"], voc.BOS_IDX, voc.EOS_IDX, 12]


def test_twin_on_the_constructed_batches_equals_the_host_functions():
    voc, names, answers, tokens = special_batch()
    table, status = twin(pack(answers, tokens), voc)
    want, want_status = host_tables(answers, tokens, voc)
    assert_tables_equal(table, want)
    assert torch.equal(status, want_status) and not status.any()
    n = dict(zip(names, table["meta"][:, 0].tolist()))
    assert n["product_24_is_cut"] == 200 and n["product_exactly_20"] == 7 * 20 + 3 * 4 and n["sixty_four_words"] == 9 * 20 + 1
    assert n["unmatched_last_word"] == 4 * 2 * 2 and n["thirteen_words"] == 5 * 20 + 5 * 2 and n["no_ocr_tokens"] == 8
    assert table["seq_len"][names.index("thirteen_words"), 0] == 12 and table["seq_len"][names.index("sixty_four_words"), 0] == 12
    voc, answers, tokens, shp, caps = tiny_batch()
    table, status = twin(pack(answers, tokens, **shp), voc, caps)
    want, want_status = host_tables(answers, tokens, voc, caps, No=shp["No"], A_=shp["A_"])
    assert_tables_equal(table, want)
    assert not status.any() and table["meta"][0, 0] > 0 and table["seq_len"].max() == 3       # "go big go": as long as L


def test_twin_reports_each_status_bit_and_leaves_the_neighbours_alone():
    voc, names, answers, tokens, expect = status_batch()
    table, status = twin(pack(answers, tokens), voc, STATUS_CAPS)
    assert status.tolist() == expect.tolist(), dict(zip(names, status.tolist()))
    want, _ = host_tables(answers, tokens, voc, STATUS_CAPS)
    assert_tables_equal(table, want)
    for b, st in enumerate(expect.tolist()):
        assert bool(table["meta"][b].any()) == (st == 0), names[b]
    assert A.status_message(status.tolist(), A.vocab_index(voc), STATUS_CAPS).startswith("sample 1: more score-index groups than the capacity G = 6")
    assert A.status_message([0, 0], A.vocab_index(voc), STATUS_CAPS) is None


# ---------------------------------------------------------------------------------------------- the vocabulary index
def near_misses(w):
    out = [w[:-1], w + "x", w.swapcase(), w.upper()]
    if w:
        out += [chr(ord(w[0]) + 1) + w[1:], w[:-1] + chr(ord(w[-1]) ^ 1), w[:len(w) // 2] + "é" + w[len(w) // 2 + 1:]]
    return out


@pytest.mark.parametrize("which", ["golden", "synthetic5000", "colliding7"])
def test_vocab_lookup_host_agrees_with_word2idx(which):
    voc = {"golden": lambda: golden_batch()[0], "synthetic5000": big_vocab, "colliding7": colliding_vocab}[which]()
    index = A.vocab_index(voc)
    V, T = len(voc), index["slots"].numel()
    assert index["V"] == V and (index["UNK"], index["BOS"], index["EOS"]) == (voc.UNK_IDX, voc.BOS_IDX, voc.EOS_IDX)
    assert T & (T - 1) == 0 and 2 * V <= T < 4 * V + 2 and sorted(index["slots"][index["slots"] >= 0].tolist()) == list(range(V))
    if which == "colliding7":
        assert (V, T) == (7, 16)
        homes = [A.text_hash([ord(c) for c in w]) & (T - 1) for w in voc.word_list]
        assert len(set(homes)) < V
        displaced = [i for i, h in enumerate(homes) if int(index["slots"][h]) != i]
        assert displaced                                                                        # a word that is not in its home slot
    for i, w in enumerate(voc.word_list):
        assert A.vocab_lookup_host(index, [ord(c) for c in w]) == i == voc.word2idx_dict[w]
    words = voc.word_list if V < 100 else voc.word_list[::37]
    for w in words:
        for m in near_misses(w):
            assert A.vocab_lookup_host(index, [ord(c) for c in m]) == voc.word2idx_dict.get(m, -1), (w, m)
    for m in ["", "zzz", "unknown", "w", "w50000", "x" * 33, "\U0001F600"]:
        assert A.vocab_lookup_host(index, [ord(c) for c in m]) == voc.word2idx_dict.get(m, -1), m
    with pytest.raises(ValueError, match="over max_word"):
        A.vocab_index(A.AnswerVocab(SPECIALS + ["abcdef"]), max_word=5)
    with pytest.raises(ValueError, match="max_word"):
        A.vocab_index(voc, max_word=65)


def test_whitespace_set_is_str_isspace_over_all_code_points():
    assert A.WHITESPACE == {c for c in range(sys.maxunicode + 1) if chr(c).isspace()}
    assert all(("a%sb" % chr(c)).split() == ["a", "b"] for c in A.WHITESPACE)
    csrc = os.path.join(os.path.dirname(A.__file__), "csrc")
    defs = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    assert [f for f, s in defs.items() if "bool is_space(" in s] == ["text.h"] and not [f for f, s in defs.items() if "bool is_ws(" in s]   # one definition, one name
    src = defs["text.h"]
    body = src[src.index("bool is_space(int c)"):]
    body = body[:body.index("}")]
    import re
    listed = set()
    for lo, hi in re.findall(r"c >= (0x[0-9A-Fa-f]+) && c <= (0x[0-9A-Fa-f]+)", body):
        listed |= set(range(int(lo, 16), int(hi, 16) + 1))
    listed |= {int(v, 16) for v in re.findall(r"c == (0x[0-9A-Fa-f]+)", body)}
    assert listed == A.WHITESPACE                                                              # the kernel's list, read from its source


# ---------------------------------------------------------------------------------------------- the packer
def test_packer_packs_exact_code_points_and_names_what_does_not_fit():
    bd = A.pack_answer_text([["Stop \U0001F600", ""], ["a", "b c"]], num_answers=2, max_chars=7)
    assert bd["answer_text"].dtype == torch.int32 and tuple(bd["answer_text"].shape) == (2, 2, 7) and tuple(bd["answer_text_len"].shape) == (2, 2)
    assert bd["answer_text_len"].tolist() == [[6, 0], [1, 3]]
    assert bd["answer_text"][0, 0].tolist() == [ord("S"), ord("t"), ord("o"), ord("p"), 32, 0x1F600, 0]
    with pytest.raises(ValueError, match="no samples"):
        A.pack_answer_text([])
    with pytest.raises(ValueError, match="sample 1: expected 2 answers, got 3"):
        A.pack_answer_text([["a", "b"], ["a", "b", "c"]], num_answers=2)
    with pytest.raises(ValueError, match="sample 1: expected 2 answers, got 1"):
        A.pack_answer_text([["a", "b"], ["a"]], num_answers=2)
    with pytest.raises(ValueError, match=r"sample 0: answer 1 \('abcdefgh'\) has 8 code points, over max_chars = 7"):
        A.pack_answer_text([["a", "abcdefgh"]], num_answers=2, max_chars=7)
    with pytest.raises(ValueError, match="max_chars"):
        A.pack_answer_text([["a"]], num_answers=1, max_chars=129)
    with pytest.raises(ValueError, match="max_chars"):
        A.pack_answer_text([["a"]], num_answers=1, max_chars=0)
    with pytest.raises(ValueError, match="num_answers"):
        A.pack_answer_text([[]], num_answers=0)
    assert A.pack_answer_text([["x" * 128]], num_answers=1)["answer_text_len"].tolist() == [[128]]


def test_key_combinations_that_cannot_be_served_raise():
    bd = pack([["a"] * 10], [["a"]])
    assert A.check_answer_text(bd) and not A.check_answer_text({"ocr_text": bd["ocr_text"]})
    for drop in A.ANSWER_TEXT_KEYS:
        with pytest.raises(ValueError, match="without"):
            A.check_answer_text({k: v for k, v in bd.items() if k != drop})
    for extra in ("answer_table", "targets"):
        with pytest.raises(ValueError, match=extra):
            A.check_answer_text(dict(bd, **{extra: None}))
    for drop in ("ocr_text", "ocr_text_len"):
        with pytest.raises(ValueError, match="without " + drop):
            A.check_answer_text({k: v for k, v in bd.items() if k != drop})


# ---------------------------------------------------------------------------------------------- the binding and the entry point
def test_the_entry_point_is_bound_from_its_header_and_the_other_tables_are_untouched():
    from ctypes import c_float, c_int, c_int64, c_uint, c_double, c_void_p as vp
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    i = c_int
    assert _capi.HEADER_SIGNATURES["answers"] == {"sam_answer_table_from_text": [vp, c_int64, vp, vp, c_int64, vp, vp, c_int64, vp, vp] + [i] * 15 + [vp] * 10}
    assert _capi.HEADER_RESTYPES["answers"] == {"sam_answer_table_from_text": c_int}
    assert "sam_answer_table_from_text" not in _capi.SIGNATURES and "sam_answer_table_from_text" not in _capi.NO_STATUS
    assert _capi.HEADER_SIGNATURES["text"] == {"sam_phoc_from_text": [vp, c_int64, vp, vp, i, i, i, vp, c_int64, i, i, i, c_float, vp]}
    assert _capi.HEADER_SIGNATURES["pipeline"] == {"sam_mask_bits_from_boxes": [vp, vp, c_int64, i, vp, c_int64, i, i, i, i, i, i, i, i, c_double, c_uint, vp, vp]}
    assert len(_capi.SIGNATURES) == 77
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_answer_table_from_text.argtypes == _capi.HEADER_SIGNATURES["answers"]["sam_answer_table_from_text"] and l.sam_answer_table_from_text.restype is c_int
    assert os.path.join(b.CSRC, "answer_text.hip") in b.sources()
    assert '#include "sam_hip.h"' in open(b.HEADERS["answers"]).read()


def test_digest_covers_the_answers_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_answers.h"
    other.write_text(open(b.HEADERS["answers"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "answers", str(other))
    assert b._digest() != was


# never dereferenced: every case below is rejected by the argument checks, before any device call
OK = dict(answer_text=1 << 16, ld_answer=128, answer_len=1 << 16, ocr_text=1 << 16, ld_ocr=32, ocr_len=1 << 16, vocab_cp=1 << 16, ld_vocab=32, vocab_len=1 << 16,
          slots=1 << 16, B=2, A=10, La=128, No=50, Lw=32, V=12, Lv=32, T=32, unk=3, eos=2, S=200, L=12, G=64, E=256, M=20, meta=1 << 16, seq_len=1 << 16,
          seq_grp=1 << 16, step0_idx=1 << 16, step0_val=1 << 16, grp_idx=1 << 16, grp_off=1 << 16, grp_extra=1 << 16, status=1 << 16)
POINTERS = ("answer_text", "answer_len", "ocr_text", "ocr_len", "vocab_cp", "vocab_len", "slots", "meta", "seq_len", "seq_grp", "step0_idx", "step0_val", "grp_idx",
            "grp_off", "grp_extra", "status")
REJECTED = [("null " + p, {p: None}, "ARG", "null") for p in POINTERS] + [
    ("B = 0", dict(B=0), "ARG", "bad shape"), ("A = 0", dict(A=0), "ARG", "bad shape"), ("No = 0", dict(No=0), "ARG", "bad shape"),
    ("La = 0", dict(La=0, ld_answer=0), "ARG", "La=0"), ("La = 129", dict(La=129, ld_answer=129), "ARG", "La=129"),
    ("Lw = 0", dict(Lw=0), "ARG", "Lw=0"), ("Lw = 65", dict(Lw=65, ld_ocr=65), "ARG", "Lw=65"),
    ("Lv = 0", dict(Lv=0), "ARG", "Lv=0"), ("Lv = 65", dict(Lv=65, ld_vocab=65), "ARG", "Lv=65"),
    ("T not a power of two", dict(T=48), "ARG", "power of two"), ("T < 2 V", dict(T=16), "ARG", "power of two"), ("V = 0", dict(V=0), "ARG", "power of two"),
    ("unk outside the vocabulary", dict(unk=12), "ARG", "unk=12"), ("eos equals unk", dict(eos=3), "ARG", "eos=3"),
    ("L = 0", dict(L=0), "ARG", "L=0"), ("max_match_num = 0", dict(M=0), "ARG", "max_match_num=0"),
    ("S < A * max_match_num", dict(S=199), "ARG", "S >= A * max_match_num"),
    ("G = 0", dict(G=0), "ARG", "G=0"), ("G over int16", dict(G=32768), "ARG", "G=32768"), ("E = 0", dict(E=0), "ARG", "E=0"),
    ("ld_answer < La", dict(ld_answer=127), "ARG", "ld_answer"), ("ld_ocr < Lw", dict(ld_ocr=31), "ARG", "ld_ocr"), ("ld_vocab < Lv", dict(ld_vocab=31), "ARG", "ld_vocab"),
    ("misaligned text", dict(answer_text=(1 << 16) + 2), "ARG", "misaligned"), ("misaligned seq_grp", dict(seq_grp=(1 << 16) + 1), "ARG", "misaligned"),
    ("65 OCR slots", dict(No=65), "UNSUPPORTED", "64 OCR slots"), ("256 answers", dict(A=256, S=5120), "UNSUPPORTED", "255 answers"),
    ("too much LDS", dict(S=4000, M=400), "UNSUPPORTED", "LDS"), ("L overflows the carve", dict(L=1 << 30), "UNSUPPORTED", "LDS"),
]


def _args(a):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return (p(a["answer_text"]), a["ld_answer"], p(a["answer_len"]), p(a["ocr_text"]), a["ld_ocr"], p(a["ocr_len"]), p(a["vocab_cp"]), a["ld_vocab"], p(a["vocab_len"]),
            p(a["slots"]), a["B"], a["A"], a["La"], a["No"], a["Lw"], a["V"], a["Lv"], a["T"], a["unk"], a["eos"], a["S"], a["L"], a["G"], a["E"], a["M"],
            *[p(a[k]) for k in POINTERS[7:]], None)


@pytest.mark.parametrize("name,change,code,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_argument_rejections_come_before_any_device_call(name, change, code, word):
    from sam_textvqa_amd import _capi
    rc = _capi.lib().sam_answer_table_from_text(*_args(dict(OK, **change)))
    assert rc == _capi.CONSTANTS["SAM_ERR_" + code] == {"ARG": -1, "UNSUPPORTED": -2}[code], name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_answer_table_from_text:") and word in msg, msg
    with pytest.raises(_capi.SamHipError, match="sam_answer_table_from_text"):
        _capi.call("sam_answer_table_from_text", *_args(dict(OK, **change)))


def test_ops_wrapper_rejects_cpu_tensors():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    voc = special_vocab()
    bd = pack([["go"] * 10], [["go"]])
    out = A._zero_tables(1, A.DEFAULT_CAPS)
    out["status"] = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(SamHipError):                                                           # CPU tensors: rejected, no fallback
        ops.answer_table_from_text(bd["answer_text"], bd["answer_text_len"], bd["ocr_text"], bd["ocr_text_len"], A.vocab_index(voc), out)
