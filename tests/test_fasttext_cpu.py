"""CPU (no GPU needed): FastText vectors of the OCR tokens from their text (sam_textvqa_amd/fasttext.py, include/sam_hip_fasttext.h) -- the hash against
the published FNV-1a vectors, the n-gram order against hand-written lists, the host twins case by case, the model file's round trip and refusals, the word
index, the batch rules, and every argument rejection of sam_fasttext_from_text, which happens before any device call.
The fastText library and a model file are not part of this repository's environment: nothing here (or anywhere in the suite) compares with the library."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

f32 = np.float32
LONG = "pneumonoultramicroscopicsilicovolcanoconiosis"          # 45 code points: over the index width of 32
WORDS = ["the", "The", "</s>", "stop", "a", "café", "日本語", "😀", "naïve", "é€😀", "b", "st", "within", LONG, b"\xff\xfe", b"caf\xc3", b"\xed\xa0\x80", b"\xc0\xaf"]


@functools.lru_cache(maxsize=None)
def toy_model(bucket=64, minn=3, maxn=6, dim=300, seed=0):
    """40 words (valid and invalid UTF-8, one over the index width) and a matrix whose magnitudes spread over 2^-12 .. 2^12 with mixed signs, so that the
    order of the fp32 adds shows in the bits; built once per argument set, never written to"""
    from sam_textvqa_amd import fasttext as FT
    words = WORDS + ["w%d" % i for i in range(40 - len(WORDS))]
    rng = np.random.default_rng(seed)
    matrix = (rng.standard_normal((40 + bucket, dim)) * np.exp2(rng.uniform(-12, 12, (40 + bucket, dim)))).astype(f32)
    matrix.setflags(write=False)
    return FT.make_model(words, matrix, minn, maxn, bucket)


@functools.lru_cache(maxsize=None)
def toy_index(bucket=64, minn=3, maxn=6, dim=300, seed=0):
    from sam_textvqa_amd import fasttext as FT
    return FT.model_index(toy_model(bucket, minn, maxn, dim, seed), max_word=32, n_slots=64)


# ---------------------------------------------------------------------------------------------------------------- hash and n-grams
def test_fnv1a_published_vectors_and_sign_extension():
    from sam_textvqa_amd import fasttext as FT
    assert FT.fnv1a(b"a") == 0xE40C292C and FT.fnv1a(b"foobar") == 0xBF9CF968 and FT.fnv1a(b"") == 2166136261
    h = 2166136261                                               # "é" = C3 A9, each byte sign-extended to 32 bits before the xor
    for byte in (0xFFFFFFC3, 0xFFFFFFA9):
        h = ((h ^ byte) * 16777619) & 0xFFFFFFFF
    assert FT.fnv1a("é".encode()) == h
    u = 2166136261                                               # the unsigned variant is another function: the upper 24 bits differ
    for byte in (0xC3, 0xA9):
        u = ((u ^ byte) * 16777619) & 0xFFFFFFFF
    assert u != h
    assert FT.utf8([0xE9, 0x20AC, 0x1F600, 0x41]) == "é€😀A".encode() and FT.utf8([0xE9 | 1 << 30, 0x41 | 1 << 31]) == "éA".encode()


def test_subwords_of_the_in_canonical_order():
    from sam_textvqa_amd import fasttext as FT
    want = [b"<th", b"<the", b"<the>", b"the", b"the>", b"he>"]
    assert FT.ngrams(b"<the>", 3, 6) == want
    assert FT.subwords(b"<the>", 3, 6, 64, 40) == [40 + FT.fnv1a(g) % 64 for g in want]
    # n = 1: the single characters at either end are skipped, the inner ones kept; start-major, length-minor
    assert FT.ngrams(b"<ab>", 1, 2) == [b"<a", b"a", b"ab", b"b", b"b>"]
    assert FT.ngrams(b"<>", 3, 6) == [] and FT.ngrams(b"<>", 1, 2) == [b"<>"] and FT.ngrams(b"<a>", 3, 6) == [b"<a>"] and FT.ngrams(b"<a>", 4, 6) == []


def test_ngram_boundaries_fall_between_characters():
    """"é€😀": 2-, 3- and 4-byte characters; with minn = 2, maxn = 3 the seven n-grams listed by hand; every one decodes: no boundary inside a character"""
    from sam_textvqa_amd import fasttext as FT
    got = FT.ngrams("<é€😀>".encode(), 2, 3)
    assert got == [g.encode() for g in ("<é", "<é€", "é€", "é€😀", "€😀", "€😀>", "😀>")]
    assert [len(g) for g in got] == [3, 6, 5, 9, 7, 8, 5]
    for g in FT.ngrams("<naïve日本>".encode(), 1, 8):
        g.decode("utf-8")


def test_reciprocal_in_double_rounds_to_the_fp32_reciprocal():
    for n in range(1, 601):
        assert f32(1.0 / n) == f32(1) / f32(n), n


# ---------------------------------------------------------------------------------------------------------------- the twins, case by case
def manual_vector(ids, matrix):
    v = np.zeros(matrix.shape[1], f32)
    for i in ids:
        v = v + matrix[i]
    return v * f32(1.0 / len(ids)) if ids else v


def test_word_vector_cases():
    from sam_textvqa_amd import fasttext as FT
    model, index = toy_model(), toy_index()
    m = model["matrix"]
    sub = lambda w: FT.subwords(b"<" + w.encode() + b">", 3, 6, 64, 40)
    cases = {"the": [0] + sub("the"), "The": [1] + sub("The"), "thex": sub("thex"), "</s>": [2], "": [], "a": [4] + sub("a"), "q": sub("q"), "café": [5] + sub("café"),
             "日本語": [6] + sub("日本語"), "😀": [7] + sub("😀"), LONG: sub(LONG)}
    for w, ids in cases.items():
        assert FT.word_ids(w, index) == ids, w
        assert np.array_equal(FT.word_vector_host(w, index), manual_vector(ids, m)), w
    assert len(cases["the"]) == 7 and len(cases["a"]) == 2 and len(cases["q"]) == 1         # "<a>" is itself a 3-gram; with minn = 4 a one-character word has none:
    four = toy_index(minn=4)
    assert FT.word_ids("a", four) == [4] and FT.word_ids("q", four) == [] and not FT.word_vector_host("q", four).any() and not FT.word_vector_host("", index).any()
    assert FT.word_ids("the", index) != FT.word_ids("The", index)                        # case-sensitive, unlike PHOC
    assert len(cases[LONG]) == 4 * (len(LONG) + 2) - 14 and 13 not in cases[LONG]        # listed in the dictionary, over the index width: n-grams only
    noeos = FT.model_index(FT.make_model(["the", "x"], m[:66], 3, 6, 64))                # no "</s>" in the dictionary: an ordinary unknown word
    assert noeos["eos"] == -1 and FT.word_ids("</s>", noeos) == FT.subwords(b"<</s>>", 3, 6, 64, 2)


def test_the_add_order_shows_in_the_bits():
    from sam_textvqa_amd import fasttext as FT
    model, index = toy_model(), toy_index()
    ids = FT.word_ids("within", index)
    a, b = manual_vector(ids, model["matrix"]), manual_vector(sorted(ids), model["matrix"])
    assert sorted(ids) != ids and not np.array_equal(a, b) and np.allclose(a, b, rtol=1e-3, atol=1e-2)


def test_mean_over_pieces_is_numpys():
    from sam_textvqa_amd import fasttext as FT
    index = toy_index()
    va, ve, vb = (FT.word_vector_host(w, index) for w in ("a", "", "b"))
    got = FT.token_vector_host("a  b", index)                    # two spaces: the empty middle piece counts
    assert got.dtype == f32 and np.array_equal(got, np.mean([va, ve, vb], axis=0)) and np.array_equal(got, ((va + ve) + vb) / f32(3))
    assert not np.array_equal(got, (va + vb) / f32(2)) and not ve.any()
    assert np.array_equal(FT.token_vector_host("stop the", index), (FT.word_vector_host("stop", index) + FT.word_vector_host("the", index)) / f32(2))
    assert np.array_equal(FT.token_vector_host("the", index), FT.word_vector_host("the", index))
    assert np.array_equal(FT.token_vector_host(" ", index), np.zeros(300, f32))
    assert np.array_equal(FT.vectors_host(["the", "a  b"], index), np.stack([FT.word_vector_host("the", index), got]))
    assert np.array_equal(FT.token_vector_host([ord(c) | 1 << 30 for c in "the"], index), FT.word_vector_host("the", index))      # the flag bits are no text


def test_vectors_host_text_clamps():
    from sam_textvqa_amd import fasttext as FT, phoc as P
    index = toy_index()
    packed = P.pack_ocr_text([["within", "the", "café", "stop"], ["a  b", "q", "x", "y"]], max_ocr_tokens=4, max_chars=6)
    packed["ocr_text"][0, 3, 4:] = torch.tensor([ord("x"), ord("y")])
    packed["ocr_text_len"][0] = torch.tensor([7, 3, -(1 << 31), 1 << 30])
    got = FT.vectors_host_text(packed["ocr_text"], packed["ocr_text_len"], index, torch.tensor([9, 1]))
    assert got.shape == (2, 4, 300) and got.dtype == f32
    assert np.array_equal(got[0], FT.vectors_host(["within", "the", "", "stopxy"], index))
    assert np.array_equal(got[1, 0], FT.token_vector_host("a  b", index)) and not got[1, 1:].any()
    assert not FT.vectors_host_text(packed["ocr_text"], packed["ocr_text_len"], index, torch.tensor([-3, 0])).any()


# ---------------------------------------------------------------------------------------------------------------- the model file
def test_bin_round_trip_is_bit_equal(tmp_path):
    from sam_textvqa_amd import fasttext as FT
    model = toy_model()
    path = str(tmp_path / "toy.bin")
    FT.write_bin(path, model, counts=range(1, 41))
    back = FT.load_bin(path)
    assert isinstance(back["matrix"], np.memmap) and not back["matrix"].flags.writeable                 # mapped, not copied
    assert back["words"] == model["words"] and back["matrix"].tobytes() == model["matrix"].tobytes()
    assert {k: back[k] for k in ("nwords", "bucket", "minn", "maxn", "dim", "args")} == {k: model[k] for k in ("nwords", "bucket", "minn", "maxn", "dim", "args")}
    a, b = FT.model_index(back, n_slots=64), toy_index()
    assert all(torch.equal(a[k], b[k]) for k in FT.INDEX_TENSORS) and {k: v for k, v in a.items() if k not in FT.INDEX_TENSORS} == {k: v for k, v in b.items() if k not in FT.INDEX_TENSORS}
    assert np.array_equal(FT.token_vector_host("the café", a), FT.token_vector_host("the café", b))


@pytest.mark.parametrize("raw,word", [(dict(magic=793712313), "magic"), (dict(version=11), "version"), (dict(version=13), "version"), (dict(quant_input=1), "quantised"),
                                      (dict(pruneidx=[(1, 2)]), "pruned"), (dict(nlabels=1), "labels"), (dict(bucket=0, m=40), "bucket"),
                                      (dict(m=103), "rows"), (dict(m=105), "rows"), (dict(n=299), "columns")],
                         ids=["magic", "version 11", "version 13", "quant_input", "pruneidx", "nlabels", "bucket 0 with maxn 6", "m short", "m long", "n"])
def test_load_bin_refusals(tmp_path, raw, word):
    from sam_textvqa_amd import fasttext as FT
    path = str(tmp_path / "bad.bin")
    FT.write_bin(path, toy_model(), raw=raw)
    with pytest.raises(ValueError, match=word):
        FT.load_bin(path)


def test_make_model_refusals():
    from sam_textvqa_amd import fasttext as FT
    m = np.zeros((66, 8), f32)
    for words, kw in ((["a", "a"], {}), (["a", ""], {}), (["a", "b"], dict(bucket=63)), (["a", "b"], dict(minn=4, maxn=3)), (["a", "b"], dict(matrix=m.astype(np.float64)))):
        with pytest.raises(ValueError, match="make_model"):
            FT.make_model(words, kw.pop("matrix", m), kw.pop("minn", 3), kw.pop("maxn", 6), kw.pop("bucket", 64))
    assert FT.make_model(["a", "b"], m[:2], 0, 0, 0)["bucket"] == 0                      # no n-grams: no buckets needed
    with pytest.raises(ValueError, match="model_index"):
        FT.model_index(FT.make_model(["a", "b"], np.zeros((66, 6), f32), 3, 6, 64))      # dim % 4
    with pytest.raises(ValueError, match="model_index"):
        FT.model_index(FT.make_model(["a", "b"], m, 3, 9, 64))                           # maxn over 8


# ---------------------------------------------------------------------------------------------------------------- the index
def test_decode_words_is_pythons_utf8_decoder():
    from sam_textvqa_amd import fasttext as FT
    words = [w.encode() if isinstance(w, str) else w for w in WORDS] + [b"\x80", b"a\x80", b"\xe0\x80\x80", b"\xf4\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xf5\x80\x80\x80",
                                                                        b"\xe2\x82", b"\xe2\x82\xac\xac", b"\xf4\x8f\xbf\xbf", b"\xef\xbf\xbf", b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80"]
    cps, nchar, valid = FT.decode_words(words)
    at = 0
    for w, n, ok in zip(words, nchar, valid):
        try:
            want = [ord(c) for c in w.decode("utf-8")]
        except UnicodeDecodeError:
            want = None
        assert bool(ok) == (want is not None), w
        if want is not None:
            assert cps[at: at + n].tolist() == want, w
        at += n
    assert at == cps.size and valid.sum() == 14 + 5


def test_model_index_finds_every_valid_word_and_nothing_else():
    from sam_textvqa_amd import fasttext as FT
    from sam_textvqa_amd.answers import text_hash
    model, index = toy_model(), toy_index()
    slots, ln = index["slots"].numpy(), index["len"].numpy()
    assert slots.size == 64 and index["matrix"].shape == (104, 300) and index["cp"].shape == (40, 32) and index["eos"] == 2
    entries = [i for i, w in enumerate(model["words"]) if i not in (13, 14, 15, 16, 17)]
    assert sorted(slots[slots >= 0].tolist()) == entries and (ln[[13, 14, 15, 16, 17]] == -1).all()
    away = 0
    for i in entries:
        cps = [ord(c) for c in model["words"][i].decode()]
        assert FT.index_lookup_host(index, cps) == i and ln[i] == len(cps)
        away += int(slots[text_hash(cps) & 63]) != i
    assert away > 0                                                                       # 35 entries in 64 slots: some were placed by probing
    for w in ("th", "thee", "", "W0", "w35", "caf", "cafe", "日本", LONG, "\udcff\udcfe"):
        assert FT.index_lookup_host(index, [ord(c) for c in w]) == -1, w
    big = FT.model_index(model)
    assert big["slots"].numel() == 128 and all(FT.index_lookup_host(big, [ord(c) for c in model["words"][i].decode()]) == i for i in entries)
    with pytest.raises(ValueError, match="n_slots"):
        FT.model_index(model, n_slots=32)
    assert FT.is_model_index(index) and not FT.is_model_index(model) and FT.index_to(index, "cpu")["nwords"] == 40


# ---------------------------------------------------------------------------------------------------------------- batches
def test_check_rules():
    from sam_textvqa_amd import fasttext as FT, phoc as P
    text = P.pack_ocr_text([["ab", "c"]], max_ocr_tokens=2)
    assert FT.check({}) is False and FT.check(dict(ocr_fasttext=torch.zeros(1, 2, 300))) is False and FT.check(dict(text)) is True and FT.check(dict(text), 2) is True
    assert FT.wants_fasttext(text) and not FT.wants_fasttext(dict(text, ocr_ft_rows=0)) and not FT.wants_fasttext({})
    with pytest.raises(ValueError, match="ocr_text_len"):
        FT.check({"ocr_text": text["ocr_text"]})
    for k in FT.FASTTEXT_KEYS:
        with pytest.raises(ValueError, match=k):
            FT.check(dict(text, **{k: torch.zeros(1, 2, 300)}))
    with pytest.raises(ValueError, match="int32"):
        FT.check(dict(text, ocr_text=text["ocr_text"].long()))
    with pytest.raises(ValueError, match="int32"):
        FT.check(dict(text, ocr_text_len=text["ocr_text_len"][:, :1]))
    with pytest.raises(ValueError, match="slots"):
        FT.check(dict(text), 3)


# ---------------------------------------------------------------------------------------------------------------- the C entry point
# a valid argument set (pointers are never dereferenced on the host), then one change per rejection
OK = dict(text=1 << 12, ld_text=32, text_len=1 << 13, counts=1 << 14, B=2, n_max=5, Lw=32, matrix=1 << 20, ld_matrix=300, cp=1 << 15, ld_cp=32, ln=1 << 17, slots=1 << 18,
          Lv=32, n_slots=128, minn=3, maxn=6, bucket=64, nwords=40, eos=2, dim=300, dst=1 << 16, ld_dst=1000, col0=0, f32=0, norm=1, eps=1e-12)
REJECTED = [
    ("null text", dict(text=None), "ARG", "null"), ("null text_len", dict(text_len=None), "ARG", "null"), ("null dst", dict(dst=None), "ARG", "null"),
    ("null matrix", dict(matrix=None), "ARG", "null"), ("null cp", dict(cp=None), "ARG", "null"), ("null len", dict(ln=None), "ARG", "null"),
    ("null slots", dict(slots=None), "ARG", "null"),
    ("Lw = 0", dict(Lw=0), "ARG", "Lw"), ("Lw = 65", dict(Lw=65, ld_text=65), "UNSUPPORTED", "Lw=65"),
    ("dim = 302", dict(dim=302, ld_matrix=304), "UNSUPPORTED", "dim=302"), ("dim = 516", dict(dim=516, ld_matrix=516), "UNSUPPORTED", "dim=516"),
    ("dim = 0", dict(dim=0), "ARG", "dim"), ("maxn = 9", dict(maxn=9), "UNSUPPORTED", "maxn=9"), ("minn > maxn", dict(minn=7), "ARG", "minn"),
    ("minn < 0", dict(minn=-1), "ARG", "minn"), ("col0 = 2", dict(col0=2), "UNSUPPORTED", "col0=2"), ("ld_dst = 1002", dict(ld_dst=1002), "UNSUPPORTED", "ld_dst=1002"),
    ("misaligned bf16 dst", dict(dst=(1 << 16) + 2), "UNSUPPORTED", "alignment"), ("misaligned fp32 dst", dict(dst=(1 << 16) + 8, f32=1), "UNSUPPORTED", "alignment"),
    ("ld_text < Lw", dict(ld_text=31), "ARG", "ld_text"), ("col0 + dim > ld_dst", dict(col0=704), "ARG", "col0"), ("col0 < 0", dict(col0=-4), "ARG", "col0"),
    ("B = 0", dict(B=0), "ARG", "shape"), ("n_max = 0", dict(n_max=0), "ARG", "shape"), ("eps = 0", dict(eps=0.0), "ARG", "eps"),
    ("bucket = 0 with maxn = 6", dict(bucket=0), "ARG", "bucket"), ("nwords = 0", dict(nwords=0), "ARG", "nwords"), ("eos = nwords", dict(eos=40), "ARG", "eos_id"),
    ("ld_matrix < dim", dict(ld_matrix=296), "ARG", "ld_matrix"), ("matrix rows off 16 bytes", dict(ld_matrix=302), "ARG", "ld_matrix"),
    ("misaligned matrix", dict(matrix=(1 << 20) + 4), "ARG", "16-byte"), ("Lv = 65", dict(Lv=65, ld_cp=65), "ARG", "Lv"), ("ld_index < Lv", dict(ld_cp=31), "ARG", "ld_index"),
    ("n_slots = 100", dict(n_slots=100), "ARG", "power of two"), ("misaligned text", dict(text=(1 << 12) + 2), "ARG", "misaligned"),
    ("misaligned counts", dict(counts=(1 << 14) + 2), "ARG", "misaligned"), ("misaligned slots", dict(slots=(1 << 18) + 1), "ARG", "misaligned"),
]


def _args(a):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return (p(a["text"]), a["ld_text"], p(a["text_len"]), p(a["counts"]), a["B"], a["n_max"], a["Lw"], p(a["matrix"]), a["ld_matrix"], p(a["cp"]), a["ld_cp"], p(a["ln"]),
            p(a["slots"]), a["Lv"], a["n_slots"], a["minn"], a["maxn"], a["bucket"], a["nwords"], a["eos"], a["dim"], p(a["dst"]), a["ld_dst"], a["col0"], a["f32"],
            a["norm"], a["eps"], None)


@pytest.mark.parametrize("name,change,code,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_argument_rejections_come_before_any_device_call(name, change, code, word):
    from sam_textvqa_amd import _capi
    rc = _capi.lib().sam_fasttext_from_text(*_args(dict(OK, **change)))
    assert rc == _capi.CONSTANTS["SAM_ERR_" + code] == {"ARG": -1, "UNSUPPORTED": -2}[code], name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_fasttext_from_text:") and word in msg, msg
    with pytest.raises(_capi.SamHipError, match="sam_fasttext_from_text"):
        _capi.call("sam_fasttext_from_text", *_args(dict(OK, **change)))


def test_the_entry_point_is_bound_from_its_header_and_the_model_abi_is_untouched():
    from ctypes import c_float, c_int, c_int64, c_void_p as vp
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    i, l64 = c_int, c_int64
    sig = [vp, l64, vp, vp, i, i, i, vp, l64, vp, l64, vp, vp, i, i, i, i, i, i, i, i, vp, l64, i, i, i, c_float, vp]
    assert _capi.HEADER_SIGNATURES["fasttext"] == {"sam_fasttext_from_text": sig} and _capi.HEADER_RESTYPES["fasttext"] == {"sam_fasttext_from_text": c_int}
    assert "sam_fasttext_from_text" not in _capi.SIGNATURES and "sam_fasttext_from_text" not in _capi.NO_STATUS
    for name, other in _capi.HEADER_SIGNATURES.items():                  # every other header of the registry
        assert name == "fasttext" or "sam_fasttext_from_text" not in other
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_fasttext_from_text.argtypes == sig and l.sam_fasttext_from_text.restype is c_int
    assert os.path.join(b.CSRC, "fasttext.hip") in b.sources()


def test_digest_covers_the_fasttext_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_fasttext.h"
    other.write_text(open(b.HEADERS["fasttext"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "fasttext", str(other))
    assert b._digest() != was


def test_the_unit_is_built_without_fast_math_and_with_contraction_off():
    import sam_textvqa_amd._build as b
    src = open(os.path.join(b.CSRC, "fasttext.hip")).read()
    assert not any("fast-math" in f or "ffp-contract" in f or f == "-Ofast" for f in b.FLAGS)
    assert "#pragma clang fp contract(off)" in src


def test_ops_wrapper_rejects_cpu_tensors():
    from sam_textvqa_amd import ops, phoc as P
    from sam_textvqa_amd._capi import SamHipError
    t = P.pack_ocr_text([["ab"]], max_ocr_tokens=2)
    with pytest.raises(SamHipError):
        ops.fasttext_from_text(t["ocr_text"], t["ocr_text_len"], None, toy_index(), torch.zeros(2, 300))        # CPU tensors: rejected, no fallback
