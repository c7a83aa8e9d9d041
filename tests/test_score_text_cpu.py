"""CPU (no GPU needed): the metrics' score tables from text (sam_textvqa_amd/metrics.py score_tables_from_text_host, include/sam_hip_metrics.h; DESIGN.md
§3.18).  The host twin of sam_score_table_from_text against collate_score_tables(build_score_table(...)), bit for bit and padding included, on the rich
synthetic samples, the reference-written golden cases and the corner shapes the GPU test launches; the NO_GLUE bit, the one deviation (ASCII-only
lowering), the status bit, the misuse checks and the ctypes table of the eighth header."""
import json
import os

import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import phoc as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_CAPS = M.ScoreTableCaps(10, 40, 64)           # the capacities tests/test_metrics_cpu.py collates the golden cases at


def pack(answers, tokens, caps=M.DEFAULT_SCORE_CAPS, n_ocr=50, max_answer=128, counts=None):
    """the text-schema half of a batch: answers [B][A] and tokens [B][<= n_ocr] packed as the dataset ships them, with the tokens per sample"""
    bd = dict(A.pack_answer_text(answers, num_answers=caps.A, max_chars=max_answer))
    if n_ocr > 0:
        bd.update(P.pack_ocr_text(tokens, max_ocr_tokens=n_ocr, max_chars=caps.Lw))
    else:
        bd.update(ocr_text=torch.zeros((len(answers), 0, caps.Lw), dtype=torch.int32), ocr_text_len=torch.zeros((len(answers), 0), dtype=torch.int32))
    bd["ocr_count"] = M.ocr_counts(tokens, n_ocr) if counts is None else torch.tensor(counts, dtype=torch.int32)
    return bd


def host_built(answers, tokens, caps, n_ocr):
    """what the host path ships: collate_score_tables of build_score_table per sample"""
    return M.collate_score_tables([M.build_score_table(a, t, num_answers=caps.A, max_ocr_tokens=n_ocr) for a, t in zip(answers, tokens)], caps)


def assert_same_table(got, want, what=""):
    for k in M.SCORE_TABLE_KEYS:
        g, w = got[k].cpu(), want[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        gi, wi = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (g, w))
        bad = (gi != wi).nonzero()
        assert bad.numel() == 0, (what, k, bad[:4].tolist(), g[tuple(bad[0])].item(), w[tuple(bad[0])].item())


def keep_lowerable(answers, tokens):
    """the samples without what the device cannot lower: a token that fails device_lowerable leaves its list, a sample with such an answer leaves the batch.
    -> (answers, tokens, strings dropped, strings seen)"""
    out_a, out_t, dropped, seen = [], [], 0, 0
    for ans, toks in zip(answers, tokens):
        seen += len(ans) + len(toks)
        good = [t for t in toks if M.device_lowerable(t)]
        dropped += len(toks) - len(good)
        if all(M.device_lowerable(a) for a in ans):
            out_a.append(ans)
            out_t.append(good)
        else:
            dropped += len(ans) + len(good)
    return out_a, out_t, dropped, seen


def golden_text():
    with open(os.path.join(HERE, "golden", "metrics.json")) as f:
        g = json.load(f)
    return g, [c["answers"] for c in g["cases"]], [c["ocr_tokens"] for c in g["cases"]]


# ---- the corner shapes: shared with tests/test_score_text_gpu.py, which launches the kernel on the same batches
# 31 periods in the first 64 code points, "-" at 63 touching the blank at 64 (the punctuation rule across the lane boundary), the 32nd period (the last
# one deleted) and twelve more (kept) in the second trip of the period filter, a period before a digit, "'s" near the end
LONG = "a." * 31 + "x- " + ".b" * 12 + " 1.5 it's (stop) dont THE x.5 joe's a/b"
ANSWERS = ["the cat", "cat", "a cat", "the", "", "   ", "The Cat", " cat\t", LONG, "JOE'S", "it's", "x's x's", "ten", "1.5", "hed've", "e\tf", " nb", "- go", "..", "'stop",
           "(stop)", "coca-cola", "St.", "NONE", "a/b", "cat ", "CAT", "the the", "an a", "\n", "q?", "1,000"]
TOKENS = ["'S", "JOE'S", "joe's", "", "Stop", "<pad>", "w1", "'s", "X'SS", "S'", "''S", "it's", "A", " ", "coca-cola", "1.5", "Z" * 64]
# (B, A, La, No, Lw, Lg, counts): Lg >= 1.5 La everywhere, so that nothing is flagged; counts include 0, No, and values the kernel clamps
SHAPES = [(1, 1, 1, 0, 8, 8, [3]), (2, 3, 63, 1, 8, 100, [0, 1]), (3, 10, 64, 50, 32, 128, [50, 0, 17]), (2, 10, 65, 64, 64, 255, [64, 70]),
          (2, 64, 16, 4, 8, 40, [-2, 3]), (3, 10, 128, 50, 32, 255, [49, -1, 99])]
assert len(LONG) == 128 and LONG[63] == "-" and LONG[64] == " " and LONG[:64].count(".") == 31 and LONG.count(".") > 32


def corner_batch(B, A_, La, No, Lw, Lg, counts):
    """sample 0: the corner answers in turn; sample 1: all answers equal; sample 2: all distinct.  Every string cut to its capacity."""
    caps = M.ScoreTableCaps(A_, Lw, Lg)
    answers, tokens = [], []
    for b in range(B):
        if b % 3 == 0:
            ans = [ANSWERS[(8 + i) % len(ANSWERS)][:La] if i % 2 else ANSWERS[i // 2 % len(ANSWERS)][:La] for i in range(A_)]
        elif b % 3 == 1:
            ans = [LONG[:La]] * A_
        else:
            ans = [("%s d%d" % (LONG[:max(La - 4, 0)], i))[-La:] for i in range(A_)]
        answers.append(ans)
        tokens.append([TOKENS[(b + i) % len(TOKENS)][:Lw] for i in range(No)])
    return caps, answers, tokens, pack(answers, tokens, caps, n_ocr=No, max_answer=La, counts=counts)


def corner_host_built(caps, answers, tokens, No, counts):
    """the host-built table of a corner batch: a sample's tokens are its first clamp(count) slots"""
    cut = [t[:max(0, min(int(c), No))] for t, c in zip(tokens, counts)]
    return host_built(answers, cut, caps, No)


# ------------------------------------------------------------------------------------------------------------------------------------ the twin
def test_twin_equals_the_host_built_table_on_the_rich_synthetic_samples():
    voc, answers, tokens = M.make_score_text(8, rich=True)
    answers, tokens, dropped, seen = keep_lowerable(answers, tokens)
    print("rich: %d of %d strings dropped" % (dropped, seen))
    assert 4 * dropped <= seen and dropped == 0          # _RICH's two non-ASCII entries are lower case already
    assert any(not t.isascii() for ts in tokens for t in ts)
    want = M.collate_score_tables(M.make_score_tables(8, rich=True)[2])
    assert_same_table(host_built(answers, tokens, M.DEFAULT_SCORE_CAPS, 50), want, "make_score_text gives make_score_tables' samples")
    got, status = M.score_tables_from_text_host(pack(answers, tokens))
    assert not status.any()
    assert_same_table(got, want, "rich")


def test_twin_equals_the_host_built_table_on_the_golden_cases():
    g, answers, tokens = golden_text()
    answers, tokens, dropped, seen = keep_lowerable(answers, tokens)
    print("golden: %d of %d strings dropped" % (dropped, seen))
    assert 4 * dropped <= seen and dropped == 0 and len(answers) == len(g["cases"])
    assert any(a != a.lower() for an in answers for a in an) or any(t != t.lower() for ts in tokens for t in ts)      # the lowering has work to do
    got, status = M.score_tables_from_text_host(pack(answers, tokens, GOLDEN_CAPS, n_ocr=g["max_ocr_tokens"]), GOLDEN_CAPS)
    assert not status.any()
    assert_same_table(got, host_built(answers, tokens, GOLDEN_CAPS, g["max_ocr_tokens"]), "golden")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-A%d-La%d-No%d-Lw%d-Lg%d" % s[:6])
def test_twin_equals_the_host_built_table_on_the_corner_shapes(shape):
    B, A_, La, No, Lw, Lg, counts = shape
    caps, answers, tokens, bd = corner_batch(*shape)
    assert all(M.device_lowerable(s) for row in answers + tokens for s in row)
    got, status = M.score_tables_from_text_host(bd, caps)
    assert not status.any()
    assert_same_table(got, corner_host_built(caps, answers, tokens, No, counts), str(shape))


def test_corner_answers_hold_what_they_are_meant_to():
    assert M.normalize_answer("the cat") == M.normalize_answer("cat") == M.normalize_answer("a cat") == "cat"
    assert M.normalize_answer("the") == "" and M.normalize_answer("   ") == ""
    t = M.score_tables_from_text_host(pack([["the cat", "cat", "a cat", "the", "", "   ", "cat", "cat", "cat", "cat"]], [[]]))[0]
    assert t["meta"][0, :2].tolist() == [2, 5]           # normalised: "cat", ""; raw: "the cat", "cat", "a cat", "the", ""
    assert t["gt_norm_len"][0, :3].tolist() == [3, 0, 0] and t["gt_raw_len"][0, :6].tolist() == [7, 3, 5, 3, 0, 0]


def test_counts_default_to_ocr_count_then_to_the_mask_rows():
    answers, tokens = [["a b"] * 10] * 2, [["x", "", "Y"], ["z"]]
    bd = pack(answers, tokens, n_ocr=4)
    want = host_built(answers, tokens, M.DEFAULT_SCORE_CAPS, 4)
    assert_same_table(M.score_tables_from_text_host(bd)[0], want)
    cnt = bd.pop("ocr_count")
    with pytest.raises(ValueError, match="ocr_count"):
        M.score_tables_from_text_host(bd)
    bd["pad_ocr_mask"] = torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0]])
    assert_same_table(M.score_tables_from_text_host(bd)[0], want)
    assert_same_table(M.score_tables_from_text_host(bd, counts=cnt)[0], want)
    assert M.score_tables_from_text_host(bd)[0]["ocr_len"].tolist() == [[1, 0, 1, 5], [1, 5, 5, 5]]          # an empty token is a token, not padding


# ------------------------------------------------------------------------------------------------------------------------------------ lowering
def test_an_s_lowered_right_after_an_apostrophe_carries_no_glue():
    t = M.score_tables_from_text_host(pack([["x"] * 10], [["'S", "JOE'S", "joe's"]], n_ocr=3))[0]
    ocr, ln = t["ocr"][0].numpy(), t["ocr_len"][0].tolist()
    assert ln == [2, 5, 5]
    assert ocr[0, :2].tolist() == [ord("'"), ord("s") | M.NO_GLUE]
    assert ocr[1, :5].tolist() == [ord(c) for c in "joe'"] + [ord("s") | M.NO_GLUE]
    assert ocr[2, :5].tolist() == [ord(c) for c in "joe's"] and not (ocr[2] & M.NO_GLUE).any()
    assert ocr[1, :5].tolist() == M._lower_word("JOE'S")


def test_device_lowerable_is_the_stated_predicate_and_the_deviation_is_real():
    for s, ok in (("Coca-Cola", True), ("über", True), ("σας", True), ("ÜBER", False), ("straße", True), ("İ", False), ("", True), ("ǅ", False)):
        assert M.device_lowerable(s) is ok, s
        assert ok == ("".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in s) == s.lower())
    answers, tokens = [["ÜBER alles"] * 10], [["ÉCOLE"]]
    got = M.score_tables_from_text_host(pack(answers, tokens, n_ocr=1))[0]
    want = host_built(answers, tokens, M.DEFAULT_SCORE_CAPS, 1)
    assert not torch.equal(got["gt_raw"], want["gt_raw"]) and not torch.equal(got["gt_norm"], want["gt_norm"]) and not torch.equal(got["ocr"], want["ocr"])
    assert got["gt_raw"][0, 0, :10].tolist() == [ord(c) for c in "Über alles"] and want["gt_raw"][0, 0, :10].tolist() == [ord(c) for c in "über alles"]


# ------------------------------------------------------------------------------------------------------------------------------------ status
LONG_S = "x's " * 32          # 128 code points; normalised "x 's x 's ..." holds 159


def status_batch():
    clean = ["red apple"] * 5 + ["Apple"] * 5
    answers, tokens = [clean, [LONG_S] + clean[1:], clean], [["Red", "apple"], ["x"], []]
    return answers, tokens, pack(answers, tokens)


def test_status_bit_1_where_collate_raises_between_clean_neighbours():
    assert len(LONG_S) == 128 and len(M.normalize_answer(LONG_S)) == 159
    answers, tokens, bd = status_batch()
    with pytest.raises(ValueError, match="Lg = 128"):
        host_built([answers[1]], [tokens[1]], M.DEFAULT_SCORE_CAPS, 50)
    got, status = M.score_tables_from_text_host(bd)
    assert status.tolist() == [0, M.STATUS_LG, 0]
    for k in M.SCORE_TABLE_KEYS:
        assert not got[k][1].any(), k
    want = host_built([answers[0], answers[2]], [tokens[0], tokens[2]], M.DEFAULT_SCORE_CAPS, 50)
    assert_same_table({k: got[k][[0, 2]] for k in M.SCORE_TABLE_KEYS}, want)
    assert "sample 1" in M.score_status_message(status.tolist(), M.DEFAULT_SCORE_CAPS) and M.score_status_message([0, 0], M.DEFAULT_SCORE_CAPS) is None


def test_a_raw_answer_over_lg_and_a_pad_over_lw_are_flagged_too():
    caps = M.ScoreTableCaps(2, 4, 6)
    got, status = M.score_tables_from_text_host(pack([["abcdefg", "the"], ["ab", "ab"], ["ab", "ab"]], [["x"], ["x"], []], caps, n_ocr=1), caps)
    assert status.tolist() == [M.STATUS_LG, 0, M.STATUS_PAD]
    with pytest.raises(ValueError, match="Lw = 4"):
        host_built([["ab", "ab"]], [[]], caps, 1)
    assert got["meta"][:, :2].tolist() == [[0, 0], [1, 1], [0, 0]]


# ------------------------------------------------------------------------------------------------------------------------------------ misuse, binding
def test_check_score_text_raises_for_each_misuse():
    bd = pack([["a"] * 10], [["x"]])
    assert M.check_score_text(bd) is True and M.check_score_text({"pad_ocr_mask": 0}) is False
    assert M.check_score_text({k: bd[k] for k in ("ocr_text", "ocr_text_len")}) is False          # OCR text alone serves PHOC and FastText
    for drop, word in (("answer_text_len", "answer_text without answer_text_len"), ("answer_text", "answer_text_len without answer_text"),
                       ("ocr_text_len", "ocr_text without ocr_text_len"), ("ocr_text", "ocr_text_len without ocr_text")):
        with pytest.raises(ValueError, match=word):
            M.check_score_text({k: v for k, v in bd.items() if k != drop})
    with pytest.raises(ValueError, match="without ocr_text / ocr_text_len"):
        M.check_score_text({k: bd[k] for k in ("answer_text", "answer_text_len")})
    with pytest.raises(ValueError, match="not both"):
        M.check_score_text(dict(bd, score_table={}))


def test_the_entry_point_is_bound_from_its_own_header():
    from ctypes import c_int, c_int64, c_void_p as vp
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    i, l64 = c_int, c_int64
    sig = [vp, l64, vp, vp, l64, vp, vp, i, i, i, i, i, i] + [vp] * 10
    assert _capi.HEADER_SIGNATURES["metrics"] == {"sam_score_table_from_text": sig} and _capi.HEADER_RESTYPES["metrics"] == {"sam_score_table_from_text": c_int}
    assert "sam_score_table_from_text" not in _capi.SIGNATURES and "sam_score_table_from_text" not in _capi.NO_STATUS
    for name, other in _capi.HEADER_SIGNATURES.items():                  # every other header of the registry
        assert name == "metrics" or "sam_score_table_from_text" not in other
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_score_table_from_text.argtypes == sig and l.sam_score_table_from_text.restype is c_int
    assert os.path.join(b.CSRC, "score_text.hip") in b.sources()


def test_digest_and_object_stamp_cover_the_header_and_the_included_tables(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_metrics.h"
    other.write_text(open(b.HEADERS["metrics"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "metrics", str(other))
    assert b._digest() != was
    assert b.SOURCE_INCLUDES["score_text.hip"] == ("score.hip",)          # score_text.hip reads the normaliser's tables out of score.hip
    src = open(os.path.join(b.CSRC, "score_text.hip")).read()
    assert '#include "score.hip"' in src and '#include "score_norm.h"' in src and "kWordMap[] = {" not in src


OK = dict(B=2, A=10, La=128, No=50, Lw=32, Lg=128, ld_answer=128, ld_ocr=32)


def _args(d, null=None):
    from ctypes import c_void_p
    ptrs = {n: c_void_p(0x1000) for n in ("answer_text", "answer_len", "ocr_text", "ocr_len", "ocr_count", "meta", "gt_norm", "gt_norm_len", "gt_score", "gt_raw",
                                           "gt_raw_len", "ocr", "ocr_out_len", "status")}
    if null:
        ptrs[null] = None
    p = ptrs
    return (p["answer_text"], d["ld_answer"], p["answer_len"], p["ocr_text"], d["ld_ocr"], p["ocr_len"], p["ocr_count"], d["B"], d["A"], d["La"], d["No"], d["Lw"],
            d["Lg"], p["meta"], p["gt_norm"], p["gt_norm_len"], p["gt_score"], p["gt_raw"], p["gt_raw_len"], p["ocr"], p["ocr_out_len"], p["status"], None)


@pytest.mark.parametrize("name,change,null,code,word", [
    ("no answers", dict(A=0), None, "ARG", "bad shape"), ("no batch", dict(B=0), None, "ARG", "bad shape"), ("negative slots", dict(No=-1), None, "ARG", "bad shape"),
    ("La 0", dict(La=0), None, "ARG", "La=0"), ("La 129", dict(La=129, ld_answer=129), None, "ARG", "La=129"), ("Lw 65", dict(Lw=65, ld_ocr=65), None, "ARG", "Lw=65"),
    ("Lw 0", dict(Lw=0), None, "ARG", "Lw=0"), ("Lg 0", dict(Lg=0), None, "ARG", "Lg=0"), ("Lg 256", dict(Lg=256), None, "ARG", "Lg=256"),
    ("ld_answer", dict(ld_answer=127), None, "ARG", "ld_answer"), ("ld_ocr", dict(ld_ocr=31), None, "ARG", "ld_ocr"),
    ("null text", {}, "answer_text", "ARG", "null answer"), ("null ocr", {}, "ocr_len", "ARG", "null OCR"), ("null out", {}, "gt_raw", "ARG", "null output"),
    ("A 65", dict(A=65), None, "UNSUPPORTED", "at most 64"), ("LDS", dict(A=64, Lg=255), None, "UNSUPPORTED", "64 KiB"),
])
def test_argument_rejections_come_before_any_device_call(name, change, null, code, word):
    from sam_textvqa_amd import _capi
    rc = _capi.lib().sam_score_table_from_text(*_args(dict(OK, **change), null))
    assert rc == _capi.CONSTANTS["SAM_ERR_" + code] == {"ARG": -1, "UNSUPPORTED": -2}[code], name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_score_table_from_text:") and word in msg, msg


def test_ops_wrapper_rejects_cpu_tensors():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    bd = pack([["a"] * 10], [["x"]])
    with pytest.raises(SamHipError):          # CPU tensors: rejected, no fallback
        ops.score_table_from_text(bd["answer_text"], bd["answer_text_len"], bd["ocr_text"], bd["ocr_text_len"], bd["ocr_count"],
                                  M.score_table_outputs(1, 50, M.DEFAULT_SCORE_CAPS, "cpu"))
