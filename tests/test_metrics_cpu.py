"""CPU: the host half of the metrics (sam_textvqa_amd/metrics.py) against tests/golden/metrics.json, which the reference's own
EvalAIAnswerProcessor, TextVQAAccuracy, STVQAAccuracy and STVQAANLS wrote (tests/golden/make_golden_metrics.py).  Bounds: the VQA and ST-VQA scores are
stored values (exact against the fp32-rounded golden); ANLS is one fp32 division and one subtraction on values in [0.5, 1]: 2^-22 absolute; a batch mean
of B values within B * 2^-24."""
import json
import os
import re

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAPS = M.ScoreTableCaps(10, 40, 64)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "metrics.json")) as f:
        g = json.load(f)
    voc = A.AnswerVocab(g["vocab"])
    tabs = [M.build_score_table(c["answers"], c["ocr_tokens"], max_ocr_tokens=g["max_ocr_tokens"]) for c in g["cases"]]
    g["voc"], g["vt"] = voc, M.vocab_text(voc, max_word=CAPS.Lw)
    g["table"] = M.collate_score_tables(tabs, CAPS)
    g["ids"] = np.array([c["pred_ids"] for c in g["cases"]], np.int64)
    return g


def check_scores(got, cases):
    got = np.asarray(got)
    for s, c in zip(got, cases):
        e = np.array(c["scores"], np.float32)
        print(c["name"], s, e)
        assert s[0] == e[0] and s[1] == e[1], c["name"]
        assert abs(float(s[2]) - float(e[2])) <= 2.0 ** -22, c["name"]


def test_normalize_answer_equals_every_golden_pair(golden):
    assert len(golden["pairs"]) >= 60
    for src, want in golden["pairs"]:
        assert M.normalize_answer(src) == want, repr(src)


def test_issue_example_and_empty_result():
    # the period rule alone turns "a.b 1.5 x. <=." into "ab 1.5 x <="; the whole processor then also deletes "<" (it touches a blank) and blanks "="
    assert M.normalize_answer("a.b 1.5 x. <=.") == "ab 1.5 x"
    assert M.normalize_answer("The a an") == ""


def test_whitespace_list_is_pythons():
    assert all(chr(c).isspace() == (c in M.WHITESPACE) for c in range(0x110000))


def test_host_twin_equals_golden_scores_and_means(golden):
    got = M.score_answers_host(golden["ids"], golden["table"], golden["vt"])
    assert got.dtype == np.float32 and got.shape == (len(golden["cases"]), 3)
    check_scores(got, golden["cases"])
    B = len(golden["cases"])
    means = got.astype(np.float64).mean(0)
    for m, e in zip(means, golden["batch_means"]):
        assert abs(m - e) <= B * 2.0 ** -24


def test_golden_covers_the_soft_score_levels_and_the_anls_tie(golden):
    by = {c["name"]: c["scores"] for c in golden["cases"]}
    assert [round(by[n][0], 6) for n in ("soft_0.3", "soft_0.6", "soft_0.9_after_normalisation", "soft_1.0")] == [0.3, 0.6, 0.9, 1.0]
    assert (by["anls_tie"][2], by["anls_one_edit_above"][2], by["anls_one_edit_below"][2]) == (0.5, 0.75, 0.0)


def test_assembled_string_agrees_with_decode_predictions(golden):
    tab = golden["table"]
    padded = [list(c["ocr_tokens"]) + [A.PAD_TOKEN] * (golden["max_ocr_tokens"] - len(c["ocr_tokens"])) for c in golden["cases"]]
    dec = A.decode_predictions(golden["ids"].tolist(), golden["voc"], padded)
    for b, c in enumerate(golden["cases"]):
        s, bad = M.assemble_prediction(golden["ids"][b], tab["ocr"][b].numpy(), tab["ocr_len"][b].numpy(), golden["vt"]["cp"].numpy(),
                                       golden["vt"]["len"].numpy(), golden["vt"]["eos"])
        assert not bad
        assert dec[b][0] == c["answer"]
        assert s == dec[b][0].lower(), c["name"]


def test_score_table_contents():
    t = M.build_score_table(["Three"] * 3 + ["3"] * 2 + [" the cat "] * 4 + ["dog"], ["a", "b"], max_ocr_tokens=4)
    assert t["gt_norm"] == ["3", "cat", "dog"]
    assert t["gt_raw"] == ["three", "3", "the cat", "dog"]
    want = A.soft_scores(["3"] * 5 + ["cat"] * 4 + ["dog"])
    assert t["gt_score"].tolist() == [np.float32(want[k]) for k in ("3", "cat", "dog")]
    assert ["".join(map(chr, o)) for o in t["ocr"]] == ["a", "b", "<pad>", "<pad>"]
    with pytest.raises(ValueError):
        M.build_score_table(["x"] * 9, [])


def test_capacity_overflow_raises_and_names_the_capacity():
    t = M.build_score_table(["abcdefghij"] * 10, ["longtoken"], max_ocr_tokens=2)
    with pytest.raises(ValueError, match=r"sample 0.*Lg = 9"):
        M.collate_score_tables([t], M.ScoreTableCaps(10, 16, 9))
    with pytest.raises(ValueError, match=r"sample 0.*Lw = 8"):
        M.collate_score_tables([t], M.ScoreTableCaps(10, 8, 16))
    t2 = M.build_score_table(list("abcdefghij"), [], max_ocr_tokens=2)
    with pytest.raises(ValueError, match=r"sample 1.*A = 4"):
        M.collate_score_tables([t, t2], M.ScoreTableCaps(4, 16, 16))
    with pytest.raises(ValueError, match=r"Lw = 4"):
        M.vocab_text(A.AnswerVocab(["<pad>", "<s>", "</s>", "<unk>", "seven"]), max_word=4)
    ok = M.collate_score_tables([t, t2], M.ScoreTableCaps(10, 16, 16))
    assert ok["gt_norm"].shape == (2, 10, 16) and ok["ocr"].shape == (2, 2, 16) and ok["meta"][:, :2].tolist() == [[1, 1], [10, 10]]


def test_host_twin_errors_and_flags(golden):
    t = M.collate_score_tables([M.build_score_table(["the"] * 10, ["x"], max_ocr_tokens=2)], M.ScoreTableCaps(10, 40, 8))
    eos, V = golden["vt"]["eos"], len(golden["vocab"])
    with pytest.raises(IndexError):
        M.score_answers_host([[V + 2, eos]], t, golden["vt"])
    sc, fl = M.score_answers_host([[V + 0, V + 2, eos], [-1, eos, eos]], {k: torch.cat([v, v]) for k, v in t.items()}, golden["vt"], return_flags=True)
    assert fl.tolist() == [1, 1]
    t0 = M.collate_score_tables([M.build_score_table([""] * 10, [], max_ocr_tokens=2)], M.ScoreTableCaps(10, 40, 8))
    with pytest.raises(ValueError, match="both empty"):
        M.score_answers_host([[eos, 0]], t0, golden["vt"])
    sc, fl = M.score_answers_host([[eos, 0]], t0, golden["vt"], return_flags=True)
    assert fl.tolist() == [2] and sc.tolist() == [[1.0, 1.0, 0.0]]          # "" is the one normalised answer, ten of ten: soft score 1


def test_make_score_tables_matches_make_answer_tables():
    voc, a_tabs, s_tabs = M.make_score_tables(5, num_vocab=300, n_ocr=20, seed=7)
    voc0, a0 = A.make_answer_tables(5, num_vocab=300, n_ocr=20, seed=7)
    assert voc.word_list == voc0.word_list
    for x, y in zip(a_tabs, a0):
        assert all(np.array_equal(x[k], y[k]) for k in y)
    assert len(s_tabs) == 5 and all(len(t["ocr"]) == 20 for t in s_tabs)
    _, _, rich = M.make_score_tables(8, num_vocab=300, n_ocr=20, seed=7, rich=True)
    M.collate_score_tables(rich)


def test_kernel_word_map_and_lists_match_the_python_ones():
    src = open(os.path.join(ROOT, "sam-textvqa_amd", "csrc", "score.hip")).read()
    body = src[src.index("kWordMap[] = {"):src.index("constexpr int kMapSize")]
    pairs = re.findall(r'\{"((?:[^"\\]|\\.)*)", "((?:[^"\\]|\\.)*)"\}', body)
    assert [tuple(p) for p in pairs] == [tuple(p) for p in M.WORD_MAP]
    assert len(M.CONTRACTIONS) == 120 and M.MAX_PERIODS == 32
    cases = re.findall(r"case '(\\?.)': return (\d+);", src)
    assert [c.replace("\\\\", "\\") for c, _ in cases] == list(M.PUNCTUATION) and [int(i) for _, i in cases] == list(range(21))


def test_library_exports_score_answers_and_keeps_the_abi_version():
    from sam_textvqa_amd import _capi as capi
    assert "sam_score_answers" in capi.SIGNATURES
    l = capi.lib()
    assert hasattr(l, "sam_score_answers") and l.sam_abi_version() == 9
    rc = l.sam_score_answers(*([None] * 11), 1, 12, 10, 64, 50, 32, 100, 2, None, None, None, None)
    assert rc != 0 and b"null pointer" in l.sam_last_error()


def test_trainer_metric_argument_checks():
    from sam_textvqa_amd.trainer import Trainer
    for kw in (dict(metric="vqa"), dict(metric="textvqa"), dict(metric="textvqa", answer_targets="table"),
               dict(metric="stvqa_anls", answer_targets="table", predictions=True)):
        with pytest.raises(ValueError):
            Trainer(None, **kw)
