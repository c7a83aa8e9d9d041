"""CPU (no GPU needed): beam-search output to per-question results (sam_textvqa_amd/metrics.py evaluate_beams_host, include/sam_hip_eval.h; DESIGN.md
§3.19).  The host twin of sam_eval_beams against tests/golden/eval_beams.json, which the reference's own evaluate_predictions wrote
(tests/golden/make_golden_eval.py): chosen beam and answer string exact, stored VQA scores exact, ANLS within 2^-22, means within B * 2^-24 -- the bounds
tests/test_metrics_cpu.py uses for the same quantities.  Also: the twin's beam scores against score_answers_host on the repeated table, the arg-max rule
against numpy.argmax, the ctypes table of the ninth header, and the entry point's argument checks."""
import json
import os

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M

HERE = os.path.dirname(os.path.abspath(__file__))
CAPS = M.ScoreTableCaps(10, 40, 64)                  # the capacities tests/test_metrics_cpu.py collates its golden cases at


def load_golden():
    """the golden questions as the batch a model run would leave: complete_seqs [B * K, S], topkscores [B * K, 1], the score table of the B questions"""
    with open(os.path.join(HERE, "golden", "eval_beams.json")) as f:
        g = json.load(f)
    voc = A.AnswerVocab(g["vocab"])
    qs = g["questions"]
    g["vt"] = M.vocab_text(voc, max_word=CAPS.Lw)
    g["table"] = M.collate_score_tables([M.build_score_table(q["answers"], q["ocr_tokens"], max_ocr_tokens=g["max_ocr_tokens"]) for q in qs], CAPS)
    g["seqs"] = np.array([row for q in qs for row in q["complete_seqs"]], np.int64)
    g["cum"] = np.array([s for q in qs for s in q["topkscores"]], np.float32).reshape(-1, 1)
    return g


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def check_against_golden(res, g):
    """res: evaluate_beams' / evaluate_beams_host's dict as numpy arrays"""
    qs = g["questions"]
    B = len(qs)
    text = M.answer_strings(res["answer"], res["answer_len"])
    for b, q in enumerate(qs):
        s = res["best_scores"][b]
        print(q["name"], int(res["best"][b]), repr(text[b]), s, q["best"], repr(q["answer"]), q["vqa"], q["anls"])
        assert int(res["best"][b]) == q["best"] and text[b] == q["answer"], q["name"]
        assert s[0] == np.float32(q["vqa"]), q["name"]
        assert abs(float(s[2]) - q["anls"]) <= 2.0 ** -22, q["name"]
        assert res["best_ids"][b].tolist() == q["complete_seqs"][q["best"]][1:] and res["best_flags"][b] == 0
    means = res["best_scores"].astype(np.float64).mean(0)
    assert abs(means[0] - g["means"]["vqa"]) <= B * 2.0 ** -24 and abs(means[2] - g["means"]["anls"]) <= B * 2.0 ** -24, (means, g["means"])


def test_golden_holds_the_cases_the_kernel_has_to_get_right(golden):
    qs = {q["name"]: q for q in golden["questions"]}
    assert golden["K"] == 5 and golden["S"] == 12 and len(qs) >= 8
    assert sum(q["best"] != 0 for q in qs.values()) >= 2
    assert [q["question_id"] for q in golden["questions"]] != sorted(q["question_id"] for q in golden["questions"])
    tie = qs["exact_tie_first_wins"]
    assert tie["topkscores"][1] == tie["topkscores"][2] == max(tie["topkscores"]) and tie["best"] == 1
    assert len(set(qs["all_scores_equal"]["topkscores"])) == 1 and qs["all_scores_equal"]["best"] == 0
    assert qs["winner_ends_at_step_0"]["answer"] == "" and qs["glue_and_whitespace_to_strip"]["answer"] == "lead joe's  bar"


def test_host_twin_equals_the_golden(golden):
    res = M.evaluate_beams_host(golden["seqs"], golden["cum"], golden["table"], golden["vt"], golden["K"])
    check_against_golden(res, golden)
    assert (res["oracle"] >= res["best_scores"]).all() and (res["oracle"][:, 0] > res["best_scores"][:, 0]).any()       # ranking leaves accuracy on the table
    assert not res["beam_flags"].any()


def test_twin_scores_every_beam_as_score_answers_host_on_the_repeated_table(golden):
    K = golden["K"]
    res = M.evaluate_beams_host(golden["seqs"], golden["cum"].reshape(-1), {"score_table": golden["table"]}, golden["vt"], K)
    rep = {k: v.repeat_interleave(K, dim=0) for k, v in golden["table"].items()}
    want, wfl = M.score_answers_host(golden["seqs"][:, 1:], rep, golden["vt"], return_flags=True)
    assert np.array_equal(res["beam_scores"].view(np.int32), want.view(np.int32)) and np.array_equal(res["beam_flags"], wfl)
    B = len(golden["questions"])
    for b in range(B):
        r = b * K + res["best"][b]
        assert np.array_equal(res["best_scores"][b], want[r]) and np.array_equal(res["oracle"][b], want[b * K:(b + 1) * K].max(0))
        assert (res["answer"][b, res["answer_len"][b]:] == 0).all()
    tot = np.zeros(4)
    M.evaluate_beams_host(golden["seqs"], golden["cum"], golden["table"], golden["vt"], K, totals=tot)
    assert np.array_equal(tot, M.host_totals(res["best_scores"])) and tot[3] == B
    assert np.abs(tot[:3] - res["best_scores"].astype(np.float64).sum(0)).max() <= B * 2.0 ** -50
    for bad in (dict(beam=4), dict(beam=0), dict(skip=12), dict(skip=-1)):
        with pytest.raises(ValueError, match="evaluate_beams_host"):
            M.evaluate_beams_host(golden["seqs"], golden["cum"], golden["table"], golden["vt"], **dict(dict(beam=K), **bad))


def test_argmax_rule_is_numpys():
    rng = np.random.RandomState(0)
    pool = np.array([-np.inf, -2.5, -0.0, 0.0, 1.0, 1.0, 3.5, np.inf, np.nan], np.float32)
    n_nan = 0
    for trial in range(3000):
        K = 1 + trial % 64
        v = rng.randn(K).astype(np.float32) if trial % 3 == 0 else pool[rng.randint(0, len(pool) - (trial % 3 == 1), K)]
        n_nan += bool(np.isnan(v).any())
        assert M.argmax_first(v) == int(np.argmax(v)), v
    assert n_nan > 300
    assert M.argmax_first(np.array([-0.0, 0.0], np.float32)) == 0 and M.argmax_first(np.array([0.0, -0.0, np.nan, np.inf, np.nan], np.float32)) == 2
    assert M.argmax_first(np.array([-np.inf, -np.inf], np.float32)) == 0 and M.argmax_first(np.array([1.0, np.inf, np.inf], np.float32)) == 1


def test_answer_strings_reads_code_points():
    ans = torch.tensor([[104, 105, 0, 0], [0x3c3, 0, 0, 0], [0, 0, 0, 0]], dtype=torch.int32)
    assert M.answer_strings(ans, torch.tensor([2, 1, 0], dtype=torch.int32)) == ["hi", "σ", ""]


# ---------------------------------------------------------------------------------------------------------------- the ninth header
def _sig():
    from ctypes import c_int as i, c_void_p as vp
    return [vp] * 12 + [i] * 10 + [vp] * 11


def test_the_entry_point_is_bound_from_its_own_header():
    from ctypes import c_int
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    assert _capi.HEADER_SIGNATURES["eval"] == {"sam_eval_beams": _sig()} and _capi.HEADER_RESTYPES["eval"] == {"sam_eval_beams": c_int}
    assert "sam_eval_beams" not in _capi.SIGNATURES and "sam_eval_beams" not in _capi.NO_STATUS
    for name, other in dict(_capi.HEADER_SIGNATURES, abi=_capi.SIGNATURES).items():          # every other header of the registry
        assert name == "eval" or not set(other) & set(_capi.HEADER_SIGNATURES["eval"])
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_eval_beams.argtypes == _sig() and l.sam_eval_beams.restype is c_int
    assert os.path.join(b.CSRC, "eval_beams.hip") in b.sources()


def test_a_wrong_signature_in_a_copy_of_the_header_is_refused(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    text = open(b.HEADERS["eval"]).read()
    other = tmp_path / "sam_hip_eval.h"
    for old, new, named in (("int B, int K,", "size_t B, int K,", "size_t B"), ("int sam_eval_beams(", "float sam_eval_beams(", "float sam_eval_beams"),
                            ("double* totals,", "sam_totals totals,", "sam_totals totals")):
        assert text.count(old) == 1
        other.write_text(text.replace(old, new))
        with pytest.raises(_capi.SamHipError, match="sam_hip_eval.h: cannot parse") as e:
            _capi.parse_header(other.read_text(), _capi.STRUCTS, header="sam_hip_eval.h")
        assert named in str(e.value)
    _, sigs, rets, consts = _capi.parse_header(text, _capi.STRUCTS, header="sam_hip_eval.h")          # the header as committed: one function, no constant
    assert list(sigs) == ["sam_eval_beams"] and set(consts) == set()
    was = b._digest()                                                                                 # ... and the build's digest covers it
    other.write_text(text + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "eval", str(other))
    assert b._digest() != was
    assert b.SOURCE_INCLUDES["eval_beams.hip"] == ("score.hip",)
    src = open(os.path.join(b.CSRC, "eval_beams.hip")).read()
    assert '#include "score.hip"' in src and '#include "score_walk.h"' in src and "kWordMap[] = {" not in src


OK = dict(B=2, K=5, S=12, skip=1, A=10, Lg=128, No=50, Lw=32, V=5000, eos=2)
INPUTS = ("seqs", "cum", "meta", "gt_norm", "gt_norm_len", "gt_score", "gt_raw", "gt_raw_len", "ocr", "ocr_len", "vocab_cp", "vocab_len")
OUTPUTS = ("beam_scores", "beam_flags", "best", "best_ids", "best_scores", "best_flags", "oracle", "answer", "answer_len")


def _args(d, null=None):
    from ctypes import c_void_p
    p = {n: (None if n == null else c_void_p(0x1000)) for n in INPUTS + OUTPUTS}
    return tuple(p[n] for n in INPUTS) + tuple(d[k] for k in ("B", "K", "S", "skip", "A", "Lg", "No", "Lw", "V", "eos")) + tuple(p[n] for n in OUTPUTS) + (None, None)


@pytest.mark.parametrize("name,change,null,code,word", [
    ("null input", {}, "cum", "ARG", "null pointer among the inputs"), ("null table", {}, "ocr_len", "ARG", "null pointer among the inputs"),
    ("null output", {}, "answer", "ARG", "null pointer among the outputs"),
    ("K 0", dict(K=0), None, "ARG", "bad shape"), ("K 65", dict(K=65), None, "UNSUPPORTED", "K=65"), ("no batch", dict(B=0), None, "ARG", "bad shape"),
    ("L 65", dict(S=66), None, "UNSUPPORTED", "L=65"), ("skip = S", dict(skip=12), None, "ARG", "skip=12"), ("skip > S", dict(skip=13), None, "ARG", "skip=13"),
    ("skip < 0", dict(skip=-1), None, "ARG", "skip=-1"), ("Lg 256", dict(Lg=256), None, "UNSUPPORTED", "Lg=256"), ("Lg 0", dict(Lg=0), None, "ARG", "bad shape"),
    ("LDS", dict(S=65, Lw=64), None, "UNSUPPORTED", "LDS"), ("negative slots", dict(No=-1), None, "ARG", "bad shape"),
])
def test_argument_rejections_come_before_any_device_call(name, change, null, code, word):
    from sam_textvqa_amd import _capi
    rc = _capi.lib().sam_eval_beams(*_args(dict(OK, **change), null))
    assert rc == _capi.CONSTANTS["SAM_ERR_" + code] == {"ARG": -1, "UNSUPPORTED": -2}[code], name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_eval_beams:") and word in msg, msg


def test_ops_wrapper_rejects_cpu_tensors_and_wrong_shapes(golden):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    with pytest.raises(SamHipError):          # CPU tensors: rejected, no fallback
        ops.eval_beams(torch.from_numpy(golden["seqs"]), torch.from_numpy(golden["cum"]).reshape(-1), golden["table"], golden["vt"]["cp"], golden["vt"]["len"],
                       golden["vt"]["eos"], golden["K"])
