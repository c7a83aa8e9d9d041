"""CPU (no GPU needed): beam-search answers chosen by string (sam_textvqa_amd/metrics.py evaluate_beams_merged_host, include/sam_hip_beam_merge.h;
DESIGN.md §3.29).  The definition is this project's own, so there is no golden file: these tests pin it on hand-built tables -- which beams merge (a
vocabulary id and an OCR slot of one word, two OCR slots of one text, "joe" + "'s" and "joe's", ids behind EOS, empty strings) and which do not (a proper
prefix, a different last code point, a beam with an out-of-range id), the mass, the two arg-max rules with ties, NaN and -inf, K = 1, the totals -- and the
entry point's argument checks, its place in the header registry and its layout.  tests/test_beam_merge_gpu.py holds the kernel to this twin."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd.layouts import EVAL_BEAMS, EVAL_MERGED, EVAL_ROWS

WORDS = ["<pad>", "<s>", "</s>", "<unk>", "stop", "shop", "joe", "'s", "joe's", "stops", "go", "cat", "car"]
PAD, BOS, EOS, UNK, STOP, SHOP, JOE, S, JOES, STOPS, GO, CAT, CAR = range(13)
V = len(WORDS)
TOKENS = ["stop", "exit", "exit", "joe"]             # OCR slots V .. V + 3; slot V + 4 is the dataset's "<pad>"
O_STOP, O_EXIT, O_EXIT2, O_JOE, O_PAD = range(V, V + 5)
CAPS = M.ScoreTableCaps(10, 8, 16)
L = 4
NEW = ("beam_answer", "beam_answer_len", "group", "mass", "n_groups", "plain_best", "best_mass")


@pytest.fixture(scope="module")
def world():
    voc = A.AnswerVocab(WORDS)
    assert voc.EOS_IDX == EOS and len(voc) == V
    one = M.build_score_table(["stop"] * 6 + ["joe's"] * 3 + ["exit"], TOKENS, max_ocr_tokens=5)
    return (lambda B: M.collate_score_tables([one] * B, CAPS)), M.vocab_text(voc, max_word=CAPS.Lw)


def beams(world, questions, cums, **kw):
    """questions: per question its K id rows (padded with EOS to L columns here); cums: per question its K cumulative scores -> (twin result, seqs, cum)"""
    table, vt = world
    K = len(questions[0])
    seqs = np.array([(list(row) + [EOS] * L)[:L] for q in questions for row in q], np.int64)
    cum = np.array([c for q in cums for c in q], np.float32)
    return M.evaluate_beams_merged_host(seqs, cum, table(len(questions)), vt, K, skip=0, **kw), seqs, cum


def texts(res):
    return M.answer_strings(res["beam_answer"], res["beam_answer_len"])


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def lse(*p):
    return np.float32(math.log(sum(p)))


def test_all_strings_distinct_is_the_plain_evaluation(world):
    qs = [[[STOP], [SHOP], [O_EXIT], [JOES], [GO, STOP]], [[CAT], [CAR], [STOPS], [EOS], [O_PAD]]]
    cums = [[-1.5, -0.25, -3.0, -0.25, -2.0], [-2.0, -1.0, -0.5, -0.75, -0.5]]
    res, seqs, cum = beams(world, qs, cums)
    plain = M.evaluate_beams_host(seqs, cum, world[0](2), world[1], 5, skip=0)
    assert tuple(res) == M.EVAL_MERGED_KEYS == EVAL_MERGED.keys and M.EVAL_MERGED_KEYS[:9] == M.EVAL_BEAMS_KEYS and M.EVAL_MERGED_KEYS[9:] == NEW
    for k in M.EVAL_BEAMS_KEYS:
        assert res[k].dtype == plain[k].dtype and res[k].shape == plain[k].shape and res[k].tobytes() == plain[k].tobytes(), k
    assert res["group"].tolist() == [0, 1, 2, 3, 4] * 2 and res["n_groups"].tolist() == [5, 5]
    assert np.array_equal(bits(res["mass"]), bits(cum)) and np.array_equal(res["plain_best"], res["best"]) and res["best"].tolist() == [1, 2]
    assert np.array_equal(bits(res["best_mass"]), bits([-0.25, -0.5]))
    assert texts(res) == ["stop", "shop", "exit", "joe's", "go stop", "cat", "car", "stops", "", "<pad>"]
    for r, s in enumerate(texts(res)):                 # zeros behind the length
        assert not res["beam_answer"][r, len(s):].any()
    assert M.answer_strings(res["answer"], res["answer_len"]) == ["shop", "stops"]


def test_a_vocabulary_id_and_an_ocr_slot_of_one_word_merge_and_so_do_two_slots_of_one_text(world):
    p = np.log(np.array([0.4, 0.3, 0.3])).astype(np.float32)
    res, _, cum = beams(world, [[[SHOP], [STOP], [O_STOP]], [[O_EXIT2, GO], [STOP], [O_EXIT, GO]]], [p, [-1.0, -0.9, -1.0]])
    assert res["group"].tolist() == [0, 1, 1, 0, 1, 0] and res["n_groups"].tolist() == [2, 2]
    assert res["plain_best"].tolist() == [0, 1] and res["best"].tolist() == [1, 0]          # within the winning group the first of two equal cum
    assert bits(res["mass"][1]) == bits(res["mass"][2]) == bits(res["best_mass"][0]) and abs(float(res["mass"][1]) - math.log(0.6)) <= 1e-6
    assert bits(res["mass"][0]) == bits(cum[0])
    want = np.float32(-1.0 + math.log(2.0))
    assert bits(res["mass"][3]) == bits(res["mass"][5]) == bits(want) and bits(res["mass"][4]) == bits(cum[4]) and bits(res["best_mass"][1]) == bits(want)
    assert M.answer_strings(res["answer"], res["answer_len"]) == ["stop", "exit go"]
    assert res["best_ids"].tolist() == [[STOP, EOS, EOS, EOS], [O_EXIT2, GO, EOS, EOS]]
    assert np.array_equal(res["best_scores"], res["beam_scores"][[1, 3]]) and res["best_scores"][0, 1] == 1.0          # "stop" is the ground truth


def test_a_split_possessive_merges_with_the_single_token(world):
    res, _, cum = beams(world, [[[JOES], [JOE, S], [STOP], [O_JOE, S, GO], [O_JOE, S]]], [[-2.0, -1.5, -1.0, -0.1, -2.5]])
    assert texts(res) == ["joe's", "joe's", "stop", "joe's go", "joe's"]
    assert res["group"].tolist() == [0, 0, 2, 3, 0] and res["n_groups"].tolist() == [3]
    assert res["plain_best"].tolist() == [3] and res["best"].tolist() == [3]          # three beams of mass log(e^-2 + e^-1.5 + e^-2.5) do not reach e^-0.1
    assert abs(float(res["mass"][0]) - math.log(math.exp(-2.0) + math.exp(-1.5) + math.exp(-2.5))) <= 1e-6 and bits(res["mass"][3]) == bits(cum[3])


def test_ids_behind_eos_do_not_split_a_group_and_empty_strings_are_one_group(world):
    res, _, _ = beams(world, [[[STOP, EOS, SHOP, STOPS], [STOP], [EOS, STOP], [SHOP], [EOS]]], [[-1.2, -1.2, -2.0, -0.8, -2.0]])
    assert texts(res) == ["stop", "stop", "", "shop", ""]
    assert res["group"].tolist() == [0, 0, 2, 3, 2] and res["n_groups"].tolist() == [3]
    assert res["best"].tolist() == [0] and res["plain_best"].tolist() == [3]          # log 2 - 1.2 = -0.507 beats -0.8
    assert res["best_ids"].tolist() == [[STOP, EOS, SHOP, STOPS]] and res["answer_len"].tolist() == [4]
    assert bits(res["mass"][2]) == bits(res["mass"][4]) == bits(np.float32(-2.0 + math.log(2.0)))


def test_a_proper_prefix_and_a_different_last_code_point_do_not_merge(world):
    res, _, cum = beams(world, [[[STOP], [STOPS], [STOP, GO], [CAT], [CAR], [GO, STOP]]], [[-1.0] * 6])
    assert texts(res) == ["stop", "stops", "stop go", "cat", "car", "go stop"]
    assert res["group"].tolist() == [0, 1, 2, 3, 4, 5] and res["n_groups"].tolist() == [6] and np.array_equal(bits(res["mass"]), bits(cum))
    assert res["best"].tolist() == [0] == res["plain_best"].tolist()


def test_a_beam_with_an_out_of_range_id_stays_alone(world):
    bad = V + 5                                        # one past the last OCR slot
    res, _, cum = beams(world, [[[STOP, bad], [STOP], [STOP, -1, GO], [O_STOP], [SHOP]]], [[-0.9, -1.5, -0.9, -1.5, -1.0]])
    assert texts(res)[:4] == ["stop"] * 4 and (res["beam_flags"] & 1).tolist() == [1, 0, 1, 0, 0]
    assert res["group"].tolist() == [0, 1, 2, 1, 4] and res["n_groups"].tolist() == [4]
    assert bits(res["mass"][0]) == bits(cum[0]) and bits(res["mass"][2]) == bits(cum[2])
    assert res["best"].tolist() == [1] and res["plain_best"].tolist() == [0]          # log 2 - 1.5 = -0.807: the two clean beams together beat each flagged one
    assert res["best_flags"].tolist() == [0]


def test_ties_between_groups_go_to_the_lower_leader(world):
    res, _, _ = beams(world, [[[SHOP], [STOP], [SHOP], [O_STOP]], [[GO], [STOP], [SHOP], [CAT]]], [[-1.0, -2.0, -2.0, -1.0], [-3.0, -1.0, -1.0, -1.0]])
    assert res["group"].tolist() == [0, 1, 0, 1, 0, 1, 2, 3]
    assert bits(res["mass"][0]) == bits(res["mass"][1])                      # two terms: the sum does not depend on their order
    assert res["best"].tolist() == [0, 1] and res["plain_best"].tolist() == [0, 1]
    res, _, _ = beams(world, [[[SHOP], [STOP], [SHOP], [O_STOP]]], [[-2.0, -1.0, -1.0, -2.0]])
    assert res["best"].tolist() == [2] and res["plain_best"].tolist() == [1]          # group 0 wins the tie, its representative is its larger member


def test_nan_follows_argmax_first_inside_a_group_and_across_groups(world):
    nan = np.float32(np.nan)
    res, _, cum = beams(world, [[[SHOP], [STOP], [O_STOP], [CAT]],          # a NaN member: the group's mass is NaN, it wins, the NaN member stands for it
                                [[SHOP], [STOP], [O_STOP], [CAT]],          # a NaN single beam behind a NaN group: the first NaN leader wins
                                [[CAT], [STOP], [O_STOP], [SHOP]]],         # a NaN single beam in front
                        [[5.0, -1.0, nan, 7.0], [0.0, nan, -1.0, nan], [nan, -1.0, nan, 0.0]])
    assert res["group"].tolist() == [0, 1, 1, 3] * 3
    assert np.isnan(res["mass"]).tolist() == [False, True, True, False, False, True, True, True, True, True, True, False]
    assert res["best"].tolist() == [2, 1, 0] and res["plain_best"].tolist() == [2, 1, 0] and np.isnan(res["best_mass"]).all()
    assert bits(res["mass"][0]) == bits(cum[0]) and bits(res["mass"][8]) == bits(cum[8])
    assert M.argmax_first([np.float32(1.0), nan, nan]) == 1


def test_minus_infinity_members_add_nothing(world):
    inf = np.float32(np.inf)
    res, _, cum = beams(world, [[[STOP], [SHOP], [O_STOP], [O_STOP, EOS, GO]], [[STOP], [O_STOP], [SHOP], [SHOP]]],
                        [[-inf, -1.0, -1.25, -inf], [-inf, -inf, -inf, -inf]])
    assert res["group"].tolist() == [0, 1, 0, 0, 0, 0, 2, 2]
    assert bits(res["mass"][0]) == bits(res["mass"][2]) == bits(res["mass"][3]) == bits(np.float32(-1.25))          # -1.25 + log(0 + 1 + 0)
    assert res["best"].tolist() == [1, 0] and res["plain_best"].tolist() == [1, 0]
    assert np.array_equal(bits(res["mass"][4:]), bits([-inf] * 4)) and bits(res["best_mass"][1]) == bits(-inf)
    assert bits(M.group_mass([-inf, -inf])) == bits(-inf) and bits(M.group_mass([inf])) == bits(inf) and np.isnan(M.group_mass([inf, 0.0]))


def test_one_beam_per_question(world):
    res, seqs, cum = beams(world, [[[STOP]], [[EOS]], [[JOE, S]]], [[-0.5], [np.nan], [-np.inf]])
    plain = M.evaluate_beams_host(seqs, cum, world[0](3), world[1], 1, skip=0)
    assert all(res[k].tobytes() == plain[k].tobytes() for k in M.EVAL_BEAMS_KEYS)
    assert res["group"].tolist() == [0, 0, 0] and res["n_groups"].tolist() == [1, 1, 1] and res["plain_best"].tolist() == [0, 0, 0]
    assert np.array_equal(bits(res["mass"]), bits(cum)) and np.array_equal(bits(res["best_mass"]), bits(cum)) and texts(res) == ["stop", "", "joe's"]


def test_mass_is_the_log_of_the_summed_probabilities():
    rng = np.random.RandomState(0)
    for n in (2, 3, 5, 64):
        c = np.log(rng.rand(n) * 0.9 + 0.05).astype(np.float32) - rng.randint(0, 30)
        want = np.logaddexp.reduce(c.astype(np.float64))
        assert abs(float(M.group_mass(c)) - want) <= 2.0 ** -24 * abs(want) * 1.01 + 1e-12          # float64 inside, one rounding to fp32


def test_totals_accumulate_in_host_totals_order(world):
    qs, cums = [[[SHOP], [STOP], [O_STOP]], [[JOES], [GO], [JOE, S]], [[CAT], [CAR], [EOS]]], [[-1.0, -1.2, -1.2]] * 3
    tot = np.zeros(4)
    res, seqs, cum = beams(world, qs, cums, totals=tot)
    assert np.array_equal(tot, M.host_totals(res["best_scores"])) and tot[3] == 3 and tot[1] == 2.0          # "stop" and "joe's" are ground truths
    res2, _, _ = beams(world, qs[::-1], cums, totals=tot)
    assert np.array_equal(tot, M.host_totals(res["best_scores"]) + M.host_totals(res2["best_scores"])) and tot[3] == 6
    for bad in (dict(beam=2), dict(beam=0), dict(skip=L), dict(skip=-1)):
        with pytest.raises(ValueError, match="evaluate_beams_host"):
            M.evaluate_beams_merged_host(seqs, cum, world[0](3), world[1], **dict(dict(beam=3, skip=0), **bad))


# ---------------------------------------------------------------------------------------------- registry, layout and C ABI
def test_the_header_is_registered_in_the_open_table_and_the_layout_is_its_run_of_outputs():
    from sam_textvqa_amd import _build, _capi, ops
    from tests.test_layouts_cpu import run_of
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert "beam_merge" in _build.ABI_ADDITIONS and _build.ABI_ADDITIONS["beam_merge"] in _build.public_headers()
    assert os.path.basename(_build.ABI_ADDITIONS["beam_merge"]) == "sam_hip_beam_merge.h"
    assert not {"beam_merge"} & (set(_build.HEADERS) | set(_build.ABI_PARTS) | set(_build.ABI_EXTENSIONS))
    assert _capi.ADDITION_SIGNATURES["beam_merge"] == {"sam_eval_beams_merged": [vp] * 12 + [i] * 10 + [vp] * 16 + [vp, vp]}
    assert _capi.ADDITION_RESTYPES["beam_merge"] == {"sam_eval_beams_merged": i}
    assert _capi.ADDITION_SIGNATURES["beam_merge"]["sam_eval_beams_merged"][:31] == _capi.HEADER_SIGNATURES["eval"]["sam_eval_beams"][:31]
    assert os.path.join(_build.CSRC, "beam_merge.hip") in _build.sources() and _build.SOURCE_INCLUDES["beam_merge.hip"] == ("score.hip",)
    src = open(os.path.join(_build.CSRC, "beam_merge.hip")).read()          # the scoring code is the one copy
    assert '#include "score_walk.h"' in src and "block_score(" in src and "wave_levenshtein" not in src and "kWordMap[] = {" not in src
    lib = _capi.lib()
    assert lib.sam_build_digest().decode() == _build._digest()
    assert lib.sam_eval_beams_merged.argtypes == _capi.ADDITION_SIGNATURES["beam_merge"]["sam_eval_beams_merged"] and lib.sam_eval_beams_merged.restype is i
    assert run_of("sam_eval_beams_merged", "beam_scores", 16) == list(EVAL_MERGED.fields)
    assert run_of("sam_eval_beams_merged", "seqs", 12) == run_of("sam_eval_beams", "seqs", 12)
    assert ops.EVAL_MERGED_KEYS == M.EVAL_MERGED_KEYS == EVAL_MERGED.keys


def test_the_layout_extends_eval_beams_and_a_twin_result_passes_the_board_row_checks(world):
    from sam_textvqa_amd import ops
    from tests.test_layouts_cpu import Fake
    assert EVAL_MERGED.keys[:9] == EVAL_BEAMS.keys and EVAL_MERGED.fields[:9] == EVAL_BEAMS.fields and EVAL_MERGED.keys[9:] == NEW
    for dims in (dict(B=2, K=3, L=4, Lw=8), dict(B=1, K=1, L=0, Lw=5)):
        assert list(EVAL_MERGED.shapes(**dims).items())[:9] == list(EVAL_BEAMS.shapes(**dims).items())
    assert list(EVAL_MERGED.shapes(B=2, K=3, L=4, Lw=8).items())[9:] == [("beam_answer", (6, 36)), ("beam_answer_len", (6,)), ("group", (6,)), ("mass", (6,)),
                                                                        ("n_groups", (2,)), ("plain_best", (2,)), ("best_mass", (2,))]
    assert [(k, tuple(v.shape), v.dtype) for k, v in ops.eval_beams_merged_outputs(2, 3, 4, 8, "cpu").items()] == \
        [(k, s, EVAL_MERGED.torch_dtypes[k]) for k, s in EVAL_MERGED.shapes(B=2, K=3, L=4, Lw=8).items()]
    res, _, _ = beams(world, [[[SHOP], [STOP], [O_STOP]], [[JOES], [GO], [JOE, S]]], [[-1.0, -1.2, -1.2]] * 2)
    EVAL_MERGED.check_host(res, "twin", B=2, K=3, L=L, Lw=CAPS.Lw)
    fake = {k: Fake(v.shape, getattr(torch, str(v.dtype))) for k, v in res.items()}          # what the GPU checks read of a tensor
    EVAL_ROWS.require(fake, ops._GPU, "evalboard_collect: res")
    EVAL_ROWS.check(fake, ops._GPU, "evalboard_collect: res", B=2, P=L * (CAPS.Lw + 1))
    EVAL_MERGED.check(fake, ops._GPU, "eval_beams_merged: out", B=2, K=3, L=L, Lw=CAPS.Lw)


OK = dict(B=2, K=5, S=12, skip=1, A=10, Lg=128, No=50, Lw=32, V=5000, eos=2)
INPUTS = ("seqs", "cum", "meta", "gt_norm", "gt_norm_len", "gt_score", "gt_raw", "gt_raw_len", "ocr", "ocr_len", "vocab_cp", "vocab_len")
OUTPUTS = EVAL_MERGED.keys


def _args(d, null=None):
    p = {n: (None if n == null else ctypes.c_void_p(0x1000)) for n in INPUTS + OUTPUTS}          # never dereferenced: the checks come before any launch
    return tuple(p[n] for n in INPUTS) + tuple(d[k] for k in ("B", "K", "S", "skip", "A", "Lg", "No", "Lw", "V", "eos")) + tuple(p[n] for n in OUTPUTS) + (None, None)


@pytest.mark.parametrize("name,change,null,code,word", [
    ("K 65", dict(K=65), None, "UNSUPPORTED", "K=65"), ("L 65", dict(S=66), None, "UNSUPPORTED", "L=65"), ("skip = S", dict(skip=12), None, "ARG", "skip=12"),
    ("skip < 0", dict(skip=-1), None, "ARG", "skip=-1"), ("Lg 256", dict(Lg=256), None, "UNSUPPORTED", "Lg=256"), ("LDS", dict(S=65, Lw=64), None, "UNSUPPORTED", "LDS"),
    ("K 0", dict(K=0), None, "ARG", "bad shape"), ("null input", {}, "cum", "ARG", "null pointer among the inputs"),
    ("null old output", {}, "answer", "ARG", "null pointer among the outputs")] +
    [("null " + k, {}, k, "ARG", "null pointer among the outputs") for k in NEW])
def test_argument_errors_are_reported_without_a_gpu(name, change, null, code, word):
    from sam_textvqa_amd import _capi
    rc = _capi.lib().sam_eval_beams_merged(*_args(dict(OK, **change), null))
    assert rc == _capi.CONSTANTS["SAM_ERR_" + code] == {"ARG": -1, "UNSUPPORTED": -2}[code], name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_eval_beams_merged:") and word in msg, msg


def test_the_wrappers_reject_cpu_tensors_and_unknown_merge_modes(world):
    from sam_textvqa_amd import evaluator as E, ops
    from sam_textvqa_amd._capi import SamHipError
    table, vt = world
    with pytest.raises(SamHipError):                   # CPU tensors: rejected, no fallback
        ops.eval_beams_merged(torch.zeros(3, L, dtype=torch.int64), torch.zeros(3), table(1), vt["cp"], vt["len"], vt["eos"], 3, skip=0)
    for call in (lambda: E.evaluate(None, [], vt, 3, merge="normalised"), lambda: E.evaluate_indexed(None, [], vt, 3, None, merge=True)):
        with pytest.raises(ValueError, match="merge = "):          # refused before the model is touched
            call()
