"""CPU: the one description of the four tensor tables that cross the C ABI as a run of pointers (sam_textvqa_amd/layouts.py) -- held against the
prototypes under include/, against the shapes the allocators produced before the description existed (written out here, not computed from it), against
the names callers import, and against what the launch wrappers' argument checks accepted and refused.

The GPU-side checks run here on stand-ins that claim to be contiguous GPU tensors: a CPU tensor gets no further than "must live on the GPU", so the
device and contiguity requirements themselves are exercised only that far; nothing here pretends otherwise."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from sam_textvqa_amd import layouts as Y
from sam_textvqa_amd.layouts import ANSWER_TABLE, ANSWER_TABLE_OUT, EVAL_BEAMS, EVAL_BOARD, EVAL_ROWS, SCORE_TABLE, SCORE_TABLE_OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i16, i32, i64, f32 = torch.int16, torch.int32, torch.int64, torch.float32
C_TYPES = {"int32_t": "int32", "int16_t": "int16", "int64_t": "int64", "float": "float32"}


# ---------------------------------------------------------------------------------------------- the public headers
def pointer_params(function):
    """[(name, pointee C type)] of the pointer parameters of `function`, in order, from the header text that declares it"""
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        m = re.search(r"^int %s\((.*?)\);" % function, text, flags=re.S | re.M)
        if m:
            params = [re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", " ".join(p.split())) for p in m.group(1).split(",")]
            assert all(params), (function, m.group(1))
            return [(p.group(3), p.group(1)) for p in params if p.group(2)]
    raise AssertionError("no prototype of %s under include/" % function)


def run_of(function, first, count, prefix="", rename=()):
    """the `count` pointer parameters of `function` from the one named prefix + first on -> [(key, dtype name)]"""
    params = pointer_params(function)
    at = [name for name, _ in params].index(prefix + first)
    run = params[at:at + count]
    assert all(name.startswith(prefix) for name, _ in run), run
    return [(dict(rename).get(name[len(prefix):], name[len(prefix):]), C_TYPES[ctype]) for name, ctype in run]


def described(layout):
    return list(layout.fields)


@pytest.mark.parametrize("layout, function, first, prefix, rename", [
    (ANSWER_TABLE, "sam_answer_sample", "meta", "", ()),
    (ANSWER_TABLE, "sam_bce_loss_table", "meta", "", ()),
    (ANSWER_TABLE_OUT, "sam_answer_table_from_text", "meta", "", ()),
    (SCORE_TABLE, "sam_score_answers", "meta", "", ()),
    (SCORE_TABLE, "sam_eval_beams", "meta", "", ()),
    (SCORE_TABLE_OUT, "sam_score_table_from_text", "meta", "", (("ocr_out_len", "ocr_len"),)),         # (ocr_len names the INPUT lengths there)
    (EVAL_BEAMS, "sam_eval_beams", "beam_scores", "", ()),
    (EVAL_ROWS, "sam_evalboard_collect", "best_scores", "", ()),
    (EVAL_BOARD, "sam_evalboard_collect", "scores", "board_", ()),
    (EVAL_BOARD, "sam_evalboard_merge", "scores", "dst_", ()),
    (EVAL_BOARD, "sam_evalboard_merge", "scores", "src_", ()),
])
def test_the_layouts_are_the_headers_pointer_runs(layout, function, first, prefix, rename):
    assert run_of(function, first, len(layout.keys), prefix, rename) == described(layout)
    for k, d in layout.fields:
        assert layout.np_dtypes[k] == np.dtype(d) and layout.torch_dtypes[k] is getattr(torch, d)


def test_the_header_comparison_sees_a_reordered_and_a_retyped_key():
    f = list(ANSWER_TABLE.fields)
    swapped = Y.Layout("t", [f[1], f[0]] + f[2:], None)
    retyped = Y.Layout("t", [f[0], f[1], ("seq_grp", "int32")] + f[3:], None)
    want = run_of("sam_answer_sample", "meta", 8)
    assert described(ANSWER_TABLE) == want and described(swapped) != want and described(retyped) != want


# ---------------------------------------------------------------------------------------------- what the allocators produced
B, S, L, G, E, A, Lg, No, Lw, K, n, P = 2, 3, 2, 4, 5, 2, 3, 3, 4, 2, 3, 6
ANSWER_WANT = {"meta": ((2, 4), i32), "seq_len": ((2, 3), i32), "seq_grp": ((2, 3, 2), i16), "step0_idx": ((2, 3), i32), "step0_val": ((2, 3), f32),
               "grp_idx": ((2, 4), i32), "grp_off": ((2, 5), i32), "grp_extra": ((2, 5), i32)}
STATUS_WANT = {"status": ((2,), i32)}


def score_want(slots):
    return {"meta": ((2, 4), i32), "gt_norm": ((2, 2, 3), i32), "gt_norm_len": ((2, 2), i32), "gt_score": ((2, 2), f32), "gt_raw": ((2, 2, 3), i32),
            "gt_raw_len": ((2, 2), i32), "ocr": ((2, slots, 4), i32), "ocr_len": ((2, slots), i32)}


def beams_want(steps):
    return {"beam_scores": ((4, 3), f32), "beam_flags": ((4,), i32), "best": ((2,), i32), "best_ids": ((2, steps), i64), "best_scores": ((2, 3), f32),
            "best_flags": ((2,), i32), "oracle": ((2, 3), f32), "answer": ((2, steps * 5), i32), "answer_len": ((2,), i32)}


BOARD_WANT = {"scores": ((3, 3), f32), "oracle": ((3, 3), f32), "flags": ((3,), i32), "best": ((3,), i32), "answer": ((3, 6), i32), "answer_len": ((3,), i32),
              "seen": ((3,), i32), "status": ((1,), i32)}
NP_OF = {i16: np.int16, i32: np.int32, i64: np.int64, f32: np.float32}


def as_listed(d):
    """[(key, shape, dtype)] in the dict's own order: keys, order, shapes and dtypes in one comparison"""
    return [(k, tuple(v.shape), v.dtype) for k, v in d.items()]


def listed(want, numpy=False):
    return [(k, s, np.dtype(NP_OF[d]) if numpy else d) for k, (s, d) in want.items()]


def test_layout_allocations_are_what_the_allocators_produced():
    a, s = dict(B=B, S=S, L=L, G=G, E=E), dict(B=B, A=A, Lg=Lg, Lw=Lw)
    assert as_listed(ANSWER_TABLE.zeros_host(**a)) == listed(ANSWER_WANT, numpy=True)
    assert as_listed(ANSWER_TABLE.empty("cpu", **a)) == as_listed(ANSWER_TABLE.zeros("cpu", **a)) == listed(ANSWER_WANT)
    assert as_listed(ANSWER_TABLE_OUT.empty("cpu", **a)) == listed(dict(ANSWER_WANT, **STATUS_WANT))
    assert list(ANSWER_TABLE.shapes(**a).items()) == [(k, sh) for k, (sh, _) in ANSWER_WANT.items()]
    for slots in (1, 3):                                        # the builders allocate max(No, 1) OCR slots: No = 0 and No = 3
        assert as_listed(SCORE_TABLE.zeros_host(No=slots, **s)) == listed(score_want(slots), numpy=True)
        assert as_listed(SCORE_TABLE_OUT.empty("cpu", No=slots, **s)) == listed(dict(score_want(slots), **STATUS_WANT))
    for steps in (0, 2):
        assert as_listed(EVAL_BEAMS.empty("cpu", B=B, K=K, L=steps, Lw=Lw)) == listed(beams_want(steps))
        assert as_listed(EVAL_BEAMS.zeros_host(B=B, K=K, L=steps, Lw=Lw)) == listed(beams_want(steps), numpy=True)
    assert as_listed(EVAL_BOARD.zeros_host(n=n, P=P)) == listed(BOARD_WANT, numpy=True)
    assert as_listed(EVAL_BOARD.zeros("cpu", n=n, P=P)) == listed(BOARD_WANT)
    assert list(EVAL_ROWS.shapes(B=B, P=P).items()) == [("best_scores", (2, 3)), ("oracle", (2, 3)), ("best_flags", (2,)), ("best", (2,)), ("answer", (2, 6)),
                                                        ("answer_len", (2,))]
    assert not any(v.any() for v in EVAL_BOARD.zeros_host(n=n, P=P).values()) and not any(v.any() for v in EVAL_BOARD.zeros("cpu", n=n, P=P).values())
    with pytest.raises(TypeError):
        ANSWER_TABLE.shapes(B=B, S=S, L=L, G=G)                 # a capacity left out is an error, not a default


def test_the_packages_allocators_go_through_the_layouts():
    from sam_textvqa_amd import answers, evalboard, metrics, ops
    caps = answers.AnswerTableCaps(S, L, G, E)
    one = {"dims": [9, 1, 2, L], "seq_len": [1], "seq_grp": [[0, 0]], "step0_idx": [3], "step0_val": [1.0], "grp_idx": [3], "grp_off": [0, 1], "grp_extra": []}
    table = answers.collate_answer_tables([one, one], caps)
    assert as_listed({k: table[k] for k in answers.TABLE_KEYS}) == listed(ANSWER_WANT) and list(table)[:8] == list(ANSWER_WANT)
    assert as_listed(answers.table_outputs(B, caps, "cpu")) == listed(dict(ANSWER_WANT, **STATUS_WANT))
    for ocr_slots, slots in ((0, 1), (3, 3)):
        assert as_listed(metrics.score_table_outputs(B, ocr_slots, metrics.ScoreTableCaps(A, Lw, Lg), "cpu")) == listed(dict(score_want(slots), **STATUS_WANT))
        sample = {"gt_norm": ["a"], "gt_score": np.ones(1, np.float32), "gt_raw": ["a"], "ocr": [[97]] * ocr_slots}
        assert as_listed(metrics.collate_score_tables([sample, sample], metrics.ScoreTableCaps(A, Lw, Lg))) == listed(score_want(slots))
    for steps in (0, 2):
        assert as_listed(ops.eval_beams_outputs(B, K, steps, Lw, "cpu")) == listed(beams_want(steps))
    assert as_listed(evalboard.new_host(n, P)) == listed(BOARD_WANT, numpy=True)
    assert as_listed(evalboard.Board(n, P, device="cpu").t) == listed(BOARD_WANT)


def test_the_imported_names_are_the_layouts_keys():
    from sam_textvqa_amd import answers, evalboard, metrics, ops
    assert ops.ANSWER_TABLE_KEYS == answers.TABLE_KEYS == ANSWER_TABLE.keys == tuple(ANSWER_WANT)
    assert ops.SCORE_TABLE_KEYS == metrics.SCORE_TABLE_KEYS == SCORE_TABLE.keys == tuple(score_want(1))
    assert ops.EVAL_BEAMS_KEYS == metrics.EVAL_BEAMS_KEYS == EVAL_BEAMS.keys == tuple(beams_want(1))
    assert ops.EVALBOARD_KEYS == evalboard.KEYS == EVAL_BOARD.keys == tuple(BOARD_WANT)
    assert ops.EVALBOARD_ROW_KEYS == evalboard.ROW_KEYS == EVAL_ROWS.keys == ("best_scores", "oracle", "best_flags", "best", "answer", "answer_len")
    assert ANSWER_TABLE_OUT.keys == ANSWER_TABLE.keys + ("status",) and SCORE_TABLE_OUT.keys == SCORE_TABLE.keys + ("status",)
    for row, key in zip(evalboard.ROW_KEYS, evalboard.KEYS[:6]):          # a result row and the board column it lands in: same dtype, same width
        assert EVAL_ROWS.torch_dtypes[row] is EVAL_BOARD.torch_dtypes[key]
        assert EVAL_ROWS.shapes(B=n, P=P)[row] == EVAL_BOARD.shapes(n=n, P=P)[key]
    src = open(Y.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(?!math|numpy|torch)\S+", src, flags=re.M)          # pure: numpy and torch only


# ---------------------------------------------------------------------------------------------- the acceptance rules
class Fake:
    """what the GPU checks read of a tensor, claiming to be a contiguous GPU tensor of this shape and dtype"""
    is_cuda, device = True, "cuda"

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype

    def numel(self):
        return math.prod(self.shape)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def fakes(want):
    return {k: Fake(s, d) for k, (s, d) in want.items()}


def without(d, k):
    return {j: v for j, v in d.items() if j != k}


def refused(call, error, *words):
    with pytest.raises(error) as e:
        call()
    assert type(e.value) is error and all(w in str(e.value) for w in words), str(e.value)


def test_the_gpu_checks_accept_and_refuse_what_the_written_out_loops_did():
    """each case: what the loop in ops.py raised before the layouts (exception type, key named, counts), recorded by running it on these stand-ins"""
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError as Err
    # the answer table: element count and leading dimension
    t, chk = fakes(ANSWER_WANT), ops._check_answer_table
    assert chk(t) == (B, S, L, G, E)
    refused(lambda: chk(without(t, "grp_off")), Err, "lacks 'grp_off'")
    refused(lambda: chk(dict(t, seq_grp=Fake((2, 3, 2), i32))), Err, "'seq_grp'", "expected dtype torch.int16, got torch.int32")
    refused(lambda: chk(dict(t, grp_off=Fake((2, 4), i32))), Err, "grp_off", "has 8 elements, expected 10", "B=2 S=3", "G=4 E=5")
    refused(lambda: chk(dict(t, seq_len=Fake((3, 2), i32))), Err, "seq_len", "has 6 elements, expected 6")          # right count, wrong leading dimension
    refused(lambda: chk(dict(t, seq_grp=Fake((2, 6), i16))), Err, "seq_grp must be [B, S, L]")                         # the flat view of seq_grp
    assert chk(dict(t, seq_len=Fake((2, 3, 1), i32))) == chk(dict(t, seq_len=Fake((2, 1, 3), i32))) == (B, S, L, G, E)          # a reshaped seq_len passes
    # the score table: the same rule, for as many samples as score_answers' predictions hold.  A table that passes gets as far as the next
    # argument, a scores buffer of the wrong dtype handed in for that purpose
    t, vocab = fakes(score_want(3)), (Fake((7, 4), i32), Fake((7,), i32))
    chk = lambda d, rows=2: ops.score_answers(Fake((rows, 5), i64), d, *vocab, 1, out=(Fake((rows, 3), i32), None))
    refused(lambda: chk(t), Err, "scores: expected dtype torch.float32")
    refused(lambda: chk(without(t, "gt_raw")), Err, "score table lacks 'gt_raw'")
    refused(lambda: chk(dict(t, gt_score=Fake((2, 2), i32))), Err, "'gt_score'", "expected dtype torch.float32, got torch.int32")
    refused(lambda: chk(dict(t, ocr_len=Fake((2, 4), i32))), Err, "ocr_len", "has 8 elements, expected 6", "B=2 A=2 Lg=3 No=3 Lw=4")
    refused(lambda: chk(dict(t, gt_norm_len=Fake((1, 4), i32))), Err, "gt_norm_len", "has 4 elements, expected 4")
    refused(lambda: chk(t, 3), Err, "meta", "has 8 elements, expected 12", "B=3")                    # a table of 2 samples for 3 predictions
    refused(lambda: chk(dict(t, ocr=Fake((2, 12), i32))), Err, "ocr [B, No, Lw]")
    refused(lambda: chk(dict(t, gt_score=Fake((2, 2, 1), f32))), Err, "scores: expected dtype torch.float32")          # a trailing unit dimension passes
    beams = lambda d: ops.eval_beams(Fake((4, 3), i64), Fake((4,), f32), d, *vocab, 1, 2, totals=Fake((4,), f32), out=fakes(beams_want(2)))
    refused(lambda: beams(t), Err, "totals: expected dtype torch.float64")                            # the same table under eval_beams: passes
    refused(lambda: beams(without(t, "gt_raw")), Err, "score table lacks 'gt_raw'")
    refused(lambda: beams(dict(t, ocr_len=Fake((2, 4), i32))), Err, "ocr_len", "has 8 elements, expected 6")
    # the board: element counts alone
    t, chk = fakes(BOARD_WANT), ops._board_shape
    assert chk(t, "evalboard_reduce") == (n, P)
    refused(lambda: chk(without(t, "seen"), "evalboard_reduce"), Err, "evalboard_reduce: board lacks 'seen'")
    refused(lambda: chk(without(t, "seen"), "evalboard_merge", "src"), Err, "evalboard_merge: src lacks 'seen'")
    refused(lambda: chk(dict(without(t, "seen"), scores=Fake((3, 3), i32)), "evalboard_reduce"), Err, "lacks 'seen'")          # absence is reported first
    refused(lambda: chk(dict(t, flags=Fake((3,), i64)), "evalboard_reduce"), Err, "board['flags']", "expected dtype torch.int32, got torch.int64")
    refused(lambda: chk(dict(t, status=Fake((2,), i32)), "evalboard_reduce"), Err, "evalboard_reduce: board['status'] has 2 elements, expected 1 (n=3 P=6)")
    refused(lambda: chk(dict(t, answer=Fake((18,), i32)), "evalboard_reduce"), Err, "['answer'] must be int32 [n, P]")
    assert chk(dict(t, scores=Fake((9,), f32)), "evalboard_reduce") == chk(dict(t, scores=Fake((1, 9), f32)), "evalboard_reduce") == (n, P)      # flat scores pass


def test_the_output_and_result_row_checks_accept_and_refuse_what_the_written_out_loops_did():
    """the dicts a caller hands in to be filled or read: a missing key of an out= dict is the dict's own KeyError, as it was"""
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError as Err

    def check(layout, d, name, who, required, **dims):
        if required:
            layout.require(d, ops._GPU, who + ": " + name)
        layout.check(d, ops._GPU, who + ": " + name, **dims)

    # eval_beams' out: element counts alone
    t, dims = fakes(beams_want(2)), dict(B=B, K=K, L=2, Lw=Lw)
    chk = lambda d: check(EVAL_BEAMS, d, "out", "eval_beams", False, **dims)
    chk(t)
    refused(lambda: chk(without(t, "best_ids")), KeyError, "best_ids")
    refused(lambda: chk(dict(t, best_ids=Fake((2, 2), i32))), Err, "out['best_ids']", "expected dtype torch.int64, got torch.int32")
    refused(lambda: chk(dict(t, answer=Fake((2, 9), i32))), Err, "eval_beams: out['answer'] has 18 elements, expected 20 (B=2 K=2 L=2 Lw=4)")
    chk(dict(t, beam_scores=Fake((3, 4), f32)))                 # 12 elements under another leading dimension pass
    # the result rows evalboard_collect reads: present, element counts alone
    t = fakes({k: beams_want(2)[k] for k in EVAL_ROWS.keys})
    t["answer"] = Fake((2, 6), i32)
    chk = lambda d: check(EVAL_ROWS, d, "res", "evalboard_collect", True, B=B, P=P)
    chk(t)
    refused(lambda: chk(without(t, "best")), Err, "evalboard_collect: res lacks 'best'")
    refused(lambda: chk(dict(t, best_flags=Fake((2,), f32))), Err, "res['best_flags']", "expected dtype torch.int32, got torch.float32")
    refused(lambda: chk(dict(t, answer=Fake((2, 7), i32))), Err, "evalboard_collect: res['answer'] has 14 elements, expected 12 (B=2 P=6)")
    chk(dict(t, answer=Fake((12,), i32)))                       # a flat answer block passes
    # the two *_from_text builders' out: the table's rule, status included
    t = fakes(dict(ANSWER_WANT, **STATUS_WANT))
    chk = lambda d: check(ANSWER_TABLE_OUT, d, "out", "answer_table_from_text", False, B=B, S=S, L=L, G=G, E=E)
    chk(t)
    refused(lambda: chk(without(t, "grp_off")), KeyError, "grp_off")
    refused(lambda: chk(without(t, "status")), KeyError, "status")
    refused(lambda: chk(dict(t, status=Fake((2,), i64))), Err, "out['status']", "expected dtype torch.int32, got torch.int64")
    refused(lambda: chk(dict(t, status=Fake((3,), i32))), Err, "answer_table_from_text: out['status'] has 3 elements, expected 2 (B=2 S=3 L=2 G=4 E=5)")
    refused(lambda: chk(dict(t, seq_len=Fake((3, 2), i32))), Err, "answer_table_from_text: out['seq_len'] has 6 elements, expected 6")
    chk(dict(t, step0_val=Fake((2, 3, 1), f32)))
    t = fakes(dict(score_want(3), **STATUS_WANT))
    chk = lambda d: check(SCORE_TABLE_OUT, d, "out", "score_table_from_text", False, B=B, A=A, Lg=Lg, No=No, Lw=Lw)
    chk(t)
    refused(lambda: chk(without(t, "ocr")), KeyError, "ocr")
    refused(lambda: chk(dict(t, gt_score=Fake((2, 2), i32))), Err, "out['gt_score']", "expected dtype torch.float32, got torch.int32")
    refused(lambda: chk(dict(t, ocr_len=Fake((2, 4), i32))), Err, "score_table_from_text: out['ocr_len'] has 8 elements, expected 6 (B=2 A=2 Lg=3 No=3 Lw=4)")
    refused(lambda: chk(dict(t, gt_raw_len=Fake((1, 4), i32))), Err, "score_table_from_text: out['gt_raw_len'] has 4 elements, expected 4")
    chk(dict(t, ocr=Fake((2, 12), i32)))                        # the flat [B, No * Lw] view passes here (the capacities come from the text)
    # a real CPU tensor gets as far as the device requirement
    refused(lambda: ops._check_answer_table(ANSWER_TABLE.zeros("cpu", B=B, S=S, L=L, G=G, E=E)), Err, "'meta'", "must live on the GPU")


def test_the_host_board_check_requires_exact_shapes_and_dtypes():
    from sam_textvqa_amd import evalboard
    h = evalboard.new_host(n, P)
    assert evalboard._host_shape(h) == (n, P)
    refused(lambda: evalboard._host_shape(without(h, "seen")), KeyError, "seen")
    refused(lambda: evalboard._host_shape(dict(h, flags=np.zeros(3, np.int64))), ValueError, "evalboard: board['flags'] is int64 (3,), expected int32 (3,)")
    refused(lambda: evalboard._host_shape(dict(h, status=np.zeros(2, np.int32))), ValueError, "evalboard: board['status'] is int32 (2,), expected int32 (1,)")
    refused(lambda: evalboard._host_shape(dict(h, scores=np.zeros(9, np.float32))), ValueError, "board['scores'] is float32 (9,), expected float32 (3, 3)")
    refused(lambda: evalboard._host_shape(dict(h, scores=np.zeros((1, 9), np.float32))), ValueError, "board['scores'] is float32 (1, 9), expected float32 (3, 3)")
    refused(lambda: evalboard._host_shape({k: torch.from_numpy(v) for k, v in h.items()}), ValueError, "board['scores'] is torch.float32")      # numpy only
    assert evalboard._host_shape(dict(h, answer=np.zeros((3, 2), np.int32))) == (3, 2)          # the board's shape is read off its answer block
