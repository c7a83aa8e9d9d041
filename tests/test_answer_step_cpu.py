"""CPU: the host side of the answer-table build's status record -- the binding of include/sam_hip_step.h, the argument
checks of sam_answer_status_fold, the host twin of its four-word record on hand-written cases, and collate_ragged packing the samples' answers."""
import ctypes

import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import ragged as R

RESET = list(A.STATUS_STATE_RESET)


# ---------------------------------------------------------------------------------------------- the binding and the entry point
def test_the_entry_point_is_bound_from_its_header_and_the_other_tables_are_untouched():
    from ctypes import c_int, c_int64, c_void_p as vp
    import os
    import sam_textvqa_amd._build as b
    from sam_textvqa_amd import _capi
    assert _capi.HEADER_SIGNATURES["step"] == {"sam_answer_status_fold": [vp, c_int, vp, c_int64, vp, vp]}
    assert _capi.HEADER_RESTYPES["step"] == {"sam_answer_status_fold": c_int}
    assert "sam_answer_status_fold" not in _capi.SIGNATURES and "sam_answer_status_fold" not in _capi.NO_STATUS
    for name, other in _capi.HEADER_SIGNATURES.items():                  # every other header of the registry
        assert name == "step" or "sam_answer_status_fold" not in other
    assert list(_capi.HEADER_SIGNATURES["answers"]) == ["sam_answer_table_from_text"] and list(_capi.HEADER_SIGNATURES["text"]) == ["sam_phoc_from_text"]
    assert list(_capi.HEADER_SIGNATURES["pipeline"]) == ["sam_mask_bits_from_boxes"] and len(_capi.SIGNATURES) == 77
    l = _capi.lib()
    assert l.sam_abi_version() == 9 and l.sam_build_digest().decode() == b._digest()
    assert l.sam_answer_status_fold.argtypes == _capi.HEADER_SIGNATURES["step"]["sam_answer_status_fold"] and l.sam_answer_status_fold.restype is c_int
    assert os.path.join(b.CSRC, "answer_status.hip") in b.sources()
    assert '#include "sam_hip.h"' in open(b.HEADERS["step"]).read()


def test_digest_covers_the_step_header(tmp_path, monkeypatch):
    import sam_textvqa_amd._build as b
    was = b._digest()
    other = tmp_path / "sam_hip_step.h"
    other.write_text(open(b.HEADERS["step"]).read() + "\n/* changed */\n")
    monkeypatch.setitem(b.HEADERS, "step", str(other))
    assert b._digest() != was


# never dereferenced: every case below is rejected by the argument checks, before any device call
OK = dict(status=1 << 16, B=4, step_dev=1 << 16, step=0, state=1 << 16)
REJECTED = [("null status", dict(status=None), "null"), ("null state", dict(state=None), "null"), ("B = 0", dict(B=0), "batch 0"), ("B < 0", dict(B=-3), "batch -3"),
            ("misaligned status", dict(status=(1 << 16) + 2), "misaligned"), ("misaligned state", dict(state=(1 << 16) + 4), "misaligned"),
            ("misaligned step_dev", dict(step_dev=(1 << 16) + 4), "misaligned")]


@pytest.mark.parametrize("name,change,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_argument_rejections_come_before_any_device_call(name, change, word):
    from sam_textvqa_amd import _capi
    a = dict(OK, **change)
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    args = (p(a["status"]), a["B"], p(a["step_dev"]), a["step"], p(a["state"]), None)
    rc = _capi.lib().sam_answer_status_fold(*args)
    assert rc == _capi.CONSTANTS["SAM_ERR_ARG"] == -1, name
    msg = _capi.lib().sam_last_error().decode()
    assert msg.startswith("sam_answer_status_fold:") and word in msg, msg
    with pytest.raises(_capi.SamHipError, match="sam_answer_status_fold"):
        _capi.call("sam_answer_status_fold", *args)


def test_ops_wrapper_rejects_cpu_tensors():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    with pytest.raises(SamHipError):                                                           # CPU tensors: rejected, no fallback
        ops.answer_status_fold(torch.zeros(4, dtype=torch.int32), torch.tensor(RESET))


# ---------------------------------------------------------------------------------------------- the host twin of the record
def test_fold_status_host_on_hand_written_cases():
    assert A.STATUS_STATE_RESET == (0, 0, -1, -1) and A.STATUS_COUNT_CAP == 1 << 62
    assert A.fold_status_host([0, 0, 0], 5, RESET) == [0, 0, -1, -1]                              # clean: nothing moves, whatever the step
    assert A.fold_status_host([0, 0, 8, 0], 5, RESET) == [8, 1, 5, 2]                             # one flagged
    assert A.fold_status_host([0, 1, 4, 0, 8, 4], 0, RESET) == [13, 4, 0, 1]                      # several bits: OR, count, the LOWEST flagged index
    state = A.fold_status_host([0, 0, 2], 7, RESET)
    assert state == [2, 1, 7, 2]
    state = A.fold_status_host([4, 0, 0], 9, state)                                              # two folds in a row: bits and count grow, the first stays
    assert state == [6, 2, 7, 2]
    assert A.fold_status_host([0, 0, 0], 10, state) == state
    assert A.fold_status_host([1], 3, [0, 0, -1, -1]) == [1, 1, 3, 0]
    # a negative status word enters the OR as its unsigned 32-bit value: the record never goes negative
    assert A.fold_status_host([-1], 0, RESET) == [0xFFFFFFFF, 1, 0, 0]
    # tensors in, a list out; the arguments are left alone
    st, before = torch.tensor([0, 2], dtype=torch.int32), torch.tensor(RESET)
    assert A.fold_status_host(st, 4, before) == [2, 1, 4, 1] and before.tolist() == RESET
    with pytest.raises(ValueError, match="no samples"):
        A.fold_status_host([], 0, RESET)


def test_fold_status_host_saturates_the_count():
    cap = 1 << 62
    assert A.fold_status_host([1, 1, 1], 2, [1, cap - 5, 0, 0]) == [1, cap - 2, 0, 0]
    assert A.fold_status_host([1, 1, 1], 2, [1, cap - 3, 0, 0]) == [1, cap, 0, 0]
    assert A.fold_status_host([1, 1, 1], 2, [1, cap - 2, 0, 0]) == [1, cap, 0, 0]
    assert A.fold_status_host([1, 0, 1], 2, [1, cap, 0, 0]) == [1, cap, 0, 0]
    assert A.fold_status_host([0, 0, 0], 2, [1, cap, 0, 0]) == [1, cap, 0, 0]


# ---------------------------------------------------------------------------------------------- collate_ragged packs the answers
def samples(n=3, answers=True, tokens=True):
    g = torch.Generator().manual_seed(0)
    out = []
    for b in range(n):
        no, nc = 2 + b, 1 + b
        s = dict(obj_features=torch.randn(no, 8, generator=g), obj_bboxes=torch.rand(no, 5, generator=g), ocr_features=torch.randn(nc, 8, generator=g),
                 ocr_fasttext=torch.randn(nc, 6, generator=g), ocr_bboxes=torch.rand(nc, 5, generator=g))
        if tokens:
            s["ocr_tokens"] = ["tok%d" % i for i in range(nc)]
        else:
            s["ocr_phoc"] = torch.rand(nc, 604, generator=g)
        if answers:
            s["answers"] = ["tok0 go"] * (4 + b) + ["Stop \U0001F600"] * (6 - b)
        out.append(s)
    return out


def test_collate_ragged_packs_the_answers_as_pack_answer_text_does():
    ss = samples()
    bd = R.collate_ragged(ss, max_obj_num=6, max_ocr_num=5)
    want = A.pack_answer_text([s["answers"] for s in ss])
    assert set(A.ANSWER_TEXT_KEYS) <= set(bd)
    for k in A.ANSWER_TEXT_KEYS:
        assert bd[k].dtype == torch.int32 and torch.equal(bd[k], want[k]), k
    assert tuple(bd["answer_text"].shape) == (3, 10, A.MAX_ANSWER_CHARS) and A.check_answer_text(bd)
    R.check(bd)


def test_collate_ragged_refuses_a_batch_that_gives_answers_unevenly():
    ss = samples()
    del ss[1]["answers"]
    with pytest.raises(ValueError, match="answers"):
        R.collate_ragged(ss, max_obj_num=6, max_ocr_num=5)
    with pytest.raises(ValueError, match="ocr_tokens"):                                         # answers are matched against the tokens' text
        R.collate_ragged(samples(tokens=False), max_obj_num=6, max_ocr_num=5)
    ss = samples()
    ss[2]["answers"] = ss[2]["answers"][:9]
    with pytest.raises(ValueError, match="sample 2: expected 10 answers, got 9"):
        R.collate_ragged(ss, max_obj_num=6, max_ocr_num=5)


@pytest.mark.parametrize("tokens", [True, False])
def test_samples_without_answers_collate_as_before(tokens):
    with_answers = R.collate_ragged(samples(tokens=True), max_obj_num=6, max_ocr_num=5) if tokens else None
    bd = R.collate_ragged(samples(answers=False, tokens=tokens), max_obj_num=6, max_ocr_num=5)
    assert not set(A.ANSWER_TEXT_KEYS) & set(bd) and not A.check_answer_text(bd)
    want = set(R.RAGGED_KEYS) - ({"ocr_phoc_rows"} if tokens else set()) | ({"ocr_text", "ocr_text_len"} if tokens else set())
    assert set(bd) == want
    if tokens:                                                                                   # the same batch but for the two answer keys
        assert set(with_answers) == want | set(A.ANSWER_TEXT_KEYS)
        n_obj, n_ocr = int(bd["obj_count"].sum()), int(bd["ocr_count"].sum())
        for k in want:
            n = bd[k].shape[0] if "count" in k or "text" in k else (n_obj if k.startswith("obj") else n_ocr)      # (rows past the total are uninitialised)
            assert torch.equal(bd[k][:n], with_answers[k][:n]), k
