"""GPU: the sticky status record of the answer-table build (csrc/answer_status.hip, sam_answer_status_fold, include/sam_hip_step.h)
-- the one-wave fold kernel against its host twin answers.fold_status_host, bit for bit, with nothing written beside its four words."""
import pytest
import torch

from sam_textvqa_amd import answers as A

pytestmark = pytest.mark.gpu


def fold(status, state, step=0, step_dev=None):
    from sam_textvqa_amd import ops
    return ops.answer_status_fold(torch.tensor(status, dtype=torch.int32, device="cuda"), state, step=step, step_dev=step_dev)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_the_fold_kernel_equals_the_host_twin_and_writes_nothing_beside_its_four_words(B):
    """one wave striding over B = 1, 63, 64, 65 (either side of the wave) and 257 (five trips, the last of one lane).  The four words sit between guard
    elements that must stay as they were"""
    guard, mark = 8, -0x0123456789ABCDEF
    arena = torch.full((guard + 4 + guard,), mark, dtype=torch.int64, device="cuda")
    state = arena[guard:guard + 4]

    def reset():
        state.copy_(torch.tensor(A.STATUS_STATE_RESET, device="cuda"))
        return list(A.STATUS_STATE_RESET)

    def check(want, what):
        assert state.tolist() == want, (B, what, state.tolist(), want)
        assert arena[:guard].eq(mark).all() and arena[guard + 4:].eq(mark).all(), (B, what)

    clean, last = [0] * B, [0] * (B - 1) + [A.STATUS_UNK_TARGET]
    several = [0] * B
    for b, bit in ((B - 1, A.STATUS_GROUPS), (B // 2, A.STATUS_PAD_SLOT), (B // 3, A.STATUS_EXTRA), (min(B - 1, 64), A.STATUS_UNK_TARGET)):
        several[b] |= bit                                     # (B = 1: all four bits in the one sample)
    want = reset()
    fold(clean, state, step=3)
    check(A.fold_status_host(clean, 3, want), "all clean")
    assert state.tolist() == [0, 0, -1, -1]
    fold(last, state, step=5)
    want = A.fold_status_host(last, 5, want)
    check(want, "only the last index flagged")
    assert want == [8, 1, 5, B - 1]
    fold(several, state, step=6)                               # a second launch accumulates: bits and count grow, the first flagged sample stays
    want = A.fold_status_host(several, 6, want)
    check(want, "two launches accumulating")
    assert want[0] == 15 and want[2:] == [5, B - 1]
    want = reset()
    fold(several, state, step=2)
    want = A.fold_status_host(several, 2, want)
    check(want, "several samples with different bits")
    assert want[1] == len([s for s in several if s]) and want[3] == min(b for b, s in enumerate(several) if s)
    want = reset()
    fold(last, state, step=-1, step_dev=torch.tensor([41], dtype=torch.int64, device="cuda"))        # the step from device memory plus a bias
    want = A.fold_status_host(last, 40, want)
    check(want, "step_dev with a bias")
    assert want[2] == 40
    state.copy_(torch.tensor([1, A.STATUS_COUNT_CAP - 1, 0, 0], device="cuda"))                        # the count saturates
    fold([1] * B, state, step=9)
    check(A.fold_status_host([1] * B, 9, [1, A.STATUS_COUNT_CAP - 1, 0, 0]), "saturation")
    assert state[1].item() == A.STATUS_COUNT_CAP


def test_the_fold_follows_a_build_on_the_same_stream():
    """the launch the record was made for: sam_answer_table_from_text, then the fold of its status, no synchronisation in between -- a sample with <unk>
    among its scored words (status bit 8) between clean neighbours"""
    from sam_textvqa_amd import ops, phoc as P
    voc = A.AnswerVocab([A.PAD_TOKEN, A.BOS_TOKEN, A.EOS_TOKEN, A.UNK_TOKEN, "go", "tok"])
    answers = [["go tok"] * 10, ["go"] * 10, ["go <unk>"] * 10, ["tok"] * 10]
    bd = dict(A.pack_answer_text(answers), **P.pack_ocr_text([["tok"], ["go"], ["go"], []], max_ocr_tokens=50))
    bd = {k: v.cuda() for k, v in bd.items()}
    index = A.index_to(A.vocab_index(voc), "cuda")
    out = A.table_outputs(4, A.DEFAULT_CAPS, "cuda")
    state = torch.tensor(A.STATUS_STATE_RESET, dtype=torch.int64, device="cuda")
    want = list(A.STATUS_STATE_RESET)
    for step in (11, 12):
        _, status = A.tables_from_text(bd, index, out=out, check=False)
        ops.answer_status_fold(status, state, step=step)
        want = A.fold_status_host(A.tables_from_text_host(*[bd[k] for k in A.ANSWER_TEXT_KEYS + ("ocr_text", "ocr_text_len")], voc)[1], step, want)
    assert state.tolist() == want == [A.STATUS_UNK_TARGET, 2, 11, 2]
    assert A.status_message([0] * want[3] + [want[0]], index, A.DEFAULT_CAPS).startswith("sample 2: <unk> (index 3)")
