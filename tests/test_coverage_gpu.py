"""GPU: answer-space upper bounds (csrc/coverage.hip, sam_textvqa_amd/coverage.py) on the MI355X -- sam_answer_witness against
its host twin (which tests/test_coverage_cpu.py judges) bit for bit in all five tensors, into outputs filled with a sentinel beforehand so that an
unwritten element shows; upper_bounds against upper_bounds_host; measure with valid flags and with three results boards; and the witnesses decoded by
the evaluator's own kernel back into the answers they stand for.  No test captures a graph."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import coverage as C
from sam_textvqa_amd import evalboard as E
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import sampler as S
from sam_textvqa_amd.wordindex import index_to
from tests.test_coverage_cpu import FUZZ_SHAPES, fuzz_sample, hand_sample, limit_sample, rich_sample, strings, twin

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def to_dev(bd):
    return {k: v.cuda() for k, v in bd.items()}


def poisoned(B, A, L):
    out = C.WITNESS.empty("cuda", B=B, A=A, L=L)
    for k, t in out.items():
        t.fill_(SENTINEL if t.dtype == torch.int32 else (SENTINEL << 32) | SENTINEL)
    return out


def same(got, want):
    """the first of the five tensors that differs from the twin's, with where; None when all are equal bit for bit"""
    for k in C.KEYS:
        g, w = got[k].cpu().numpy(), want[k]
        if g.dtype != w.dtype or g.shape != w.shape or (g != w).any():
            return k, (g.dtype, g.shape, w.shape) if g.shape != w.shape else np.argwhere(g != w)[:4].tolist()
    return None


def launch_and_compare(sample, want):
    voc, index, bd, L = sample
    B, A, _ = bd["answer_text"].shape
    out = poisoned(B, A, L)
    ptrs = {k: t.data_ptr() for k, t in out.items()}
    got = C.witness(to_dev(bd), index_to(index, "cuda"), L, out=out)
    assert {k: t.data_ptr() for k, t in got.items()} == ptrs
    assert same(got, want) is None, same(got, want)
    return got


def test_the_hand_written_sample_equals_the_twin_in_all_five_tensors():
    got = launch_and_compare(hand_sample(), twin("hand"))
    assert got["seqs"].reshape(3, 2, 10, 3)[2, 0, 2].tolist() == [4, 12, 2] and got["counts"].tolist() == [[16, 11, 5, 1], [11, 0, 0, 11]]
    fresh = C.witness(to_dev(hand_sample()[2]), index_to(hand_sample()[1], "cuda"), 3)              # buffers allocated by the call
    assert same(fresh, twin("hand")) is None


@pytest.mark.parametrize("B", [1, 5])
def test_rich_batches_at_the_5000_word_vocabulary_equal_the_twin(B):
    launch_and_compare(rich_sample(B), twin("rich", B))


def test_every_capacity_at_its_limit_equals_the_twin():
    """A = 64, La = 128, No = 64, Lw = Lv = 64, L = 64: the largest LDS carve the entry point accepts"""
    got = launch_and_compare(limit_sample(), twin("limit"))
    assert tuple(got["seqs"].shape) == (3, 3 * 64, 64) and got["any"].min().item() == 1


@pytest.mark.parametrize("A_, No, L", FUZZ_SHAPES)
def test_a_fuzz_of_256_samples_in_one_launch_equals_the_twin(A_, No, L):
    got = launch_and_compare(fuzz_sample(A_, No, L), twin("fuzz", A_, No, L))
    assert tuple(got["seqs"].shape) == (3, 256 * A_, L)


# ---------------------------------------------------------------------------------------------- bounds
def bounds_inputs(kind, *key):
    voc, index, bd, L = {"hand": hand_sample, "rich": rich_sample}[kind](*key)
    Lw = bd["ocr_text"].shape[2]
    return voc, index, bd, L, M.vocab_text(voc, max_word=Lw), (10, Lw, 128)


@pytest.mark.parametrize("kind, key", [("hand", ()), ("rich", (5,))])
def test_upper_bounds_equal_the_host_twin_exactly(kind, key):
    voc, index, bd, L, vt, caps = bounds_inputs(kind, *key)
    want = C.upper_bounds_host(bd, index, vt, caps=caps, L=L)
    got = C.upper_bounds(to_dev(bd), index_to(index, "cuda"), vt, caps=caps, L=L)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (3, bd["answer_text"].shape[0], 3)
    assert got.cpu().numpy().tobytes() == want.tobytes(), (got.cpu().numpy(), want)
    # a shipped table gives the same
    table, _ = M.score_tables_from_text_host(bd, caps)
    again = C.upper_bounds(to_dev(bd), index_to(index, "cuda"), vt, caps=caps, L=L, table=table)
    assert torch.equal(again, got)


def host_report(ub, wit, keep):
    """measure's dict from the twins: sums over the kept slots (float32 multiples of 2^-25 in [0.25, 1] or 0, a few hundred of them: the float64 sums
    are exact, so the order they are added in does not matter)"""
    keep = np.asarray(keep, bool)
    return C._report([[float(ub[s, keep, m].astype(np.float64).sum()) for m in range(3)] for s in range(3)],
                     [int(wit["any"][s, keep].sum()) for s in range(3)], wit["counts"][keep].sum(0).tolist(), int(keep.sum()))


def take(bd, idx):
    sel = torch.as_tensor(idx, dtype=torch.long)
    return {k: v[sel].cuda() for k, v in bd.items()}


def test_measure_without_boards_leaves_out_the_slots_that_are_not_valid():
    voc, index, bd, L, vt, caps = bounds_inputs("rich", 5)
    ub, wit = C.upper_bounds_host(bd, index, vt, caps=caps, L=L), twin("rich", 5)
    first, second = take(bd, [0, 1]), take(bd, [2, 3, 4])
    first["valid"] = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    second["valid"] = torch.tensor([-3, 1, 0], dtype=torch.int32, device="cuda")                    # any non-zero value is valid
    got = C.measure([first, second], index_to(index, "cuda"), vt, caps=caps, L=L)
    assert got == host_report(ub, wit, [1, 0, 1, 1, 0]) and got["count"] == 3
    everything = C.measure([take(bd, [0, 1, 2, 3, 4])], index_to(index, "cuda"), vt, caps=caps, L=L)
    assert everything == host_report(ub, wit, [1] * 5) and everything["words"]["words"] == int(wit["words"].sum())
    assert set(everything["sources"]) == set(C.SOURCES) and everything["sources"]["both"]["reachable"] >= everything["sources"]["ocr"]["reachable"]


def test_measure_with_boards_counts_every_question_once():
    """n = 10 questions in batches of 4 drawn by Sampler(shuffle=False): three batches, the last with two wrapped slots -- marked not valid, and in a
    second pass passed as valid, so that the boards themselves have to drop the repeats"""
    n, B = 10, 4
    voc, index, bd, L, vt, caps = bounds_inputs("rich", n)
    dev_index = index_to(index, "cuda")
    want = C.measure([take(bd, list(range(n)))], dev_index, vt, caps=caps, L=L)
    P = L * (caps[1] + 1)
    for use_valid in (True, False):
        smp = S.Sampler(n, B, shuffle=False)
        drawn = []

        def feed():
            for _ in range(smp.steps_per_epoch):
                idx, valid = smp.next()
                batch = take(bd, idx.cpu().tolist())
                batch["sample_idx"] = idx
                if use_valid:
                    batch["valid"] = valid
                drawn.append((idx.cpu().tolist(), valid.cpu().tolist()))
                yield batch

        boards = [E.Board(n, P) for _ in C.SOURCES]
        got = C.measure(feed(), dev_index, vt, boards=boards, caps=caps, L=L)
        assert drawn == [([0, 1, 2, 3], [1, 1, 1, 1]), ([4, 5, 6, 7], [1, 1, 1, 1]), ([8, 9, 0, 1], [1, 1, 0, 0])]
        assert (got.pop("missing"), got.pop("repeats")) == (0, 0 if use_valid else 2)
        assert got == want and got["count"] == n
        assert all(bd_.t["seen"].min().item() == 1 for bd_ in boards)
    with pytest.raises(ValueError, match="needs sample_idx"):
        C.measure([take(bd, [0, 1])], dev_index, vt, boards=[E.Board(n, P) for _ in C.SOURCES], caps=caps, L=L)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind, key", [("hand", ()), ("rich", (5,))])
def test_the_witnesses_decode_to_the_answers_they_stand_for(kind, key):
    """for every sample whose best answer (the largest soft score) is reachable from both sources within L words, sam_eval_beams gives the beam of that
    answer exactly its soft VQA score and ST-VQA accuracy 1; and the chosen beam (beam 0: all cumulative scores are equal) decodes to answer 0"""
    voc, index, bd, L, vt, caps = bounds_inputs(kind, *key)
    wit = twin(kind, *key)
    dev = to_dev(bd)
    got = C.witness(dev, index_to(index, "cuda"), L)
    table, _ = M.score_tables_from_text(dev, caps=caps, check=False)
    B, A = wit["words"].shape
    res = M.evaluate_beams(got["seqs"][2], torch.zeros(B * A, device="cuda"), table, vt, beam=A, skip=0)
    beam_scores, answers = res["beam_scores"].cpu().numpy(), strings(bd)[0]
    text = M.answer_strings(res["answer"], res["answer_len"])
    checked = 0
    for b in range(B):
        sc = M.soft_scores_normalized(answers[b])
        a = max(range(A), key=lambda j: np.float32(sc[M.normalize_answer(answers[b][j])]))          # (as the score table holds them; the first of equals)
        if wit["reach"][2, b, a] and wit["words"][b, a] <= L:
            assert beam_scores[b * A + a, 0] == np.float32(sc[M.normalize_answer(answers[b][a])]) > 0 and beam_scores[b * A + a, 1] == 1.0, (b, a, answers[b][a])
            assert res["oracle"][b, 0].item() == beam_scores[b * A + a, 0]
            checked += 1
        if wit["reach"][2, b, 0] and wit["words"][b, 0] <= L:
            assert text[b] == " ".join(answers[b][0].split()) and res["best"][b].item() == 0, (b, text[b], answers[b][0])
    assert checked >= (1 if kind == "hand" else 3)
