"""CPU: answer-space upper bounds (sam_textvqa_amd/coverage.py) -- the host twin of sam_answer_witness against the matcher that is
pinned to the reference (answers.match_answer_to_vocab_ocr_seq) on the golden samples and a synthetic set, the relations between the three sources, all
five tensors of a hand-written sample against literals, a census of the answer classes in the inputs the GPU parity tests use (so that none of them is
covered in name only), the registry line with the derived signature, and every argument check of the entry point, which needs no GPU.

The input builders below are shared with tests/test_coverage_gpu.py; each is computed once."""
import ctypes
import functools
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A
from sam_textvqa_amd import coverage as C
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import phoc as P
from sam_textvqa_amd import wordindex as W
from tests.test_answer_text_cpu import SPECIALS, golden_batch, special_batch


# ---------------------------------------------------------------------------------------------- inputs, shared with tests/test_coverage_gpu.py
def pack(answers, tokens, A_, No, La, Lw):
    bd = A.pack_answer_text(answers, num_answers=A_, max_chars=La)
    bd.update(P.pack_ocr_text(tokens, max_ocr_tokens=No, max_chars=Lw))
    bd["ocr_count"] = M.ocr_counts(tokens, No)
    return bd


HAND_WORDS = SPECIALS + ["bus", "no", "bar", "audi", "stop", "west", "coca", "cola"]          # ids 4 .. 11; </s> = 2
HAND_L = 3
HAND_ANSWERS = [["bus stop",                 # 0: vocabulary only
                 "taxi exit",                # 1: OCR only
                 "bus taxi",                 # 2: reachable only from both
                 "bus zebra",                # 3: unreachable, one word nowhere
                 "",                         # 4: empty
                 " \t  \t ",                 # 5: whitespace only: tabs and doubled blanks
                 "no bar audi west",         # 6: four words at L = 3: truncated
                 "taxi",                     # 7: a word two OCR slots hold: the lowest wins
                 "cola",                     # 8: in the vocabulary and in an OCR slot
                 "bus stop"],                # 9: an exact duplicate of answer 0
                ["zebra"] * 5 + ["", " "] + ["gnu emu"] * 3]          # a sample no source reaches
HAND_TOKENS = [["taxi", "", "cola", "taxi", "exit"], ["", "okapi"]]   # slot 1 of sample 0 has length 0


@functools.lru_cache(None)
def hand_sample():
    """(vocabulary, index, batch on the CPU, L): A = 10, No = 5, V = 12, T = 32, La = 16 (answer 6 fills it), Lw = Lv = 5"""
    voc = A.AnswerVocab(HAND_WORDS)
    return voc, A.vocab_index(voc, max_word=5), pack(HAND_ANSWERS, HAND_TOKENS, 10, 5, 16, 5), HAND_L


@functools.lru_cache(None)
def rich_sample(B):
    """metrics.make_score_text(rich=True) at the 5000-word vocabulary: A = 10, No = 50, L = 12"""
    voc, answers, tokens = M.make_score_text(B, num_vocab=5000, n_ocr=50, seed=7 + B, rich=True)
    return voc, A.vocab_index(voc), pack(answers, tokens, 10, 50, 128, 32), 12


FUZZ_WORDS = SPECIALS + ["a", "b", "c", "go", "stop", "sign", "tok", "x1", "über", "σας", "longword", "wwwwwwww"]
FUZZ_LA, FUZZ_LW = 128, 8
FUZZ_B = 256
FUZZ_SHAPES = [(A_, No, L) for A_ in (1, 3, 10) for No in (1, 50, 64) for L in (1, 3, 12)]
_OOV = ["oov1", "oov2", "oov3", "q", "zz", "\U0001F600", "Stop"]
_JUNK = ["nowhere", "zebra9", "toolongforanyslot", "y" * 40]
_SEPS = [" ", "  ", "\t", " \t ", "　", "\x85", "\n", "\x1c "]


@functools.lru_cache(None)
def fuzz_vocab():
    voc = A.AnswerVocab(FUZZ_WORDS)
    return voc, A.vocab_index(voc, max_word=FUZZ_LW)


def _full_length(rng):
    """an answer of exactly 128 code points: 64 words (the most there can be), one word, blanks only, or five words"""
    kind = rng.randint(4)
    if kind == 0:
        singles = ["a", "b", "c", "q"]
        parts = [singles[rng.randint(4)] + [" ", "\t", "　"][rng.randint(3)] for _ in range(63)]
        return "".join(parts) + ["go", "x1", "zz"][rng.randint(3)]
    if kind == 1:
        return "y" * 128
    if kind == 2:
        return "".join(_SEPS[rng.randint(3)][0] for _ in range(128))
    return "stop sign " + "w" * 8 + " " * 102 + "tok über"


@functools.lru_cache(None)
def fuzz_sample(A_, No, L):
    """FUZZ_B samples for one launch: answers of every class with separators from the whole whitespace set, OCR slots that repeat, are empty or hold
    vocabulary words, answers at exactly La = 128 code points, garbage behind every length and a few lengths outside [0, capacity]"""
    voc, index = fuzz_vocab()
    rng = np.random.RandomState(1000 * A_ + 10 * No + L)
    vocab_words = FUZZ_WORDS[4:]
    all_answers, all_tokens = [], []
    for b in range(FUZZ_B):
        pool = [vocab_words[i] for i in rng.randint(0, len(vocab_words), 3)] + [_OOV[i] for i in rng.randint(0, len(_OOV), 3)]
        tokens = [("" if rng.rand() < 0.2 else pool[rng.randint(len(pool))]) for _ in range(rng.randint(0, No + 1))]
        if b % 16 == 0:
            tokens = []
        solid = [t for t in tokens if t] or vocab_words
        barren = b % 16 == 5                             # a sample no source reaches: words that are nowhere, blanks, nothing
        answers = []
        for _ in range(A_):
            r = rng.rand()
            if barren:
                ans = ["", " \t", "nowhere", "zebra9 nowhere", "y" * 128][rng.randint(5)]
            elif r < 0.07:
                ans = ""
            elif r < 0.14:
                ans = "".join(_SEPS[rng.randint(len(_SEPS))] for _ in range(rng.randint(1, 5)))
            elif r < 0.24 and answers:
                ans = answers[rng.randint(len(answers))]
            elif r < 0.32:
                ans = _full_length(rng)
            else:
                n = int(rng.choice([1, 1, 2, 2, 3, 4, 13, 14]))
                kind = rng.randint(4)                    # vocabulary words, OCR tokens, a mix of the two, a mix with words that are nowhere
                src = [vocab_words, solid, vocab_words + solid, vocab_words + solid + _JUNK][kind]
                ws = [src[rng.randint(len(src))] for _ in range(n)]
                ans = "".join(w + _SEPS[rng.randint(len(_SEPS))] for w in ws)
                ans = (_SEPS[rng.randint(len(_SEPS))] if rng.rand() < 0.3 else "") + (ans if rng.rand() < 0.3 else ans.rstrip())
                ans = ans[:FUZZ_LA]
            answers.append(ans)
        all_answers.append(answers)
        all_tokens.append(tokens)
    bd = pack(all_answers, all_tokens, A_, No, FUZZ_LA, FUZZ_LW)
    at, al, ot, ol = (bd[k].numpy() for k in ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len"))
    junk_a, junk_o = rng.randint(33, 0x2FF, at.shape).astype(np.int32), rng.randint(33, 0x2FF, ot.shape).astype(np.int32)
    np.copyto(at, junk_a, where=np.arange(FUZZ_LA)[None, None, :] >= al[:, :, None])
    np.copyto(ot, junk_o, where=np.arange(FUZZ_LW)[None, None, :] >= ol[:, :, None])
    al[(al == FUZZ_LA) & (rng.rand(*al.shape) < 0.5)] = FUZZ_LA + 9                                 # clamped to La
    al[(al == 0) & (rng.rand(*al.shape) < 0.5)] = -4                                               # clamped to 0
    ol[(ol == 0) & (rng.rand(*ol.shape) < 0.3)] = -1
    ol[(ol == FUZZ_LW) & (rng.rand(*ol.shape) < 0.5)] = FUZZ_LW + 3
    return voc, index, bd, L


@functools.lru_cache(None)
def limit_sample():
    """every capacity at its limit: A = 64, La = 128, No = 64, Lw = Lv = 64, L = 64 (the kernel's largest LDS carve): words of 64 code points in the
    vocabulary and in the last OCR slot, an answer of 64 words whose witness fills all 64 steps, 64 answers over 64 slots"""
    long_v, long_o = "w" * 64, "x" * 64
    voc = A.AnswerVocab(SPECIALS + ["a", "b", "c", long_v])
    rng = np.random.RandomState(64)
    all_answers, all_tokens = [], []
    for b in range(3):
        pool = ["q", "a", "", "zz"] + [long_o] * (b == 1)                # sample 0 holds the 64-code-point token in its last slot alone
        tokens = [pool[rng.randint(len(pool))] for _ in range(63)] + [long_o if b < 2 else "q"]
        words = ["a", "b", "c", "q", "zz", "nowhere"]
        answers = [" ".join(["a", "q"][rng.randint(2)] for _ in range(64)), long_v + " " + long_o[:63], long_o + " " + long_v[:63], long_v, long_o, "a" * 65, ""]
        answers += [" ".join(words[rng.randint(len(words) - (k % 3 == 0))] for _ in range(rng.randint(1, 5))) for k in range(64 - len(answers))]
        all_answers.append(answers)
        all_tokens.append(tokens)
    return voc, A.vocab_index(voc, max_word=64), pack(all_answers, all_tokens, 64, 64, 128, 64), 64


@functools.lru_cache(None)
def twin(kind, *key):
    """witness_host of one of the inputs above, computed once: kind in ("hand", "rich", "fuzz", "limit")"""
    voc, index, bd, L = {"hand": hand_sample, "rich": rich_sample, "fuzz": fuzz_sample, "limit": limit_sample}[kind](*key)
    return C.witness_host(bd, index, L)


def strings(bd):
    """(answers [B][A], tokens [B][No]) of a packed batch, lengths clamped as the kernel clamps them"""
    at, al, ot, ol = (bd[k].numpy() for k in ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len"))
    al, ol = np.clip(al, 0, at.shape[2]), np.clip(ol, 0, ot.shape[2])
    return ([["".join(map(chr, at[b, a, :al[b, a]])) for a in range(at.shape[1])] for b in range(at.shape[0])],
            [["".join(map(chr, ot[b, o, :ol[b, o]])) for o in range(ot.shape[1])] for b in range(ot.shape[0])])


def census(bd, index, wit, L):
    """which answer classes occur in a batch, read off the twin's own output and the batch's strings"""
    answers, tokens = strings(bd)
    vocab = C.vocab_dict(index)
    r = wit["reach"].transpose(1, 2, 0)                                    # [B, A, 3]
    words = wit["words"]
    has = lambda *pattern: bool((r == np.array(pattern)).all(-1).any())
    seen = {"vocab only": has(1, 0, 1), "OCR only": has(0, 1, 1), "only from both": has(0, 0, 1), "from every source": has(1, 1, 1),
            "unreachable": bool(((r == 0).all(-1) & (words > 0)).any()), "truncated": bool(((words > L) & (r[:, :, 2] == 1)).any()),
            "no source reaches the sample": bool((wit["any"].sum(0) == 0).any()), "empty": False, "whitespace only": False, "duplicate": False,
            "two slots hold a word": False, "word in vocabulary and OCR": False, "empty slot below a token": False, "full length": False}
    for ans, tok in zip(answers, tokens):
        seen["empty"] |= "" in ans
        seen["whitespace only"] |= any(a and not a.split() for a in ans)
        seen["duplicate"] |= any(a and ans.count(a) > 1 for a in ans)
        seen["full length"] |= any(len(a) == bd["answer_text"].shape[2] for a in ans)
        used = {w for a in ans for w in a.split()}
        seen["two slots hold a word"] |= any(t and tok.count(t) > 1 and t in used for t in tok)
        seen["word in vocabulary and OCR"] |= any(t in vocab and t in used for t in tok)
        last = max([o for o, t in enumerate(tok) if t], default=-1)
        seen["empty slot below a token"] |= "" in tok[:max(last, 0)]
    return seen


# ---------------------------------------------------------------------------------------------- the twin against the reference-pinned matcher
def _matcher_rows(voc, answers, tokens, No, L):
    """per sample and answer: match_answer_to_vocab_ocr_seq as build_answer_table calls it (every one of the first No tokens an OCR slot), its first
    sequence cut to L and padded with </s>, or None"""
    rows = []
    for ans, tok in zip(answers, tokens):
        ocr2inds = defaultdict(list)
        for i, t in enumerate(list(tok)[:No]):
            ocr2inds[t].append(i)
        got = [A.match_answer_to_vocab_ocr_seq(a, voc.word2idx_dict, ocr2inds) for a in ans]
        rows.append([(list(g[0])[:L] + [voc.EOS_IDX] * max(L - len(g[0]), 0)) if g else None for g in got])
    return rows


@pytest.mark.parametrize("which", ["golden", "synthetic"])
def test_source_2_is_the_first_sequence_of_the_reference_pinned_matcher(which):
    if which == "golden":
        voc, answers, tokens, _ = golden_batch()
    else:
        voc, _, answers, tokens = special_batch()
    L, No = 12, 50
    bd = pack(answers, tokens, 10, No, 128, 32)
    wit = C.witness_host(bd, A.vocab_index(voc), L)
    want = _matcher_rows(voc, answers, tokens, No, L)
    seqs = wit["seqs"].reshape(3, len(answers), 10, L)
    reachable = 0
    for b in range(len(answers)):
        for a in range(10):
            assert wit["reach"][2, b, a] == (want[b][a] is not None), (b, a, answers[b][a])
            if want[b][a] is not None:
                assert seqs[2, b, a].tolist() == want[b][a], (b, a, answers[b][a])
                reachable += 1
            assert wit["words"][b, a] == len(answers[b][a].split())
    assert reachable >= 20 and (wit["reach"][2] == 0).any()               # both kinds occur
    assert {k: (v.dtype, v.shape) for k, v in wit.items()} == {k: (C.WITNESS.np_dtypes[k], s) for k, s in C.WITNESS.shapes(B=len(answers), A=10, L=L).items()}


# ---------------------------------------------------------------------------------------------- relations between the sources
@pytest.mark.parametrize("kind, key", [("hand", ()), ("rich", (5,)), ("fuzz", (10, 50, 3))])
def test_both_reaches_whatever_one_source_reaches_and_counts_add_up(kind, key):
    wit = twin(kind, *key)
    r = wit["reach"]
    assert (r[2] >= np.maximum(r[0], r[1])).all() and set(np.unique(r).tolist()) <= {0, 1}
    assert (wit["any"] == r.max(2)).all()
    c = wit["counts"]
    assert (c[:, 0] == wit["words"].sum(1)).all() and (c[:, 1:] <= c[:, :1]).all() and (c[:, 1] + c[:, 2] + c[:, 3] >= c[:, 0]).all()
    assert ((wit["words"] == 0) <= (r.sum(0) == 0)).all()                 # an answer without a word is reachable from nowhere


@pytest.mark.parametrize("kind, key, Lw", [("hand", (), 5), ("rich", (5,), 32)])
def test_the_bound_from_both_is_no_lower_than_from_one_source(kind, key, Lw):
    voc, index, bd, L = {"hand": hand_sample, "rich": rich_sample}[kind](*key)
    ub = C.upper_bounds_host(bd, index, M.vocab_text(voc, max_word=Lw), caps=(10, Lw, 128), L=L, counts=bd["ocr_count"])
    assert ub.shape == (3, bd["answer_text"].shape[0], 3) and ub.dtype == np.float32
    assert (ub[2] >= ub[0]).all() and (ub[2] >= ub[1]).all() and (ub >= 0).all() and (ub <= 1).all()
    wit = twin(kind, *key)
    assert not ub[wit["any"] == 0].any()                                   # no reachable answer: 0 by definition
    assert (ub[2][:, 0] > 0).any()


def test_the_bounds_of_the_hand_written_sample():
    """sample 0: every source reaches "bus stop" (twice among the ten answers) or "taxi exit" / "cola" (once each); sample 1: nothing"""
    voc, index, bd, L = hand_sample()
    ub = C.upper_bounds_host(bd, index, M.vocab_text(voc, max_word=5), caps=(10, 5, 128), L=L, counts=bd["ocr_count"])
    sc = M.soft_scores_normalized(HAND_ANSWERS[0])
    assert ub[0, 0].tolist() == [np.float32(sc["bus stop"]), 1.0, 1.0]     # vocabulary: "bus stop", "cola", and the cut "no bar audi" (worth nothing)
    assert ub[1, 0].tolist() == [np.float32(max(sc["taxi exit"], sc["taxi"], sc["cola"])), 1.0, 1.0]
    assert ub[2, 0].tolist() == ub[0, 0].tolist() and sc["bus stop"] > sc["cola"]
    assert not ub[:, 1].any()


# ---------------------------------------------------------------------------------------------- the hand-written sample, all five tensors
def test_the_hand_written_sample_against_literals():
    voc, index, bd, L = hand_sample()
    assert (index["V"], index["EOS"], index["slots"].numel(), L) == (12, 2, 32, 3) and tuple(bd["answer_text"].shape) == (2, 10, 16)
    # the probes chain and wrap: "<unk>" and "bus" share home slot 31, "no" and "bar" home slot 0, "audi" lives at 1: "bus" is found at 3 after 31, 0, 1, 2
    slots = index["slots"].tolist()
    home = lambda w: W.text_hash([ord(c) for c in w]) & 31
    assert (home("<unk>"), home("bus"), home("no"), home("bar"), home("audi")) == (31, 31, 0, 0, 1)
    assert (slots[31], slots[0], slots[1], slots[2], slots[3]) == (3, 5, 7, 6, 4) and W.lookup_host(index, [ord(c) for c in "bus"]) == 4
    wit = C.witness_host(bd, index, L)
    E = 2                                                                   # </s>
    assert wit["words"].tolist() == [[2, 2, 2, 2, 0, 0, 4, 1, 1, 2], [1, 1, 1, 1, 1, 0, 0, 2, 2, 2]]
    assert wit["reach"].tolist() == [[[1, 0, 0, 0, 0, 0, 1, 0, 1, 1], [0] * 10],
                                     [[0, 1, 0, 0, 0, 0, 0, 1, 1, 0], [0] * 10],
                                     [[1, 1, 1, 0, 0, 0, 1, 1, 1, 1], [0] * 10]]
    assert wit["any"].tolist() == [[1, 0], [1, 0], [1, 0]]
    bus_stop, taxi_exit, nothing = [4, 8, E], [12, 16, E], [[E, E, E]] * 10
    want = [[[bus_stop] * 6 + [[5, 6, 7], bus_stop, [11, E, E], bus_stop], nothing],                              # vocabulary: "no bar audi west" is cut
            [[taxi_exit] * 7 + [[12, E, E], [14, E, E], taxi_exit], nothing],                                      # OCR: "taxi" is slot 0, not 3; "cola" slot 2
            [[bus_stop, taxi_exit, [4, 12, E], bus_stop, bus_stop, bus_stop, [5, 6, 7], [12, E, E], [11, E, E], bus_stop], nothing]]      # both: "cola" is 11
    assert wit["seqs"].reshape(3, 2, 10, 3).tolist() == want
    assert wit["counts"].tolist() == [[16, 11, 5, 1], [11, 0, 0, 11]]
    assert wit["seqs"].dtype == np.int64 and all(wit[k].dtype == np.int32 for k in ("words", "reach", "any", "counts"))


def test_lengths_are_clamped_and_text_behind_them_is_not_read():
    voc, index, bd, L = hand_sample()
    want = C.witness_host(bd, index, L)
    other = {k: v.clone() for k, v in bd.items()}
    at, al, ot, ol = (other[k].numpy() for k in ("answer_text", "answer_text_len", "ocr_text", "ocr_text_len"))
    at[np.arange(16)[None, None, :] >= al[:, :, None]] = ord("x")
    ot[np.arange(5)[None, None, :] >= ol[:, :, None]] = ord("x")
    al[0, 4], al[0, 6], ol[0, 1], ol[1, 1] = -7, 16 + 100, -1, 5 + 4        # "" and the 16-code-point answer; the empty slot and the 5-code-point "okapi"
    got = C.witness_host(other, index, L)
    assert all(got[k].tobytes() == want[k].tobytes() for k in C.KEYS)
    with pytest.raises(ValueError, match="over the limits"):
        C.witness_host(bd, index, 65)
    with pytest.raises(ValueError, match="at least 1"):
        C.witness_host(bd, index, 0)


# ---------------------------------------------------------------------------------------------- non-vacuity of the GPU parity inputs
ALL_CLASSES = ("vocab only", "OCR only", "only from both", "from every source", "unreachable", "truncated", "no source reaches the sample", "empty",
               "whitespace only", "duplicate", "two slots hold a word", "word in vocabulary and OCR", "empty slot below a token")


def test_every_answer_class_occurs_in_the_inputs_of_the_gpu_parity_tests():
    voc, index, bd, L = hand_sample()
    seen = census(bd, index, twin("hand"), L)
    assert all(seen[k] for k in ALL_CLASSES), seen
    # the fuzz: every class in the launches whose shapes admit it, and answers of exactly 128 code points in every launch
    for A_, No, L in FUZZ_SHAPES:
        voc, index, bd, _ = fuzz_sample(A_, No, L)
        seen = census(bd, index, twin("fuzz", A_, No, L), L)
        need = set(ALL_CLASSES) | {"full length"}
        if A_ == 1:
            need -= {"duplicate"}
        if No == 1:
            need -= {"two slots hold a word", "empty slot below a token"}
        assert all(seen[k] for k in need), ((A_, No, L), {k: seen[k] for k in need if not seen[k]})
        al = bd["answer_text_len"].numpy()
        assert (al > FUZZ_LA).any() and (al < 0).any() and (bd["ocr_text_len"].numpy() < 0).any()
    # the limits: a witness of 64 steps, words of 64 code points matched in the vocabulary and in slot 63
    voc, index, bd, L = limit_sample()
    wit = twin("limit")
    seqs = wit["seqs"].reshape(3, 3, 64, 64)
    assert tuple(bd["answer_text"].shape) == (3, 64, 128) and tuple(bd["ocr_text"].shape) == (3, 64, 64) and index["cp"].shape[1] == 64 and L == 64
    assert (wit["words"][:, 0] == 64).all() and (wit["reach"][2, :, 0] == 1).all() and (seqs[2, :, 0] != index["EOS"]).all()
    assert wit["reach"][:, 0, 3].tolist() == [1, 0, 1] and wit["reach"][:, 0, 4].tolist() == [0, 1, 1] and seqs[1, 0, 4, 0] == index["V"] + 63
    assert not wit["reach"][:, :, 1:3].any() and not wit["reach"][:, :, 5].any()          # 63 of the 64 code points, and a word of 65, match nothing
    # the rich batches: what make_score_text draws
    for B in (1, 5):
        voc, index, bd, L = rich_sample(B)
        seen = census(bd, index, twin("rich", B), L)
        assert seen["duplicate"] and (seen["vocab only"] or seen["OCR only"] or seen["from every source"]), (B, seen)
        assert B == 1 or (seen["unreachable"] and seen["OCR only"] and seen["word in vocabulary and OCR"] and seen["two slots hold a word"]), (B, seen)
    assert index["slots"].numel() == 16384 and len(voc) == 5000


# ---------------------------------------------------------------------------------------------- registry and C ABI
def test_the_header_is_registered_ahead_of_evalboard_and_parses_into_the_written_signature():
    from sam_textvqa_amd import _build, _capi, layouts, ops
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "coverage" in _build.ABI_ADDITIONS and _build.ABI_ADDITIONS["coverage"] in _build.public_headers()
    assert os.path.basename(_build.ABI_ADDITIONS["coverage"]) == "sam_hip_coverage.h"
    keys = list(_build.ABI_ADDITIONS)
    assert keys[-1] == "evalboard" and keys.index("coverage") == len(keys) - 2
    assert _capi.ADDITION_SIGNATURES["coverage"] == {"sam_answer_witness": [vp, i64, vp, vp, i64, vp, vp, i64, vp, vp] + [i] * 10 + [vp] * 5 + [vp]}
    assert _capi.ADDITION_RESTYPES["coverage"] == {"sam_answer_witness": i}
    for name, path in list(_build.HEADERS.items()) + list(_build.ABI_PARTS.items()) + list(_build.ABI_EXTENSIONS.items()) + list(_build.ABI_ADDITIONS.items()):
        assert name == "coverage" or "sam_answer_witness" not in open(path).read(), name
    assert os.path.join(_build.CSRC, "coverage.hip") in _build.sources()
    lib = _capi.lib()                                           # builds coverage.hip for gfx950 with the rest when the tree changed
    assert lib.sam_build_digest().decode() == _build._digest()
    assert lib.sam_answer_witness.argtypes == _capi.ADDITION_SIGNATURES["coverage"]["sam_answer_witness"] and lib.sam_answer_witness.restype is i
    assert ops.WITNESS_KEYS == C.KEYS == layouts.WITNESS.keys == ("words", "reach", "any", "seqs", "counts")
    # the layout is the header's run of output pointers, and allocates what the header says
    from tests.test_layouts_cpu import run_of
    assert run_of("sam_answer_witness", "words", 5) == list(layouts.WITNESS.fields)
    assert list(layouts.WITNESS.shapes(B=2, A=3, L=4).items()) == [("words", (2, 3)), ("reach", (3, 2, 3)), ("any", (3, 2)), ("seqs", (3, 6, 4)), ("counts", (2, 4))]


FAKE, STEP = 1 << 20, 1 << 16                                   # never dereferenced: the checks reject the call before any launch
POINTERS = ("answer_text", "answer_len", "ocr_text", "ocr_len", "vocab_cp", "vocab_len", "slots", "words", "reach", "any", "seqs", "counts")


def _call(**kw):
    from sam_textvqa_amd import _capi
    p = {k: FAKE + j * STEP for j, k in enumerate(POINTERS)}
    p.update(dict(B=2, A=10, La=128, No=50, Lw=32, V=12, Lv=32, T=32, eos=2, L=12, ld_answer=128, ld_ocr=32, ld_vocab=32))
    p.update(kw)
    return _capi.call("sam_answer_witness", p["answer_text"], p["ld_answer"], p["answer_len"], p["ocr_text"], p["ld_ocr"], p["ocr_len"], p["vocab_cp"], p["ld_vocab"],
                      p["vocab_len"], p["slots"], p["B"], p["A"], p["La"], p["No"], p["Lw"], p["V"], p["Lv"], p["T"], p["eos"], p["L"],
                      *[p[k] for k in POINTERS[7:]], None)


def test_the_entry_point_rejects_bad_arguments_without_a_gpu():
    from sam_textvqa_amd._capi import SamHipError
    for k in POINTERS:
        with pytest.raises(SamHipError, match="null") as e:
            _call(**{k: None})
        assert "rc=-1" in str(e.value)                          # SAM_ERR_ARG
        with pytest.raises(SamHipError, match="misaligned") as e:
            _call(**{k: FAKE + 2})
        assert "rc=-1" in str(e.value)
    with pytest.raises(SamHipError, match="misaligned"):
        _call(seqs=FAKE + 4)                                    # int64 rows: 8-byte alignment
    for k in ("B", "A", "No", "La", "Lw", "Lv", "L"):
        for v in (0, -1):
            with pytest.raises(SamHipError, match="bad shape") as e:
                _call(**{k: v})
            assert "rc=-1" in str(e.value)
    # each limit: the last supported value gets past the limit check (and fails a later one, so nothing is launched), the next is unsupported
    for k, top in (("La", 128), ("Lw", 64), ("Lv", 64), ("No", 64), ("L", 64), ("A", 64)):
        wide = {"La": dict(ld_answer=1 << 10), "Lw": dict(ld_ocr=1 << 10), "Lv": dict(ld_vocab=1 << 10)}.get(k, {})
        with pytest.raises(SamHipError, match="eos=-1 outside") as e:
            _call(**dict(wide, eos=-1, **{k: top}))
        assert "rc=-1" in str(e.value)
        for v in (top + 1, 1 << 20):
            with pytest.raises(SamHipError, match="at most 128 code points per answer, 64 per word, 64 OCR slots") as e:
                _call(**dict(wide, **{k: v}))
            assert "rc=-2" in str(e.value)                      # SAM_ERR_UNSUPPORTED
    for kw, words in ((dict(ld_answer=127), "ld_answer >= La"), (dict(ld_ocr=31), "ld_ocr >= Lw"), (dict(ld_vocab=31), "ld_vocab >= Lv"),
                      (dict(T=48), "power of two"), (dict(T=16), ">= 2 V"), (dict(T=1), "power of two"), (dict(V=0), "V=0"), (dict(eos=12), "eos=12 outside"),
                      (dict(eos=-1), "eos=-1 outside")):
        with pytest.raises(SamHipError, match=words) as e:
            _call(**kw)
        assert "rc=-1" in str(e.value)


def test_the_python_surface_refuses_cpu_tensors_and_wrong_shapes():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd._capi import SamHipError
    voc, index, bd, L = hand_sample()
    with pytest.raises(SamHipError, match="GPU"):               # no CPU path: the twin is the definition, not a fallback
        C.witness(bd, index, L)
    with pytest.raises(SamHipError, match="must be a tensor"):
        ops.answer_witness(bd["answer_text"].numpy(), bd["answer_text_len"], bd["ocr_text"], bd["ocr_text_len"], index, L)
    with pytest.raises(ValueError, match="three evalboard.Board"):
        C.measure([bd], index, M.vocab_text(voc, max_word=5), boards=[1, 2])
    with pytest.raises(ValueError, match="no batches"):
        C.measure([], index, M.vocab_text(voc, max_word=5))
    with pytest.raises(ValueError, match="distinct words"):
        C.vocab_dict(dict(index, V=13))
