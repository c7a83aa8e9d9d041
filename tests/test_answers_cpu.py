"""CPU: the answer-table half of M4CAnswerProcessor (sam_textvqa_amd.answers) against the reference golden (tests/golden/make_golden_answers.py):
build_answer_table + collate_answer_tables + the torch twin of the GPU sampler reproduce every (case, forced draw) of the reference exactly; capacities
and the reference's own assertions raise; the host twin of the draw is deterministic, uniform and folds in the rank."""
import json
import os

import numpy as np
import pytest
import torch

from sam_textvqa_amd import answers as A

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    with open(os.path.join(HERE, "golden", "answers.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(HERE, "golden", "answers.npz")))


def case_tables(meta, caps=A.DEFAULT_CAPS):
    voc = A.AnswerVocab(meta["vocab"])
    tabs = [A.build_answer_table(c["answers"], c["context_tokens"], voc, max_ocr_tokens=meta["max_ocr_tokens"], max_copy_steps=meta["max_copy_steps"])
            for c in meta["cases"]]
    return voc, tabs, A.collate_answer_tables(tabs, caps)


def dense_record(g, r, L, W):
    t = np.zeros(L * W, np.float32)
    lo, hi = g["nz_off"][r], g["nz_off"][r + 1]
    t[g["nz_idx"][lo:hi]] = g["nz_val"][lo:hi]
    return t.reshape(L, W)


def records_by_round(g):
    """the golden records grouped into rounds: round j forces draw j on every case that has a j-th candidate (-1 elsewhere)"""
    n_case = len(g["n_cand"])
    rounds = max(1, int(g["n_cand"].max()))
    out = []
    for j in range(rounds):
        choice = np.full(n_case, -1, np.int64)
        recs = {}
        for r, (c, k) in enumerate(zip(g["rec_case"], g["rec_k"])):
            if k == j or (k == -1 and j == 0):
                choice[c] = k
                recs[int(c)] = r
        out.append((choice, recs))
    return out


def test_table_and_twin_reproduce_every_golden_draw():
    meta, g = golden()
    _, tabs, table = case_tables(meta)
    W, L = meta["W"], meta["max_copy_steps"]
    assert int(table["dims"][0]) == W
    np.testing.assert_array_equal(table["meta"][:, 0].numpy(), g["n_cand"])
    seen = 0
    for choice, recs in records_by_round(g):
        out = A.sample_answers_torch(table, torch.from_numpy(choice))
        for c, r in recs.items():
            np.testing.assert_array_equal(out["targets"][c].numpy(), dense_record(g, r, L, W), err_msg="case %s k %d" % (meta["cases"][c]["name"], choice[c]))
            np.testing.assert_array_equal(out["train_prev_inds"][c].numpy(), g["prev"][r])
            np.testing.assert_array_equal(out["train_loss_mask"][c].numpy(), g["loss_mask"][r])
            np.testing.assert_array_equal(out["train_acc_mask"][c].numpy(), g["acc_mask"][r])
            assert int(out["answer_choice"][c]) == choice[c]
            seen += 1
    assert seen == len(g["rec_case"])


def test_soft_scores_and_step0_values():
    meta, g = golden()
    voc = A.AnswerVocab(meta["vocab"])
    c = meta["cases"][0]
    s = A.soft_scores(c["answers"])
    assert [round(s[w], 6) for w in ("red", "apple", "flag", "stop")] == [1.0, 0.9, 0.6, 0.3]
    t = A.build_answer_table(c["answers"], c["context_tokens"], voc)
    vals = dict(zip(t["step0_idx"].tolist(), t["step0_val"].tolist()))
    assert vals[voc.word2idx("red")] == np.float32(s["red"])
    assert vals[len(voc) + 0] == np.float32(s["red"])                      # OCR "red" at slot 0
    assert vals[voc.word2idx("stop")] == np.float32(s["stop"])


def test_duplicate_sequences_keep_their_multiplicity():
    meta, _ = golden()
    voc = A.AnswerVocab(meta["vocab"])
    t = A.build_answer_table(["cola"] * 10, [], voc)
    assert len(t["seq_len"]) == 10 and len(t["step0_idx"]) == 1


def test_group_overflow_raises_naming_sample_and_capacity():
    meta, _ = golden()
    voc = A.AnswerVocab(meta["vocab"])
    tabs = [A.build_answer_table(c["answers"], c["context_tokens"], voc) for c in meta["cases"]]
    big = max(range(len(tabs)), key=lambda i: len(tabs[i]["grp_idx"]))
    n_g = len(tabs[big]["grp_idx"])
    with pytest.raises(ValueError, match=r"sample %d: %d score-index groups exceed the capacity G = %d" % (big, n_g, n_g - 1)):
        A.collate_answer_tables(tabs, A.AnswerTableCaps(200, 12, n_g - 1, 256))
    big = max(range(len(tabs)), key=lambda i: len(tabs[i]["grp_extra"]))
    n_e = len(tabs[big]["grp_extra"])
    with pytest.raises(ValueError, match=r"sample %d: %d target indices exceed the capacity E = %d" % (big, n_e, n_e - 1)):
        A.collate_answer_tables(tabs, A.AnswerTableCaps(200, 12, 64, n_e - 1))
    with pytest.raises(ValueError, match="capacity S"):
        A.collate_answer_tables(tabs, A.AnswerTableCaps(50, 12, 64, 256))
    with pytest.raises(ValueError, match="decoding steps"):
        A.collate_answer_tables(tabs, A.AnswerTableCaps(200, 11, 64, 256))


def test_reference_assertion_cases_raise():
    meta, _ = golden()
    voc = A.AnswerVocab(meta["vocab"])
    assert meta["failing"]
    for c in meta["failing"]:
        with pytest.raises(ValueError):
            A.build_answer_table(c["answers"], c["context_tokens"], voc)
    with pytest.raises(ValueError, match="expected 10 answers"):
        A.build_answer_table(["red"] * 9, [], voc)
    with pytest.raises(ValueError, match="<pad> first"):
        A.AnswerVocab(["<s>", "<pad>", "</s>", "<unk>", "red"])
    with pytest.raises(ValueError, match="more than once"):
        A.AnswerVocab(["<pad>", "<s>", "</s>", "<unk>", "red", "red"])
    with pytest.raises(ValueError, match="no </s>"):
        A.AnswerVocab(["<pad>", "<s>", "<unk>", "red"])


def test_unk_only_at_step0_is_accepted_as_upstream():
    """upstream asserts on the target indices of steps t >= 1 only: <unk> starting an answer is a valid (if odd) step-0 target"""
    meta, _ = golden()
    voc = A.AnswerVocab(meta["vocab"])
    t = A.build_answer_table(["<unk> red"] * 10, [], voc)
    assert voc.UNK_IDX in t["step0_idx"].tolist()


def test_ocr_tokens_are_cut_to_max_ocr_tokens():
    meta, _ = golden()
    voc = A.AnswerVocab(meta["vocab"])
    t = A.build_answer_table(["w55"] * 10, ["w%d" % i for i in range(60)], voc)
    assert len(t["seq_len"]) == 0
    t = A.build_answer_table(["w55"] * 10, ["w%d" % i for i in range(60)], voc, max_ocr_tokens=60)
    assert t["step0_idx"].tolist() == [len(voc) + 55] and int(t["dims"][0]) == len(voc) + 60


def test_host_draw_is_deterministic_in_range_and_folds_in_rank():
    n = np.array([0, 1, 2, 7, 200, 13])
    a = A.draw_choices(A.answer_key(5, 0), 3, n)
    np.testing.assert_array_equal(a, A.draw_choices(A.answer_key(5, 0), 3, n))
    assert a[0] == -1 and a[1] == 0 and ((a[1:] >= 0) & (a[1:] < n[1:])).all()
    n = np.full(64, 200)
    r0, r1 = A.draw_choices(A.answer_key(5, 0), 3, n), A.draw_choices(A.answer_key(5, 1), 3, n)
    s1 = A.draw_choices(A.answer_key(5, 0), 4, n)
    assert (r0 != r1).sum() > 50 and (r0 != s1).sum() > 50
    assert A.answer_key(5, 1) == 5 ^ (1 << 32)
    # uniform: 20 000 steps over 7 candidates, chi-square with 6 degrees of freedom (deterministic seeds: never flaky)
    cnt = np.zeros(7)
    for st in range(20000):
        cnt[A.draw_choices(A.answer_key(11), st, [7])[0]] += 1
    chi2 = (((cnt - 20000 / 7) ** 2) / (20000 / 7)).sum()
    assert chi2 < 22.5, chi2                                                   # p = 0.001


def test_hash_matches_a_scalar_restatement():
    def mix(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    key, step = 0x0123456789ABCDEF, -3 & 0xFFFFFFFFFFFFFFFF
    for b in range(5):
        h = mix((key & 0xFFFFFFFF) ^ 0xA0761D65)
        h = mix(h ^ (key >> 32))
        h = mix(h ^ (step & 0xFFFFFFFF))
        h = mix(h ^ (step >> 32))
        h = mix(h ^ ((b * 0x9E3779B1) & 0xFFFFFFFF))
        assert int(A.draw_hash(key, -3, [b])[0]) == h


def test_sample_answers_rejects_dense_targets_too():
    meta, _ = golden()
    _, _, table = case_tables(meta)
    with pytest.raises(ValueError, match="both"):
        A.sample_answers({"answer_table": table, "targets": torch.zeros(1)}, step=0)


def test_answer_sample_entry_point_is_bound_and_rejects_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi as capi
    import ctypes as C
    assert "sam_answer_sample" in capi.SIGNATURES
    l = capi.lib()
    rc = l.sam_answer_sample(*([None] * 8), 1, 200, 12, 64, 256, 62, 1, 0, None, 0, None, None, 62, *([None] * 4), None)
    assert rc == -1 and b"null" in l.sam_last_error()
    nn = C.c_void_p(16)
    rc = l.sam_answer_sample(*([nn] * 8), 1, 200, 12, 64, 256, 62, 1, 0, None, 0, None, nn, 61, *([nn] * 4), None)
    assert rc == -1 and b"W <= ld" in l.sam_last_error()
    rc = l.sam_answer_sample(*([nn] * 8), 1, 200, 12, 64, 256, 62, 62, 0, None, 0, None, nn, 62, *([nn] * 4), None)
    assert rc == -1 and b"bos" in l.sam_last_error()
