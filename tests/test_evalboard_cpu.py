"""CPU: the results board's host twins (sam_textvqa_amd/evalboard.py), which are its definition -- the ownership rule, first
write wins, the fixed summation order, two ranks' boards merged against the single rank's over sampler.batch_host's epochs -- and the registry line, the
derived signatures and every argument check of the three entry points (csrc/evalboard.hip), which need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from sam_textvqa_amd import evalboard as E
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import sampler as S

VALUES = np.array([0.0, 0.3, 0.6, 0.9, 1.0], np.float32)                    # what the two accuracies can be


def table(n, P, seed):
    """a fixed table of per-question results, in evaluate_beams' keys: what question q yields whenever it is evaluated"""
    rng = np.random.RandomState(seed)
    ln = rng.randint(0, P + 1, n).astype(np.int32)
    ans = rng.randint(1, 0x10FFFF, (n, P)).astype(np.int32) * (np.arange(P)[None, :] < ln[:, None])
    sc = np.stack([VALUES[rng.randint(0, 5, n)], VALUES[rng.randint(0, 2, n) * 4], rng.rand(n).astype(np.float32)], 1)
    return {"best_scores": sc, "oracle": np.maximum(sc, rng.rand(n, 3).astype(np.float32)), "best_flags": rng.randint(0, 4, n).astype(np.int32),
            "best": rng.randint(0, 5, n).astype(np.int32), "answer": ans.astype(np.int32), "answer_len": ln}


def rows_of(tab, idx):
    """the batch a model would produce for the questions idx: out-of-range slots hold question 0's rows"""
    idx = np.asarray(idx, np.int64)
    safe = np.where((idx >= 0) & (idx < tab["best"].shape[0]), idx, 0)
    return {k: v[safe] for k, v in tab.items()}


def same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in E.KEYS) and set(a) == set(b) == set(E.KEYS)


def test_a_batch_equal_to_the_board_in_index_order_reproduces_its_inputs():
    n, P = 9, 6
    tab = table(n, P, 0)
    b = E.collect_host(E.new_host(n, P), tab, np.arange(n, dtype=np.int32))
    for k, r in zip(E.KEYS[:6], E.ROW_KEYS):
        assert b[k].tobytes() == tab[r].tobytes() and b[k].dtype == tab[r].dtype, k
    assert b["seen"].tolist() == [1] * n and b["status"].tolist() == [0]
    assert {k: v.dtype for k, v in E.new_host(1, 1).items()} == {k: np.dtype(E._DTYPES[k]) for k in E.KEYS}
    assert not any(v.any() for v in E.new_host(3, 2).values())


def test_the_ownership_rule_on_a_hand_written_batch():
    n, P = 5, 4
    tab = table(n, P, 1)
    #      slot:   0  1   2  3  4  5  6  7   8
    idx = np.array([2, 2, -1, 5, 0, 2, 4, 5, -1], np.int32)
    valid = np.array([0, 1, 0, 1, 1, 1, 0, 0, 1], np.int32)
    res = rows_of(tab, idx)
    for k in res:                                               # every slot's row differs, so the owner is visible in the board
        res[k] = res[k].copy()
    res["best"][:] = 100 + np.arange(9)
    res["answer_len"][4] = P + 7                                # clamped to P
    res["answer_len"][1] = -2                                   # clamped to 0
    b = E.collect_host(E.new_host(n, P), res, idx, valid)
    # live: slots 1, 4, 5 (slot 0 is not valid, 3 and 8 are valid but out of range, 2, 6, 7 are not valid).  Slot 1 owns q = 2 with m = 2; slot 4 owns q = 0.
    assert b["seen"].tolist() == [1, 0, 2, 0, 0] and b["status"].tolist() == [E.BAD_INDEX]
    assert b["best"].tolist() == [104, 0, 101, 0, 0] and b["answer_len"].tolist() == [P, 0, 0, 0, 0]
    assert b["answer"][2].tolist() == res["answer"][1].tolist() and b["scores"][0].tolist() == res["best_scores"][4].tolist()
    assert not b["answer"][[1, 3, 4]].any() and not b["scores"][[1, 3, 4]].any()
    # without valid every slot counts: slot 0 owns q = 2 with m = 3; q = 4 appears; the status bit comes from slots 2, 3, 7, 8
    b = E.collect_host(E.new_host(n, P), res, idx)
    assert b["seen"].tolist() == [1, 0, 3, 0, 1] and b["status"].tolist() == [1] and b["best"].tolist() == [104, 0, 100, 0, 106]
    # an out-of-range slot that is not valid is ignored
    b = E.collect_host(E.new_host(n, P), res, idx, (valid * (idx >= 0) * (idx < n)).astype(np.int32))
    assert b["status"].tolist() == [0] and b["seen"].tolist() == [1, 0, 2, 0, 0]
    # all slots invalid: nothing moves
    assert same(E.collect_host(E.new_host(n, P), res, idx, np.zeros(9, np.int32)), E.new_host(n, P))
    with pytest.raises(ValueError, match="batch of"):
        E.collect_host(E.new_host(n, P + 1), res, idx)


def test_first_write_wins_across_two_collects():
    n, P = 6, 3
    first, second = table(n, P, 2), table(n, P, 3)
    b = E.collect_host(E.new_host(n, P), rows_of(first, [1, 3, 3]), np.array([1, 3, 3], np.int32))
    E.collect_host(b, rows_of(second, [3, 4, 1, 1]), np.array([3, 4, 1, 1], np.int32), np.array([1, 1, 1, 0], np.int32))
    assert b["seen"].tolist() == [0, 2, 0, 3, 1, 0]
    for k, r in zip(E.KEYS[:6], E.ROW_KEYS):
        assert b[k][[1, 3]].tobytes() == first[r][[1, 3]].tobytes() and b[k][4].tobytes() == second[r][4].tobytes(), k
    b["seen"][1] = 0x7FFFFFFF                                    # int32 two's complement, as the kernel's unsigned add
    E.collect_host(b, rows_of(second, [1]), np.array([1], np.int32))
    assert b["seen"][1] == -(1 << 31)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_reduce_host_is_host_totals_on_the_seen_rows_and_ignores_the_rest(n):
    tab = table(n, 2, n)
    full = E.collect_host(E.new_host(n, 2), tab, np.arange(n, dtype=np.int32))
    red = E.reduce_host(full)
    assert red.dtype == np.float64 and red.shape == (8,)
    assert red[:4].tobytes() == M.host_totals(tab["best_scores"]).tobytes()
    assert red[4:7].tobytes() == M.host_totals(tab["oracle"])[:3].tobytes() and red[7] == n
    # a third of the rows unseen, holding NaN and garbage: the sums are those of the board with these rows at zero, in the board's row order
    part = {k: v.copy() for k, v in full.items()}
    gone = np.arange(n) % 3 == 1
    part["seen"][gone] = np.where(np.arange(n)[gone] % 2, 0, -5)
    part["scores"][gone], part["oracle"][gone] = np.nan, -np.inf
    part["seen"][~gone] = 1 + np.arange(n)[~gone] % 4
    red = E.reduce_host(part)
    zeroed = np.where(gone[:, None], np.float32(0), tab["best_scores"])
    assert np.isfinite(red).all() and red[:3].tobytes() == M.host_totals(zeroed)[:3].tobytes()
    assert red[3] == (~gone).sum() and red[7] == part["seen"][~gone].sum()
    # the two accuracy columns are sums of multiples of 2^-25 below 2^28: exact in float64, so any order gives them, host_totals of the seen rows alone too
    assert red[:2].tobytes() == M.host_totals(tab["best_scores"][~gone])[:2].tobytes()
    assert abs(red[2] - M.host_totals(tab["best_scores"][~gone])[2]) <= 1e-9 * max(n, 1)


def epoch(n, B, W, r, shuffle, seed=11):
    state = (seed, 0, 0, 0)
    for _ in range(S.plan(n, B, r, W)[1]):
        idx, valid, state = S.batch_host(state, n, B, r, W, shuffle=shuffle)
        yield idx, valid


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 5, 7, 17])
def test_two_ranks_merged_equal_the_single_rank(n, B, shuffle):
    P = 5
    tab = table(n, P, 7 * n + B)
    single = E.new_host(n, P)
    for idx, valid in epoch(n, B, 1, 0, shuffle):
        E.collect_host(single, rows_of(tab, idx), idx, valid)
    assert single["seen"].tolist() == [1] * n and single["status"][0] == 0
    ranks = []
    for r in range(2):
        b = E.new_host(n, P)
        for idx, valid in epoch(n, B, 2, r, shuffle):
            E.collect_host(b, rows_of(tab, idx), idx, valid)
        ranks.append(b)
    merged = E.merge_host(E.merge_host(E.new_host(n, P), ranks[0]), ranks[1])
    for k in E.KEYS:
        if k != "seen":
            assert merged[k].tobytes() == single[k].tobytes(), k
    pad = 2 * -(-n // 2) - n
    assert merged["seen"].min() >= 1 and merged["seen"].max() <= 2 and merged["seen"].sum() == n + pad
    res, one = E.result_host(merged), E.result_host(single)
    assert res["repeats"] == pad and res["missing"] == 0 and res["count"] == n and one["repeats"] == 0
    assert E.reduce_host(merged)[:7].tobytes() == E.reduce_host(single)[:7].tobytes()
    assert {k: v for k, v in res.items() if k != "repeats"} == {k: v for k, v in one.items() if k != "repeats"}
    assert [a["question_id"] for a in res["answers"]] == list(range(n))
    assert same(E.merge_host({k: v.copy() for k, v in ranks[1].items()}, E.new_host(n, P)), ranks[1])      # an empty src changes nothing


def test_merge_keeps_dst_rows_adds_seen_and_ors_status():
    n, P = 4, 2
    a, b = table(n, P, 20), table(n, P, 21)
    dst = E.collect_host(E.new_host(n, P), rows_of(a, [0, 1]), np.array([0, 1], np.int32))
    src = E.collect_host(E.new_host(n, P), rows_of(b, [1, 1, 2, 9]), np.array([1, 1, 2, 9], np.int32))
    src["seen"][3], src["best"][3] = -4, 77                      # a row with seen <= 0 is not a row
    E.merge_host(dst, src)
    assert dst["seen"].tolist() == [1, 3, 1, 0] and dst["status"].tolist() == [1] and dst["best"][3] == 0
    assert dst["answer"][1].tolist() == a["answer"][1].tolist() and dst["answer"][2].tolist() == b["answer"][2].tolist()
    with pytest.raises(ValueError, match="share no memory"):
        E.merge_host(dst, dst)
    with pytest.raises(ValueError, match="different shapes"):
        E.merge_host(dst, E.new_host(n, P + 1))


def test_result_question_ids_missing_and_the_status_word(tmp_path):
    import json
    from sam_textvqa_amd import evaluator
    n, P = 5, 8
    tab = table(n, P, 30)
    tab["answer"][3, :3], tab["answer_len"][3] = [ord(c) for c in "abc"], 3
    b = E.collect_host(E.new_host(n, P), rows_of(tab, [3, 1, 3]), np.array([3, 1, 3], np.int32))
    res = E.result_host(b, question_ids=[50, 40, 30, 20, 10])
    assert (res["count"], res["missing"], res["repeats"]) == (2, 3, 1) and [a["question_id"] for a in res["answers"]] == [40, 20]
    assert res["answers"][1]["answer"] == "abc"
    want = M.host_totals(np.where(b["seen"][:, None] > 0, tab["best_scores"], np.float32(0)))
    assert (res["vqa_accuracy"], res["stvqa_accuracy"], res["anls"]) == tuple(want[:3] / 2) and len(res["oracle"]) == 3
    evaluator.write_evalai(res, str(tmp_path / "evalai.json"))
    assert json.load(open(tmp_path / "evalai.json")) == res["answers"]
    assert E.result_host(b, question_ids=torch.tensor([50, 40, 30, 20, 10]))["answers"] == res["answers"]
    with pytest.raises(ValueError, match="question ids"):
        E.result_host(b, question_ids=[1, 2])
    with pytest.raises(ValueError, match="no question"):
        E.result_host(E.new_host(n, P))
    E.collect_host(b, rows_of(tab, [7]), np.array([7], np.int32))
    with pytest.raises(ValueError, match="bit 0"):
        E.result_host(b)
    assert E.result_host(b, check=False)["count"] == 2


def test_board_object_on_the_cpu_state_dict_and_no_fallback():
    from sam_textvqa_amd import _capi
    bd = E.Board(6, 4, device="cpu", question_ids=range(10, 16))
    assert (bd.n, bd.P, bd.question_ids) == (6, 4, list(range(10, 16))) and set(bd.t) == set(E.KEYS)
    assert {k: (tuple(t.shape), t.dtype) for k, t in bd.t.items()} == {
        "scores": ((6, 3), torch.float32), "oracle": ((6, 3), torch.float32), "flags": ((6,), torch.int32), "best": ((6,), torch.int32),
        "answer": ((6, 4), torch.int32), "answer_len": ((6,), torch.int32), "seen": ((6,), torch.int32), "status": ((1,), torch.int32)}
    assert not any(t.any() for t in bd.t.values()) and bd.status() == 0
    bd.t["seen"][2], bd.t["best"][2] = 3, 9
    d = bd.state_dict()
    other = E.Board(6, 4, device="cpu", question_ids=range(10, 16))
    other.load_state_dict(d)
    assert all(torch.equal(other.t[k], bd.t[k]) for k in E.KEYS) and other.t["seen"].data_ptr() != d["seen"].data_ptr()
    assert same(other.host(), {k: v.numpy() for k, v in d.items() if k in E.KEYS})
    other.reset()
    assert not any(t.any() for t in other.t.values()) and other.question_ids == list(range(10, 16))
    for bad in (E.Board(7, 4, device="cpu", question_ids=range(7)), E.Board(6, 5, device="cpu", question_ids=range(10, 16)), E.Board(6, 4, device="cpu")):
        with pytest.raises(ValueError, match="saved state"):
            bad.load_state_dict(d)
    with pytest.raises(ValueError, match="saved state"):
        other.load_state_dict(dict(d, seen=d["seen"].long()))
    for n, P in ((0, 4), (1 << 31, 4), (5, 0)):
        with pytest.raises(ValueError, match="evalboard"):
            E.Board(n, P, device="cpu")
    with pytest.raises(ValueError, match="merge needs"):
        bd.merge(bd)
    with pytest.raises(ValueError, match="merge needs"):
        bd.merge(E.Board(6, 5, device="cpu"))
    res = {k: torch.from_numpy(v) for k, v in table(2, 4, 0).items()}
    for launch in (lambda: bd.collect(res, torch.zeros(2, dtype=torch.int32)), bd.reduce, lambda: bd.merge(E.Board(6, 4, device="cpu")), bd.result):
        with pytest.raises(_capi.SamHipError):                  # no CPU path: the twins are the definition, not a fallback
            launch()


# ---------------------------------------------------------------------------------------------- registry and C ABI
NAMES = ("sam_evalboard_collect", "sam_evalboard_reduce", "sam_evalboard_merge")


def test_the_header_parses_into_the_open_table_and_the_library_holds_the_kernels():
    from sam_textvqa_amd import _build, _capi
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "evalboard" in _build.ABI_ADDITIONS and _build.ABI_ADDITIONS["evalboard"] in _build.public_headers()
    assert list(_build.ABI_ADDITIONS)[-1] == "evalboard" and os.path.basename(_build.ABI_ADDITIONS["evalboard"]) == "sam_hip_evalboard.h"
    assert _capi.ADDITION_SIGNATURES["evalboard"] == {"sam_evalboard_collect": [vp, vp, i] + [vp] * 6 + [i64, i] + [vp] * 8 + [vp],
                                                      "sam_evalboard_reduce": [vp, vp, vp, i64, vp, vp],
                                                      "sam_evalboard_merge": [vp] * 16 + [i64, i, vp]}
    assert _capi.ADDITION_RESTYPES["evalboard"] == {k: i for k in NAMES}
    for other in ("sampler", "store", "aux_stats"):
        assert "sam_evalboard" not in open(_build.ABI_ADDITIONS[other]).read()
    assert "sam_evalboard" not in open(_build.HEADERS["eval"]).read() and "sam_evalboard" not in open(_build.HEADER).read()
    assert os.path.join(_build.CSRC, "evalboard.hip") in _build.sources()
    lib = _capi.lib()                                           # builds evalboard.hip for gfx950 with the rest when the tree changed
    assert lib.sam_build_digest().decode() == _build._digest()
    for k in NAMES:
        assert getattr(lib, k).argtypes == _capi.ADDITION_SIGNATURES["evalboard"][k] and getattr(lib, k).restype is i


FAKE = 1 << 20                                                  # never dereferenced: the checks reject the call before any launch
STEP = 1 << 16                                                  # the fake tensors lie 64 KiB apart: boards of n = 23, P = 8 do not overlap


def test_collect_rejects_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi
    names = ("sample_idx", "valid", "best_scores", "oracle", "best_flags", "best", "answer", "answer_len", "b_scores", "b_oracle", "b_flags", "b_best", "b_answer",
             "b_answer_len", "b_seen", "b_status")

    def call(n=23, B=4, P=8, **kw):
        p = {k: FAKE + j * STEP for j, k in enumerate(names)}
        p.update(kw)
        return _capi.call("sam_evalboard_collect", p["sample_idx"], p["valid"], B, *[p[k] for k in names[2:8]], n, P, *[p[k] for k in names[8:]], None)

    for k in names:
        if k == "valid":
            continue
        with pytest.raises(_capi.SamHipError, match="null") as e:
            call(**{k: None})
        assert "rc=-1" in str(e.value)                          # SAM_ERR_ARG
    for k in names:
        with pytest.raises(_capi.SamHipError, match="misaligned"):
            call(**{k: FAKE + 2})
    for B in (0, -3):
        with pytest.raises(_capi.SamHipError, match="bad shape"):
            call(B=B)
    for P in (0, -1):
        with pytest.raises(_capi.SamHipError, match="bad answer width"):
            call(P=P)
    for n in (0, -1, 1 << 31, 1 << 40):
        with pytest.raises(_capi.SamHipError, match="bad size"):
            call(n=n)


def test_reduce_and_merge_reject_bad_arguments_without_a_gpu():
    from sam_textvqa_amd import _capi

    def reduce(scores=FAKE, oracle=FAKE + STEP, seen=FAKE + 2 * STEP, n=23, out=FAKE + 3 * STEP):
        return _capi.call("sam_evalboard_reduce", scores, oracle, seen, n, out, None)

    for kw in (dict(scores=None), dict(oracle=None), dict(seen=None), dict(out=None)):
        with pytest.raises(_capi.SamHipError, match="null pointer"):
            reduce(**kw)
    for kw in (dict(scores=FAKE + 1), dict(oracle=FAKE + 2), dict(seen=FAKE + 3), dict(out=FAKE + 4)):      # out holds float64: 8-byte alignment
        with pytest.raises(_capi.SamHipError, match="misaligned"):
            reduce(**kw)
    for n in (0, -1, 1 << 31):
        with pytest.raises(_capi.SamHipError, match="bad size"):
            reduce(n=n)

    def merge(n=23, P=8, **kw):
        p = [FAKE + j * STEP for j in range(16)]
        for j, v in kw.items():
            p[int(j[1:])] = v
        return _capi.call("sam_evalboard_merge", *p, n, P, None)

    for j in range(16):
        with pytest.raises(_capi.SamHipError, match="null (dst|src) pointer"):
            merge(**{"p%d" % j: None})
        with pytest.raises(_capi.SamHipError, match="misaligned"):
            merge(**{"p%d" % j: FAKE + j * STEP + 2})
    for n in (0, 1 << 31):
        with pytest.raises(_capi.SamHipError, match="bad size"):
            merge(n=n)
    with pytest.raises(_capi.SamHipError, match="bad answer width"):
        merge(P=0)
    # aliasing: the same tensor on both sides, a src tensor inside another dst tensor, and the last byte of the widest tensor
    for j in range(8):
        with pytest.raises(_capi.SamHipError, match="boards overlap"):
            merge(**{"p%d" % (8 + j): FAKE + j * STEP})
    with pytest.raises(_capi.SamHipError, match="boards overlap"):
        merge(p14=FAKE + 4 * STEP + 4 * (23 * 8 - 1))           # src.seen starts at dst.answer's last element
    with pytest.raises(_capi.SamHipError, match="boards overlap"):
        merge(p7=FAKE + 12 * STEP + 4 * (23 * 8 - 1) - 0)       # dst.status is src.answer's last element
    with pytest.raises(_capi.SamHipError, match="boards overlap"):
        merge(n=1 << 20, P=1)                                   # the tensors now reach into each other
    # the Python wrappers: CPU tensors are refused, a board of the wrong shape is named
    from sam_textvqa_amd import ops
    bd = E.Board(3, 2, device="cpu")
    with pytest.raises(_capi.SamHipError, match="GPU"):
        ops.evalboard_reduce(bd.t)
    with pytest.raises(_capi.SamHipError, match="lacks 'seen'"):
        ops.evalboard_reduce({k: v for k, v in bd.t.items() if k != "seen"})
