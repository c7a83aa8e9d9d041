"""GPU: the results board (csrc/evalboard.hip, sam_textvqa_amd/evalboard.py) on the MI355X -- collect, reduce and merge against
their host twins (which tests/test_evalboard_cpu.py judges) bit for bit in all eight board tensors, on boards filled with a sentinel beforehand so that
a stray write shows; the invariance the board exists for (one table of results through every batch size, order and sharding ends in the same board and
the same sums); the 64-bit addressing; evaluator.evaluate_indexed end to end at beam 3 and greedy; evaluator.store_batches.  No test captures a graph."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import evalboard as E
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops
from sam_textvqa_amd import sampler as S
from tests.test_evalboard_cpu import VALUES, rows_of, same, table

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
NAN_BITS = np.array([0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800001, 0x7FFFFFFF], np.int64).astype(np.int32)      # quiet, negative, signalling, all ones


def sentinel_board(n, P, rng, occupied=0.3):
    """a host board whose every element holds the sentinel, except seen (0, or a positive count in `occupied` of the rows) and status (4: a foreign bit
    that must survive)"""
    b = {k: np.full(v.shape, SENTINEL, np.int32).view(v.dtype) for k, v in E.new_host(n, P).items()}
    b["seen"] = np.where(rng.rand(n) < occupied, rng.randint(1, 9, n), 0).astype(np.int32)
    b["status"] = np.array([4], np.int32)
    return b


def to_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def diff(got, want):
    """the first board tensor that differs, with where"""
    for k in E.KEYS:
        g, w = got[k].view(np.int32), want[k].view(np.int32)
        if g.shape != w.shape or (g != w).any():
            return k, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else (g.shape, w.shape)
    return None


def batch_variants(B, n, P, rng):
    """(name, sample_idx, valid or None, answer_len override or None)"""
    inside = rng.randint(0, n, B).astype(np.int32)
    outside = inside.copy()
    pick = rng.rand(B) < 0.4
    outside[pick] = rng.choice(np.array([-1, n, n + 7, -(1 << 31), (1 << 31) - 1], np.int64), int(pick.sum())).astype(np.int32)
    some = (rng.rand(B) < 0.6).astype(np.int32)
    some[rng.rand(B) < 0.1] = -7                                 # any non-zero value is valid
    return [("random", inside, some, None), ("valid=None", inside, None, None), ("no slot valid", inside, np.zeros(B, np.int32), None),
            ("one index B times", np.full(B, n - 1, np.int32), None, None), ("one index, some valid", np.full(B, n // 2, np.int32), some, None),
            ("out of range, valid=None", outside, None, None), ("out of range under valid", outside, some, None),
            ("out of range only where valid is 0", outside, (~pick).astype(np.int32), None),
            ("answer_len outside [0, P]", inside, None, rng.choice(np.array([-3, 0, P, P + 1, (1 << 31) - 1, -(1 << 31)], np.int64), B).astype(np.int32))]


@pytest.mark.parametrize("P", [1, 13, 780])
def test_collect_equals_the_twin_in_all_eight_tensors(P):
    rng = np.random.RandomState(P)
    for n in (1, 7, 300):
        tab = table(n, P, n + P)
        for B in (1, 5, 64, 70, 257):                           # 70 and 257: the ownership scan goes past its 64-lane stride
            for name, idx, valid, lens in batch_variants(B, n, P, rng):
                res = {k: v.copy() for k, v in rows_of(tab, idx).items()}
                res["best"] = (1000 + np.arange(B)).astype(np.int32)              # every slot's row differs: the owner shows in the board
                if lens is not None:
                    res["answer_len"] = lens
                want = sentinel_board(n, P, rng)
                board = to_dev(want)
                ops.evalboard_collect(board, to_dev(res), torch.from_numpy(idx).cuda(), None if valid is None else torch.from_numpy(valid).cuda())
                E.collect_host(want, res, idx, valid)
                assert diff(to_host(board), want) is None, (name, n, B, P, diff(to_host(board), want))
                assert want["status"][0] & 4 and 0 <= want["answer_len"][want["answer_len"] != SENTINEL].min(initial=0)


def test_collect_twice_first_write_wins_and_the_board_object():
    n, P, B = 40, 6, 16
    first, second = table(n, P, 1), table(n, P, 2)
    bd, want = E.Board(n, P), E.new_host(n, P)
    assert bd.t["seen"].is_cuda and same(bd.host(), want)
    rng = np.random.RandomState(3)
    for tab in (first, second, first):
        idx, valid = rng.randint(0, n, B).astype(np.int32), (rng.rand(B) < 0.8).astype(np.int32)
        ptrs = {k: t.data_ptr() for k, t in bd.t.items()}
        bd.collect(to_dev(rows_of(tab, idx)), torch.from_numpy(idx).cuda(), torch.from_numpy(valid).cuda())
        assert ptrs == {k: t.data_ptr() for k, t in bd.t.items()}
        E.collect_host(want, rows_of(tab, idx), idx, valid)
    assert diff(bd.host(), want) is None and bd.status() == 0 and want["seen"].max() > 1
    assert bd.result() == E.result_host(want) and bd.reduce().cpu().numpy().tobytes() == E.reduce_host(want).tobytes()
    d = bd.state_dict()
    other = E.Board(n, P)
    other.load_state_dict(d)
    assert diff(other.host(), want) is None
    bd.collect(to_dev(rows_of(first, [n])), torch.tensor([n], dtype=torch.int32, device="cuda"))
    assert bd.status(check=False) == E.BAD_INDEX
    with pytest.raises(ValueError, match="bit 0"):
        bd.result()
    bd.reset()
    assert same(bd.host(), E.new_host(n, P)) and diff(other.host(), want) is None
    with pytest.raises(ops.capi.SamHipError, match="expected 96"):
        bd.collect(to_dev(rows_of(table(n, P + 1, 0), np.zeros(B, np.int32))), torch.zeros(B, dtype=torch.int32, device="cuda"))
    with pytest.raises(ops.capi.SamHipError, match="valid must be"):
        bd.collect(to_dev(rows_of(first, np.zeros(B, np.int32))), torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B + 1, dtype=torch.int32, device="cuda"))


def reduce_board(n, seed):
    """scores from the metrics' own value set and random fp32 ANLS; a third of the rows unseen (seen 0 or negative), holding NaN bit patterns"""
    rng = np.random.RandomState(seed)
    b = E.new_host(n, 2)
    b["scores"] = np.stack([VALUES[rng.randint(0, 5, n)], VALUES[rng.randint(0, 2, n) * 4], rng.rand(n).astype(np.float32)], 1)
    b["oracle"] = np.stack([VALUES[rng.randint(0, 5, n)], VALUES[rng.randint(0, 2, n) * 4], rng.rand(n).astype(np.float32)], 1)
    b["seen"] = rng.randint(1, 5, n).astype(np.int32)
    gone = rng.permutation(n) < n // 3
    b["seen"][gone] = rng.choice(np.array([0, 0, -1, -(1 << 31)], np.int64), int(gone.sum())).astype(np.int32)
    for k in ("scores", "oracle"):
        b[k].view(np.int32)[gone] = NAN_BITS[rng.randint(0, 4, (int(gone.sum()), 3))]
    return b, gone


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 35000])
def test_reduce_equals_the_twin_and_ignores_unseen_rows(n):
    b, gone = reduce_board(n, n)
    assert n < 3 or np.isnan(b["scores"][gone]).all()
    dev = to_dev(b)
    out = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    got = ops.evalboard_reduce(dev, out)
    assert got.data_ptr() == out.data_ptr()
    got, want = got.cpu().numpy(), E.reduce_host(b)
    assert np.isfinite(got).all() and got.tobytes() == want.tobytes(), (got, want)
    assert got[3] == n - gone.sum() and got[7] == b["seen"][~gone].sum()
    assert diff(to_host(dev), b) is None                         # reduce writes nothing but out
    again = ops.evalboard_reduce(dev)                            # a fresh out; the order is fixed: the same bits
    assert again.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 35000])
def test_merge_equals_the_twin(n, overlap):
    P = 3
    rng = np.random.RandomState(n + overlap)
    dst, src = sentinel_board(n, P, rng, 0.5), sentinel_board(n, P, rng, 0.5)
    for k in E.KEYS[:6]:                                         # src's rows differ from dst's sentinel
        src[k] = (np.arange(src[k].size, dtype=np.int32).reshape(src[k].shape) + 7).view(src[k].dtype)
    src["seen"][rng.rand(n) < 0.2] = -3                          # not a row
    if not overlap:
        src["seen"][dst["seen"] != 0] = 0
    src["status"][0] = 1 | 8
    d_dev, s_dev = to_dev(dst), to_dev(src)
    ops.evalboard_merge(d_dev, s_dev)
    want = E.merge_host({k: v.copy() for k, v in dst.items()}, src)
    assert diff(to_host(d_dev), want) is None, (n, overlap, diff(to_host(d_dev), want))
    assert diff(to_host(s_dev), src) is None and want["status"][0] == 13
    if n > 1:
        assert overlap == bool(((dst["seen"] > 0) & (src["seen"] > 0)).any())
    with pytest.raises(ops.capi.SamHipError, match="boards overlap"):
        ops.evalboard_merge(d_dev, dict(s_dev, seen=d_dev["seen"]))
    with pytest.raises(ops.capi.SamHipError, match="boards overlap"):
        ops.evalboard_merge(d_dev, d_dev)


@pytest.mark.parametrize("n", [1000, 999])
def test_every_route_ends_in_the_same_board_and_the_same_sums(n):
    """one fixed table of per-question results through Sampler batches at B in {3, 64, 257}, shuffled and not, as one rank and as two ranks merged:
    every route's board is bitwise the same apart from seen (the wrap padding of two ranks at an odd n), and so is reduce()[0:7]"""
    P = 13
    tab = table(n, P, 5)
    tab_dev = to_dev(tab)
    ref = E.collect_host(E.new_host(n, P), tab, np.arange(n, dtype=np.int32))
    ref_sums = E.reduce_host(ref)
    for B in (3, 64, 257):
        for shuffle in (False, True):
            for W in (1, 2):
                boards = []
                for r in range(W):
                    bd, smp = E.Board(n, P), S.Sampler(n, B, seed=21, rank=r, world=W, shuffle=shuffle)
                    slots = 0
                    for _ in range(smp.steps_per_epoch):
                        idx, valid = smp.next()
                        bd.collect({k: v[idx.long()] for k, v in tab_dev.items()}, idx, valid)
                        slots += B
                    assert slots >= -(-n // W) and smp.status() == 0
                    boards.append(bd)
                final = boards[0]
                if W == 2:
                    final = E.Board(n, P)
                    final.merge(boards[0])
                    final.merge(boards[1])
                got, where = final.host(), (n, B, shuffle, W)
                for k in E.KEYS:
                    if k != "seen":
                        assert got[k].tobytes() == ref[k].tobytes(), (where, k)
                pad = W * -(-n // W) - n
                assert got["seen"].min() == 1 and got["seen"].sum() == n + pad, where
                sums = final.reduce().cpu().numpy()
                assert sums[:7].tobytes() == ref_sums[:7].tobytes() and sums[7] == n + pad, where
                res = final.result()
                assert (res["count"], res["missing"], res["repeats"]) == (n, 0, pad), where


def test_rows_past_two_to_the_32_bytes_are_addressed_in_64_bits():
    n, P = 260000, 4160                                         # answer: 4.33e9 bytes
    assert n * P * 4 > 1 << 32
    try:
        boards = [dict(to_dev(E.new_host(n, 1)), answer=torch.empty((n, P), dtype=torch.int32, device="cuda")) for _ in range(2)]
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip("two boards of 4.33 GB each do not fit this device: %s" % str(e)[:80])
    dst, src = boards
    rng = np.random.RandomState(0)
    guard = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")
    for b in boards:
        for q in (0, 1, n - 2, n - 1, n // 2, (1 << 32) // (4 * P), (1 << 32) // (4 * P) + 1):
            b["answer"][q] = guard
    tab = table(3, P, 9)
    idx = np.array([n - 1, 0, (1 << 32) // (4 * P) + 1], np.int32)           # the last row, the first, and the first one wholly past 2^32 bytes
    ops.evalboard_collect(dst, to_dev(tab), torch.from_numpy(idx).cuda())
    for b, q in enumerate(idx.tolist()):
        assert dst["answer"][q].cpu().numpy().tobytes() == tab["answer"][b].tobytes() and dst["best"][q].item() == tab["best"][b], q
    for q in (1, n - 2, n // 2, (1 << 32) // (4 * P)):
        assert torch.equal(dst["answer"][q], guard), q
    assert dst["seen"].sum().item() == 3 and dst["status"].item() == 0
    # merge: src holds the rows n - 2 (empty in dst: copied) and n - 1 (taken in dst: kept)
    ops.evalboard_collect(src, to_dev(rows_of(tab, [1, 2])), torch.tensor([n - 2, n - 1], dtype=torch.int32, device="cuda"))
    ops.evalboard_merge(dst, src)
    assert dst["answer"][n - 2].cpu().numpy().tobytes() == tab["answer"][1].tobytes() and dst["answer"][n - 1].cpu().numpy().tobytes() == tab["answer"][0].tobytes()
    assert dst["seen"][[0, n - 2, n - 1]].tolist() == [1, 1, 2] and dst["seen"].sum().item() == 5
    assert torch.equal(dst["answer"][n // 2], guard) and torch.equal(dst["answer"][1], guard)
    sums = ops.evalboard_reduce(dst).cpu().numpy()
    assert sums[3] == 4 and sums[7] == 5


# ---------------------------------------------------------------------------------------------- the evaluator
def _seven_questions():
    """the smallest model of tests/test_decode_gpu.py, a batch of seven questions and their score tables, built the way
    tests/test_eval_beams_gpu.test_evaluator_end_to_end_equals_the_host_on_the_same_beams builds them"""
    from sam_textvqa_amd.registry import registry
    from tests.test_decode_gpu import _batch, _models
    model, _, shapes = _models(layers=("n", "s"))
    registry.EOS_IDX, registry.BOS_IDX = 2, 1
    n, n_ocr = 7, shapes[2]
    voc, answers, tokens = M.make_score_text(n, num_vocab=300, n_ocr=n_ocr, seed=4)
    assert len(voc) == 300 and voc.EOS_IDX == 2
    tabs = [M.build_score_table(a, t, max_ocr_tokens=n_ocr) for a, t in zip(answers, tokens)]
    bd = _batch(n, shapes, 300, 40, "cuda")
    bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"])
    bd["train_prev_inds"][:, 0] = 1
    return model, M.vocab_text(voc), tabs, bd


def _take(bd, idx):
    sel = torch.as_tensor(idx, dtype=torch.long, device="cuda")
    out = {k: v[sel].clone() for k, v in bd.items() if torch.is_tensor(v)}
    out["spatial_adj_matrices"] = {k: v[sel].clone() for k, v in bd["spatial_adj_matrices"].items()}
    return out


@pytest.mark.parametrize("beam", [3, 0], ids=["beam3", "greedy"])
def test_evaluate_indexed_end_to_end_counts_every_question_once(beam, tmp_path):
    """n = 7 questions in batches of 3 drawn by Sampler(shuffle=False): three batches, the last with two wrapped slots.  The result is that of
    evaluate_beams_host -> collect_host -> reduce_host on the complete_seqs / topkscores (beam 3) or the argmax (greedy) each forward left."""
    import json
    from sam_textvqa_amd import evaluator as Ev
    model, vt, tabs, bd = _seven_questions()
    n, B = 7, 3
    qids = [70, 5, 33, 170, 105, 133, 9]
    smp = S.Sampler(n, B, shuffle=False)
    assert smp.steps_per_epoch == 3
    seen, drawn = [], []

    def feed():
        for _ in range(smp.steps_per_epoch):
            idx, valid = smp.next()
            at = idx.cpu().tolist()
            batch = _take(bd, at)
            batch["score_table"] = M.collate_score_tables([tabs[q] for q in at])
            batch["sample_idx"], batch["valid"] = idx, valid
            drawn.append((at, valid.cpu().tolist()))
            yield batch
            if beam:
                seen.append((batch["complete_seqs"].reshape(B * beam, -1).cpu().numpy().copy(), batch["topkscores"].reshape(-1).cpu().numpy().copy()))
            else:
                seen.append((batch["scores"].argmax(-1).cpu().numpy().copy(), np.zeros(B, np.float32)))

    L = 11 if beam else 12                                      # beam search: the BOS column is skipped; greedy: all 12 steps are predictions
    P = L * (vt["cp"].shape[1] + 1)
    board = E.Board(n, P, question_ids=qids)
    res = Ev.evaluate_indexed(model, feed(), vt, beam, board)
    assert not model.training and len(seen) == 3
    assert drawn == [([0, 1, 2], [1, 1, 1]), ([3, 4, 5], [1, 1, 1]), ([6, 0, 1], [1, 0, 0])]
    assert sum(len(at) for at, _ in drawn) == 9                  # what evaluate would count on these batches: questions 0 and 1 twice
    want = E.new_host(n, P)
    for (seqs, cum), (at, valid) in zip(seen, drawn):
        assert seqs.shape == (B * max(beam, 1), 12)
        h = M.evaluate_beams_host(seqs, cum, M.collate_score_tables([tabs[q] for q in at]), vt, max(beam, 1), skip=1 if beam else 0)
        E.collect_host(want, h, np.array(at, np.int32), np.array(valid, np.int32))
    assert diff(board.host(), want) is None
    assert res == E.result_host(want, question_ids=qids)
    assert (res["count"], res["missing"], res["repeats"]) == (7, 0, 0) and [a["question_id"] for a in res["answers"]] == qids
    red = E.reduce_host(want)
    assert (res["vqa_accuracy"], res["stvqa_accuracy"], res["anls"]) == tuple(red[:3] / 7) and res["oracle"] == list(red[4:7] / 7)
    Ev.write_evalai(res, str(tmp_path / "evalai.json"))
    assert json.load(open(tmp_path / "evalai.json")) == res["answers"]
    with pytest.raises(ValueError, match="needs sample_idx"):
        Ev.evaluate_indexed(model, [_take(bd, [0])], vt, beam, board)
    with pytest.raises(ValueError, match="no batches"):
        Ev.evaluate_indexed(model, [], vt, beam, board)


def test_store_batches_two_ranks_cover_every_question_once():
    from sam_textvqa_amd import evaluator as Ev
    from sam_textvqa_amd import store
    from tests.test_sampler_gpu import _small_store
    s_host = _small_store()
    s_dev = store.to(s_host, "cuda")
    n, B, n_max, P = 23, 4, 4, 5
    tab = table(n, P, 12)
    tab_dev = to_dev(tab)
    shape, _ = store.gather_host(s_host, torch.zeros(B, dtype=torch.int32), max_obj_num=n_max, max_ocr_num=n_max)
    boards, wants = [], []
    for r in range(2):
        smp = S.for_store(s_dev, B, seed=8, rank=r, world=2)
        into = {k: torch.zeros_like(v, device="cuda") for k, v in shape.items()}
        into_h = {k: torch.zeros_like(v) for k, v in shape.items()}              # reused like `into`: rows past a batch's total keep what they held
        bd, want, state, steps = E.Board(n, P), E.new_host(n, P), (8, 0, 0, 0), 0
        for batch in Ev.store_batches(s_dev, smp, into, max_obj_num=n_max, max_ocr_num=n_max):
            assert batch is into
            w_idx, w_valid, state = S.batch_host(state, n, B, r, 2)
            assert batch["sample_idx"].cpu().tolist() == w_idx.tolist() and batch["valid"].cpu().tolist() == w_valid.tolist()
            store.gather_host(s_host, torch.from_numpy(w_idx), into=into_h, max_obj_num=n_max, max_ocr_num=n_max)
            for k in into_h:
                assert torch.equal(batch[k].cpu().view(-1).view(torch.uint8), into_h[k].view(-1).view(torch.uint8)), k
            bd.collect({k: v[batch["sample_idx"].long()] for k, v in tab_dev.items()}, batch["sample_idx"], batch["valid"])
            E.collect_host(want, rows_of(tab, w_idx), w_idx, w_valid)
            steps += 1
        assert steps == smp.steps_per_epoch == 3 and smp.state.tolist() == [8, 1, 0, 3]
        assert diff(bd.host(), want) is None and 0 < (want["seen"] > 0).sum() < n
        boards.append(bd)
        wants.append(want)
    assert len(list(Ev.store_batches(s_dev, S.for_store(s_dev, B), into, steps=2, max_obj_num=n_max, max_ocr_num=n_max))) == 2
    boards[0].merge(boards[1])
    merged = E.merge_host(wants[0], wants[1])
    assert diff(boards[0].host(), merged) is None
    res = boards[0].result()
    assert (res["count"], res["missing"], res["repeats"]) == (n, 0, 1) and merged["seen"].min() == 1       # all 23 questions, the one padded repeat
    assert [a["question_id"] for a in res["answers"]] == list(range(n))
    for k, r in zip(E.KEYS[:6], E.ROW_KEYS):
        assert merged[k].tobytes() == tab[r].tobytes(), k
