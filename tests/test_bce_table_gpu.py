"""GPU: the answer-table loss path (csrc/bce_table.hip, sam_bce_loss_table) -- gradients bit-identical to sam_bce_loss on the targets the
dense sampler writes for the same draw (full c3 size, odd widths, unaligned strides, both op routes), the greedy predictions equal to torch.argmax and
sam_greedy_pick with ties going to the lowest index, masked rows predicted only on request, hostile tables matching the dense path fed the same table,
the loss-only call storing nothing else, and a Trainer in "table" mode (eager, captured, pipelined, 1-rank data parallel) training like the dense one."""
import os
import sys

import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi as capi
from sam_textvqa_amd import answers as A
from sam_textvqa_amd import ops
from tests.test_answers_cpu import case_tables, golden
from tests.test_answers_gpu import batches, on_gpu, sample, small_model, with_inputs

pytestmark = pytest.mark.gpu

SPARSE_KEYS = ("train_prev_inds", "train_loss_mask", "train_acc_mask", "answer_choice")


def tables_for(shape):
    """(collated table on the GPU, V, No, row strides of the two score blocks or None) -- tables built as tests/test_answers_cpu.py::case_tables builds them"""
    if shape == "c3":                                      # B = 64, V = 5000, No = 50: the flagship width, 8-byte column pairs
        voc, tabs = A.make_answer_tables(64, seed=3)
        return on_gpu(A.collate_answer_tables(tabs)), len(voc), 50, None
    if shape == "odd_width":                               # V = 201, No = 49: both odd -> the one-column path
        voc, tabs = A.make_answer_tables(5, num_vocab=201, n_ocr=49, seed=4)
        return on_gpu(A.collate_answer_tables(tabs)), len(voc), 49, None
    meta, _ = golden()                                     # the reference-generated cases, even widths under ODD row strides (unaligned rows)
    voc, _, table = case_tables(meta)
    return on_gpu(table), len(voc), meta["max_ocr_tokens"], (len(voc) + 3, meta["max_ocr_tokens"] + 1)


def scores(R, V, No, strides=None, seed=0, scale=3.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ldf, ldo = (V, No) if strides is None else strides
    fixed = (torch.randn(R, ldf, device="cuda", generator=g) * scale)[:, :V]
    ocr = (torch.randn(R, ldo, device="cuda", generator=g) * scale)[:, :No]
    return fixed, ocr


def dense_route(tab, W, bos, fixed, ocr, **draw):
    """the parent path: the dense sampler, then sam_bce_loss on the targets it wrote"""
    out = sample(tab, W, bos, **draw)
    R = fixed.shape[0]
    loss, d_fixed, d_ocr = ops.bce_loss(fixed, ocr, out["targets"].reshape(R, W), out["train_loss_mask"].reshape(R))
    return out, loss, d_fixed, d_ocr


def sparse_sample(tab, W, bos, key=0, step=0, force=None):
    B, _, L = tab["seq_grp"].shape
    out = ops.answer_outputs(B, L, W, "cuda", dense=False)
    assert "targets" not in out
    fc = None if force is None else torch.as_tensor(force, dtype=torch.int32, device="cuda")
    ops.answer_sample(tab, W, bos, key, step=step, force_choice=fc, out=out)
    return out


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


# ---------------------------------------------------------------------------------------------- 4. bitwise gradients
@pytest.mark.parametrize("route", ["1", "0"])
@pytest.mark.parametrize("shape", ["c3", "odd_width", "odd_stride"])
def test_gradients_are_bit_identical_to_the_dense_pair(shape, route, monkeypatch):
    monkeypatch.setenv("SAM_COARSE_OPS", route)
    tab, V, No, strides = tables_for(shape)
    W, bos = V + No, 1
    B, _, L = tab["seq_grp"].shape
    R = B * L
    fixed, ocr = scores(R, V, No, strides, seed=1)
    n = tab["meta"][:, 0].cpu().numpy()
    rng = np.random.RandomState(0)
    force = np.where(n > 0, (rng.rand(len(n)) * np.maximum(n, 1)).astype(np.int64), -1)
    for draw in (dict(force=force), dict(key=A.answer_key(9, 0), step=7)):
        dense, loss_d, df_d, do_d = dense_route(tab, W, bos, fixed, ocr, **draw)
        sp = sparse_sample(tab, W, bos, **draw)
        for k in SPARSE_KEYS:                              # the sampler without targets writes everything else exactly as with them
            assert torch.equal(sp[k], dense[k]), k
        loss_t, df_t, do_t, pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], sp["train_loss_mask"].reshape(R))
        assert pred is None
        assert df_t.dtype == torch.bfloat16 and do_t.dtype == torch.float32
        assert torch.equal(df_t.view(torch.int16), df_d.view(torch.int16)), shape
        assert torch.equal(do_t, do_d), shape
        print("%s route %s: loss table %.9g dense %.9g" % (shape, route, loss_t.item(), loss_d.item()))
        assert rel(loss_t.item(), loss_d.item()) <= 1e-6
        # with predictions (one block per row instead of column chunks) the gradients are the same bits again
        loss_p, df_p, do_p, pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], sp["train_loss_mask"].reshape(R), pred=True, grad_scale=1.0)
        assert torch.equal(df_p.view(torch.int16), df_d.view(torch.int16)) and torch.equal(do_p, do_d)
        assert rel(loss_p.item(), loss_d.item()) <= 1e-6
        assert torch.equal(pred, torch.argmax(torch.cat([fixed, ocr], 1), 1))


def test_grad_scale_and_global_count_match_the_dense_kernel_bitwise():
    tab, V, No, _ = tables_for("odd_stride")
    W, bos = V + No, 1
    B, _, L = tab["seq_grp"].shape
    R = B * L
    fixed, ocr = scores(R, V, No, None, seed=2)
    out = sample(tab, W, bos, key=5, step=3)
    gc = torch.tensor([37.0], device="cuda")
    mask = out["train_loss_mask"].reshape(R)
    loss_d, df_d, do_d = ops.bce_loss(fixed, ocr, out["targets"].reshape(R, W), mask, 128.0, gc)
    loss_t, df_t, do_t, _ = ops.bce_loss_table(fixed, ocr, tab, out["answer_choice"], mask, 128.0, gc)
    assert torch.equal(df_t.view(torch.int16), df_d.view(torch.int16)) and torch.equal(do_t, do_d)
    assert rel(loss_t.item(), loss_d.item()) <= 1e-6


# ---------------------------------------------------------------------------------------------- 5. argmax
def test_pred_equals_torch_argmax_and_greedy_pick():
    tab, V, No, _ = tables_for("c3")
    B, _, L = tab["seq_grp"].shape
    R = B * L
    fixed, ocr = scores(R, V, No, None, seed=3)
    ocr = ocr + 1.5                                        # so that a fair share of the maxima sit in the pointer block
    sp = sparse_sample(tab, V + No, 1, key=1, step=0)
    _, _, _, pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], sp["train_loss_mask"].reshape(R), pred=True)
    want = torch.argmax(torch.cat([fixed, ocr], 1), 1)
    assert pred.dtype == torch.int64 and torch.equal(pred, want)
    assert (want >= V).any() and (want < V).any()
    prev = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    ops.greedy_pick(fixed, ocr, prev)
    assert torch.equal(pred.view(B, L)[:, :-1], prev[:, 1:])


@pytest.mark.parametrize("with_grads", [True, False])
def test_ties_resolve_to_the_lowest_index(with_grads):
    """equal maxima inside one 512-column stretch, in two different stretches (what are two column chunks when the row is split), across the V | No
    boundary, and a row of all-equal values"""
    voc, tabs = A.make_answer_tables(2, num_vocab=2000, n_ocr=50, seed=6, max_copy_steps=4)
    tab = on_gpu(A.collate_answer_tables(tabs, A.AnswerTableCaps.for_config(max_copy_steps=4)))
    V, No = len(voc), 50
    B, _, L = tab["seq_grp"].shape
    R = B * L
    assert R == 8
    fixed, ocr = scores(R, V, No, None, seed=4, scale=1.0)
    fixed.clamp_(max=3.0); ocr.clamp_(max=3.0)
    fixed[0, 77] = fixed[0, 300] = 9.0                     # inside one stretch
    fixed[1, 1900] = fixed[1, 130] = 9.0                   # two stretches apart
    fixed[2, 1999] = ocr[2, 0] = 9.0                       # last classifier column and first pointer column
    fixed[3, 5] = ocr[3, 49] = ocr[3, 7] = 9.0             # ... and not adjacent
    fixed[4].fill_(0.25); ocr[4].fill_(0.25)               # all equal: index 0
    ocr[5, 11] = ocr[5, 12] = 9.0                          # a pair inside the pointer block
    fixed[6].fill_(-5.0); ocr[6].fill_(-5.0); ocr[6, 3] = ocr[6, 30] = -1.0
    fixed[7].fill_(float("-inf")); ocr[7].fill_(float("-inf"))      # nothing beats -inf: index 0, as torch.argmax
    want = torch.tensor([77, 130, 1999, 5, 0, V + 11, V + 3, 0], device="cuda")
    assert torch.equal(torch.argmax(torch.cat([fixed, ocr], 1), 1), want)
    for mask in (torch.ones(R, device="cuda"), torch.zeros(R, device="cuda")):      # the unmasked loop and the masked scan
        mask[7] = 0.0                                      # (a row of -inf has no finite loss)
        sp = sparse_sample(tab, V + No, 1, key=2, step=1)
        _, _, _, pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], mask, want_grads=with_grads, pred=True)
        assert torch.equal(pred, want), pred


def test_masked_rows_are_predicted_on_request_and_untouched_and_unread_otherwise():
    tab, V, No, _ = tables_for("odd_stride")
    W = V + No
    B, _, L = tab["seq_grp"].shape
    R = B * L
    fixed, ocr = scores(R, V, No, None, seed=5)
    sp = sparse_sample(tab, W, 1, key=3, step=2)
    mask = sp["train_loss_mask"].reshape(R)
    masked = mask == 0
    assert masked.any() and (~masked).any()
    sentinel = -(1 << 40)
    pred = torch.full((R,), sentinel, dtype=torch.int64, device="cuda")
    loss_a, df_a, do_a, got = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], mask, pred=pred)
    assert got is pred
    assert torch.equal(pred, torch.argmax(torch.cat([fixed, ocr], 1), 1))          # every row, the masked ones too: no sentinel left
    # without pred: NaN in the masked rows' scores reaches nothing (they are not read) -- same loss, same gradients, zero in the masked rows
    fixed_p, ocr_p = fixed.clone(), ocr.clone()
    fixed_p[masked] = float("nan"); ocr_p[masked] = float("nan")
    loss_b, df_b, do_b, none = ops.bce_loss_table(fixed_p, ocr_p, tab, sp["answer_choice"], mask)
    assert none is None
    assert torch.isfinite(loss_b).all() and rel(loss_b.item(), loss_a.item()) <= 1e-6
    assert torch.equal(df_b.view(torch.int16), df_a.view(torch.int16)) and torch.equal(do_b, do_a)
    assert not df_b[masked].any() and not do_b[masked].any()


# ---------------------------------------------------------------------------------------------- 6. degenerate and hostile tables
def test_no_candidates_equals_all_zero_targets():
    tab, V, No, _ = tables_for("odd_stride")
    W = V + No
    B, _, L = tab["seq_grp"].shape
    R = B * L
    tab = dict(tab, meta=tab["meta"].clone())
    tab["meta"][:, 0] = 0                                  # n_seq = 0 everywhere
    fixed, ocr = scores(R, V, No, None, seed=6)
    sp = sparse_sample(tab, W, 1, key=4, step=0)
    assert (sp["answer_choice"] == -1).all() and not sp["train_loss_mask"].any()
    mask = torch.ones(R, device="cuda")                    # (the sampler's mask would hide every row: the all-zero rows are checked unmasked)
    zeros = torch.zeros(R, W, device="cuda")
    loss_d, df_d, do_d = ops.bce_loss(fixed, ocr, zeros, mask)
    loss_t, df_t, do_t, _ = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], mask)
    assert torch.equal(df_t.view(torch.int16), df_d.view(torch.int16)) and torch.equal(do_t, do_d)
    assert rel(loss_t.item(), loss_d.item()) <= 1e-6
    loss_m, df_m, do_m, _ = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], sp["train_loss_mask"].reshape(R))
    assert loss_m.item() == 0.0 and not df_m.any() and not do_m.any()


def test_a_table_of_bad_data_matches_the_dense_path_fed_the_same_table():
    """parity on out-of-range DATA (counts, offsets, indices, group ids, lengths): the dense sampler's clamps are the specification, and both paths complete
    normally.  (Step-0 lists keep their indices distinct: one index listed with two values is a race in the dense sampler itself.)"""
    meta, _ = golden()
    voc, _, table = case_tables(meta)
    V, No = len(voc), meta["max_ocr_tokens"]
    W = V + No
    B, S, L = table["seq_grp"].shape
    G, E = table["grp_idx"].shape[1], table["grp_extra"].shape[1]
    rng = np.random.RandomState(12)
    t = {k: v.clone() for k, v in table.items()}
    big = 2 ** 31 - 1
    t["meta"][:, 1] = torch.from_numpy(rng.choice([-3, 0, 2, S, S + 9, big], B))                 # n_step0
    t["meta"][:, 2] = torch.from_numpy(rng.choice([-1, 1, 3, G, G + 5, big], B))                 # n_grp
    t["meta"][:, 3] = torch.from_numpy(rng.choice([-7, 0, 4, E, E + 1, big], B))                 # n_extra
    t["meta"][0, 0], t["meta"][1, 0] = S + 50, -2                                                # n_seq over the capacity / negative
    bad = lambda shape, p: torch.from_numpy(rng.rand(*shape) < p)
    pick = lambda shape, vals: torch.from_numpy(rng.choice(vals, shape))
    m = bad((B, S), 0.3)
    t["step0_idx"][m] = pick((B, S), [-1, -big, W, W + 1, big])[m].to(torch.int32)               # (out of range only: in-range entries stay distinct)
    m = bad((B, G + 1), 0.4)
    t["grp_off"][m] = pick((B, G + 1), [-5, 0, 3, E - 1, E, E + 2, big, -big])[m].to(torch.int32)
    m = bad((B, E), 0.3)
    t["grp_extra"][m] = pick((B, E), [-1, W, W + 7, big, -big, 0, W - 1])[m].to(torch.int32)
    m = bad((B, S, L), 0.3)
    t["seq_grp"][m] = pick((B, S, L), [-1, -32768, G, G + 1, 32767, 0])[m].to(torch.int16)
    m = bad((B, S), 0.3)
    t["seq_len"][m] = pick((B, S), [-4, 0, L, L + 1, big])[m].to(torch.int32)
    tab = on_gpu(t)
    R = B * L
    fixed, ocr = scores(R, V, No, None, seed=7)
    for rnd in range(4):
        force = rng.choice([-1, 0, 1, 2, 5, S - 1, S, S + 3], B)
        dense, loss_d, df_d, do_d = dense_route(tab, W, 1, fixed, ocr, force=force)
        sp = sparse_sample(tab, W, 1, force=force)
        for k in SPARSE_KEYS:
            assert torch.equal(sp[k], dense[k]), k
        loss_t, df_t, do_t, pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], sp["train_loss_mask"].reshape(R), pred=True)
        assert torch.equal(df_t.view(torch.int16), df_d.view(torch.int16)) and torch.equal(do_t, do_d), rnd
        assert rel(loss_t.item(), loss_d.item()) <= 1e-6 or (loss_d.item() == 0.0 and loss_t.item() == 0.0)
        assert torch.equal(pred, torch.argmax(torch.cat([fixed, ocr], 1), 1))
        # every row unmasked, a choice the sampler never wrote (out of range counts as no sequence)
        ones = torch.ones(R, device="cuda")
        raw = torch.as_tensor(force, dtype=torch.int32, device="cuda")
        loss_d, df_d, do_d = ops.bce_loss(fixed, ocr, dense["targets"].reshape(R, W), ones)
        loss_t, df_t, do_t, _ = ops.bce_loss_table(fixed, ocr, tab, raw, ones)
        assert torch.equal(df_t.view(torch.int16), df_d.view(torch.int16)) and torch.equal(do_t, do_d), rnd
        assert rel(loss_t.item(), loss_d.item()) <= 1e-6
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. loss-only call, guard regions
def test_loss_only_call_gives_the_same_loss_and_pred_and_stores_nothing_else():
    tab, V, No, _ = tables_for("odd_stride")
    W = V + No
    B, S, L = tab["seq_grp"].shape
    G, E = tab["grp_idx"].shape[1], tab["grp_extra"].shape[1]
    R = B * L
    fixed, ocr = scores(R, V, No, None, seed=8)
    sp = sparse_sample(tab, W, 1, key=6, step=4)
    mask = sp["train_loss_mask"].reshape(R).contiguous()
    nan = float("nan")
    PAD, SENT = 6, -(1 << 50)

    def buffers():
        return (torch.full((3,), nan, device="cuda"), torch.full((R + 2, V + PAD), nan, dtype=torch.bfloat16, device="cuda"),
                torch.full((R + 2, No + PAD), nan, device="cuda"), torch.full((R + 16,), SENT, dtype=torch.int64, device="cuda"))

    def call(loss, dfix, docr, pred, grads, want_pred):
        capi.call("sam_bce_loss_table", capi.ptr(fixed), fixed.stride(0), capi.ptr(ocr), ocr.stride(0), *[capi.ptr(tab[k]) for k in ops.ANSWER_TABLE_KEYS], B, S, L, G, E,
                  capi.ptr(sp["answer_choice"]), capi.ptr(mask), R, V, No, 1.0, None, capi.ptr(loss[1:]), capi.ptr(dfix[1:]) if grads else None, dfix.stride(0),
                  capi.ptr(docr[1:]) if grads else None, docr.stride(0), capi.ptr(pred[8:]) if want_pred else None, capi.stream_handle())
        torch.cuda.synchronize()

    full = buffers()
    call(*full, grads=True, want_pred=True)
    loss, dfix, docr, pred = full
    ref_loss, ref_df, ref_do, ref_pred = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], mask, pred=True)
    assert torch.isnan(loss[0]) and torch.isnan(loss[2]) and rel(loss[1].item(), ref_loss.item()) <= 1e-6
    assert torch.equal(dfix[1:R + 1, :V].view(torch.int16), ref_df.view(torch.int16)) and torch.equal(docr[1:R + 1, :No], ref_do)
    assert torch.isnan(dfix[0]).all() and torch.isnan(dfix[R + 1]).all() and torch.isnan(dfix[:, V:]).all()
    assert torch.isnan(docr[0]).all() and torch.isnan(docr[R + 1]).all() and torch.isnan(docr[:, No:]).all()
    assert torch.equal(pred[8:8 + R], ref_pred) and (pred[:8] == SENT).all() and (pred[8 + R:] == SENT).all()

    for want_pred in (True, False):
        only = buffers()
        call(*only, grads=False, want_pred=want_pred)
        loss_o, dfix_o, docr_o, pred_o = only
        assert torch.isnan(loss_o[0]) and torch.isnan(loss_o[2]) and rel(loss_o[1].item(), ref_loss.item()) <= 1e-6
        assert torch.isnan(dfix_o).all() and torch.isnan(docr_o).all()                    # nothing stored into either gradient block
        assert (pred_o[:8] == SENT).all() and (pred_o[8 + R:] == SENT).all()
        if want_pred:
            assert torch.equal(pred_o[8:8 + R], ref_pred)
        else:
            assert (pred_o == SENT).all()
    # the public route of the same call
    loss_p, none_f, none_o, pred_p = ops.bce_loss_table(fixed, ocr, tab, sp["answer_choice"], mask, want_grads=False, pred=True)
    assert none_f is None and none_o is None and torch.equal(pred_p, ref_pred) and rel(loss_p.item(), ref_loss.item()) <= 1e-6


def test_rows_wider_than_the_lds_budget_are_refused():
    tab, V, No, _ = tables_for("odd_stride")
    B, _, L = tab["seq_grp"].shape
    R = B * L
    fixed = torch.zeros(R, 16000, device="cuda")
    ocr = torch.zeros(R, 2, device="cuda")
    with pytest.raises((capi.SamHipError, RuntimeError), match="LDS"):
        ops.bce_loss_table(fixed, ocr, tab, torch.zeros(B, dtype=torch.int32, device="cuda"), torch.ones(R, device="cuda"))


# ---------------------------------------------------------------------------------------------- 8. / 9. Trainer
MODES = dict(eager=dict(use_graph=False), graph=dict(use_graph=True, pipeline_update=False), graph_pipelined=dict(use_graph=True, pipeline_update=True))


@pytest.mark.parametrize("mode", ["eager", "graph", "graph_pipelined"])
def test_trainer_in_table_mode_equals_the_dense_table_trainer(mode):
    from sam_textvqa_amd.autograd import dropout_clock
    from sam_textvqa_amd.trainer import Trainer
    kw = MODES[mode]
    bd, table = batches()
    n = table["meta"][:, 0].numpy()
    runs = {}
    for name, extra in (("table", dict(answer_targets="table")), ("dense", {})):
        # one after the other: the dropout clock is process-wide, and each Trainer re-seeds it
        tr = Trainer(small_model(), seed=7, **kw, **extra)
        losses = []
        for step in range(4):
            losses.append(tr.step(with_inputs(bd, answer_table=table)).item())
            got = tr.sampled_answers()
            np.testing.assert_array_equal(got["answer_choice"].cpu().numpy(), A.draw_choices(A.answer_key(7, 0), step, n))
            assert ("targets" in got) == (name == "dense")
            if name == "table":
                twin = A.sample_answers_torch({k: v.cuda() for k, v in table.items()}, got["answer_choice"])
                for k in SPARSE_KEYS:
                    assert torch.equal(got[k], twin[k]), k
        tr.flush_update()
        torch.cuda.synchronize()
        if mode != "eager":
            assert tr._graph is not None
        assert tr.predictions() is None
        runs[name] = (losses, tr.flat.flat.clone(), dropout_clock.offset)
    (lt, pt, ot), (ld, pd, od) = runs["table"], runs["dense"]
    for step, (a, b) in enumerate(zip(lt, ld)):
        print("%s step %d: loss table %.9g dense %.9g" % (mode, step, a, b))
        assert abs(a - b) <= 1e-6 * abs(b), (mode, step, a, b)
    # (not bit for bit: two fresh Trainers agree to a few fp32 ulps only, see test_trainer_with_answer_table_equals_trainer_fed_the_dense_draws)
    assert (pt - pd).abs().max().item() < 1e-5
    assert ot == od


def test_a_table_step_launches_the_table_loss_once_and_never_the_dense_one():
    from sam_textvqa_amd.autograd import dropout_clock
    from sam_textvqa_amd.trainer import Trainer
    bd, table = batches()
    calls, offsets = {}, {}
    for name, extra in (("dense", {}), ("table", dict(answer_targets="table"))):
        tr = Trainer(small_model(), seed=7, use_graph=False, **extra)
        capi.profiler = []
        try:
            tr.step(with_inputs(bd, answer_table=table))
            torch.cuda.synchronize()
            calls[name] = [c[0] for c in capi.profiler]
        finally:
            capi.profiler = None
        offsets[name] = dropout_clock.offset
    assert calls["table"].count("sam_bce_loss_table") == 1 and "sam_bce_loss" not in calls["table"]
    assert calls["dense"].count("sam_bce_loss") == 1 and "sam_bce_loss_table" not in calls["dense"]
    assert calls["table"][0] == "sam_answer_sample"
    assert [("sam_bce_loss" if c == "sam_bce_loss_table" else c) for c in calls["table"]] == calls["dense"]      # one node swapped, nothing added
    assert offsets["dense"] == offsets["table"]
    dense = A.sample_answers_torch({k: v.cuda() for k, v in table.items()}, torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="both"):
        Trainer(small_model(), seed=7, answer_targets="table").step(with_inputs(bd, answer_table=table, targets=dense["targets"]))
    with pytest.raises(ValueError, match="answer_table"):
        Trainer(small_model(), seed=7, answer_targets="table").step(
            with_inputs(bd, targets=dense["targets"], train_prev_inds=dense["train_prev_inds"], train_loss_mask=dense["train_loss_mask"]))


def test_trainer_predictions_equal_the_argmax_of_the_steps_own_scores():
    """eager: a forward hook keeps the two score blocks the step's model call produced; predictions() must be their argmax exactly (the small random
    model has no greedy ties), on every row, the masked ones included"""
    from sam_textvqa_amd.trainer import Trainer
    bd, table = batches()
    model = small_model()
    tr = Trainer(model, seed=7, use_graph=False, answer_targets="table", predictions=True)
    assert tr.predictions() is None
    kept = []
    hook = model.register_forward_hook(lambda mod, args, out: kept.append((args[0]["fixed_scores"].detach().clone(), args[0]["dynamic_ocr_scores"].detach().clone())))
    seen = []
    try:
        for step in range(3):
            tr.step(with_inputs(bd, answer_table=table))
            pred = tr.predictions()
            fixed, ocr = kept[-1]
            B, L = pred.shape
            assert pred.dtype == torch.int64 and (B, L) == tuple(fixed.shape[:2])
            want = torch.argmax(torch.cat([fixed.float(), ocr.float()], -1), -1)
            assert torch.equal(pred, want), step
            assert (tr.sampled_answers()["train_loss_mask"] == 0).any()
            seen.append(pred.clone())
    finally:
        hook.remove()
    assert tr.predictions() is tr.predictions() and tr.predictions().data_ptr() != seen[-1].data_ptr()      # the Trainer's own resident buffer
    words = A.decode_predictions(seen[-1], A.make_answer_tables(1, num_vocab=200, n_ocr=50, seed=5)[0], [["tok%d" % i for i in range(50)]] * seen[-1].shape[0])
    assert len(words) == seen[-1].shape[0] and all(isinstance(w[0], str) for w in words)


@pytest.mark.parametrize("mode", ["graph", "graph_pipelined"])
def test_trainer_predictions_are_rewritten_by_every_replay(mode):
    from sam_textvqa_amd.trainer import Trainer
    bd, table = batches(B=8)
    tr = Trainer(small_model(), seed=3, base_lr=1e-3, answer_targets="table", predictions=True, **MODES[mode])
    tr.step(with_inputs(bd, answer_table=table))
    tr.step(with_inputs(bd, answer_table=table))
    assert tr._graph is not None
    buf = tr.predictions()
    seen = []
    for step in range(2, 8):
        tr.step(with_inputs(bd, answer_table=table))
        assert tr.predictions() is buf                       # resident: every replay overwrites the same tensor
        p = buf.clone()
        assert ((p >= 0) & (p < 250)).all()
        seen.append(p)
    assert any(not torch.equal(a, b) for a, b in zip(seen[:-1], seen[1:]))


# ---------------------------------------------------------------------------------------------- 10. data parallel, one rank
_DIST_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, os.environ["SAM_REPO"])
from tests.test_answers_gpu import batches, small_model, with_inputs
from sam_textvqa_amd import _capi as capi
from sam_textvqa_amd import parallel
from sam_textvqa_amd.trainer import Trainer
os.environ["SAM_FORCE_DIST"] = "1"
parallel.init_distributed()                               # 1-rank RCCL group: the count all-reduce really goes through RCCL
bd, table = batches()
res = []
for dist_on in (True, False):
    os.environ["SAM_FORCE_DIST"] = "1" if dist_on else "0"
    tr = Trainer(small_model(), base_lr=1e-3, seed=3, answer_targets="table", predictions=True)
    assert (tr.reducer is not None) == dist_on
    losses = [tr.step(with_inputs(bd, answer_table=table)).item() for _ in range(4)]
    assert "targets" not in tr.sampled_answers() and tr.predictions() is not None
    tr.flush_update()
    res.append((losses, tr.flat.flat.clone()))
torch.cuda.synchronize()
(l1, p1), (l0, p0) = res
print("LOSSES", l1, l0)
assert all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(l1, l0)), (l1, l0)
d = (p1 - p0).abs().max().item()
print("MAXDIFF", d)
assert d < 5e-3, d
print("TABLE_DIST_OK")
"""


def test_one_rank_data_parallel_table_step_matches_the_plain_trainer():
    """SAM_FORCE_DIST=1: the loss node of a "table" step takes the all-reduced count (global_count) and trains like the reducer-less path, within the
    bounds of tests/test_model_gpu.py::test_rccl_path_one_rank_matches_plain_trainer"""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAM_REPO=root, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from tests.util import run_child
    run_child([sys.executable, "-c", _DIST_SCRIPT], env, "TABLE_DIST_OK", "bce_table_one_rank")
