"""GPU: M4C answer targets sampled on the MI355X (csrc/answers.hip, sam_answer_sample) -- forced draws bit-identical to the reference golden at every
row stride, free draws equal to the host twin, reproducible and uniform, the Trainer's first node (eager, graph replay, pipelined graph) writing exactly
the twin's tensors and training like
a Trainer fed the dense targets of the same draws (to fp32 ulps), fresh draws on every replay, and nothing launched or drawn for a batch without an answer table."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi as capi
from sam_textvqa_amd import answers as A
from sam_textvqa_amd import ops
from tests.test_answers_cpu import case_tables, dense_record, golden, records_by_round

pytestmark = pytest.mark.gpu

KEYS_OUT = ("targets", "train_prev_inds", "train_loss_mask", "train_acc_mask", "answer_choice")


def on_gpu(table):
    return {k: v.cuda() for k, v in table.items()}


def sample(table, W, bos, key=0, step=0, force=None, ld=None, step_dev=None):
    B, _, L = table["seq_grp"].shape
    out = ops.answer_outputs(B, L, W, "cuda", ld=ld)
    if ld is not None and ld > W:
        out["targets"].as_strided((B, L, ld), (L * ld, ld, 1)).fill_(float("nan"))      # the padding columns must stay untouched
    fc = None if force is None else torch.as_tensor(force, dtype=torch.int32, device="cuda")
    ops.answer_sample(table, W, bos, key, step=step, step_dev=step_dev, force_choice=fc, out=out)
    return out


@pytest.mark.parametrize("pad", [0, 2, 3])
def test_forced_draws_match_the_reference_golden_bitwise(pad):
    meta, g = golden()
    _, _, table = case_tables(meta)
    W, L = meta["W"], meta["max_copy_steps"]
    tab = on_gpu(table)
    bos = int(table["dims"][1])
    for choice, recs in records_by_round(g):
        out = sample(tab, W, bos, force=choice, ld=W + pad)
        tg = out["targets"].cpu()
        for c, r in recs.items():
            np.testing.assert_array_equal(tg[c].numpy(), dense_record(g, r, L, W), err_msg="case %s k %d" % (meta["cases"][c]["name"], choice[c]))
            np.testing.assert_array_equal(out["train_prev_inds"][c].cpu().numpy(), g["prev"][r])
            np.testing.assert_array_equal(out["train_loss_mask"][c].cpu().numpy(), g["loss_mask"][r])
            np.testing.assert_array_equal(out["train_acc_mask"][c].cpu().numpy(), g["acc_mask"][r])
        np.testing.assert_array_equal(out["answer_choice"].cpu().numpy(), choice)
        if pad:
            full = out["targets"].as_strided((len(choice), L, W + pad), (L * (W + pad), W + pad, 1))
            assert torch.isnan(full[:, :, W:]).all()


def test_full_size_forced_and_free_draws_match_the_torch_twin():
    """c3 width (5000-word vocabulary + 50 OCR slots), B = 64: the vector-store path of the kernel against the torch twin, forced and free"""
    _, tabs = A.make_answer_tables(64, seed=3)
    table = A.collate_answer_tables(tabs)
    tab = on_gpu(table)
    W, bos = A.table_dims(table)
    n = table["meta"][:, 0].numpy()
    for step in (0, 7):
        out = sample(tab, W, bos, key=A.answer_key(9, 0), step=step)
        want = A.draw_choices(A.answer_key(9, 0), step, n)
        np.testing.assert_array_equal(out["answer_choice"].cpu().numpy(), want)
        twin = A.sample_answers_torch(tab, torch.from_numpy(want).cuda())
        for k in KEYS_OUT:
            assert torch.equal(out[k], twin[k]), k
    rng = np.random.RandomState(0)
    force = np.where(n > 0, (rng.rand(len(n)) * np.maximum(n, 1)).astype(np.int64), -1)
    out = sample(tab, W, bos, force=force)
    twin = A.sample_answers_torch(tab, torch.from_numpy(force).cuda())
    for k in KEYS_OUT:
        assert torch.equal(out[k], twin[k]), k


def test_free_draws_are_reproducible_and_read_the_step_from_device_memory():
    meta, _ = golden()
    _, _, table = case_tables(meta)
    tab = on_gpu(table)
    W, bos = A.table_dims(table)
    key = A.answer_key(123, 1)
    a = sample(tab, W, bos, key=key, step=41)
    b = sample(tab, W, bos, key=key, step=41)
    for k in KEYS_OUT:
        assert torch.equal(a[k], b[k]), k
    np.testing.assert_array_equal(a["answer_choice"].cpu().numpy(), A.draw_choices(key, 41, table["meta"][:, 0].numpy()))
    c = sample(tab, W, bos, key=key, step=1, step_dev=torch.tensor([40], dtype=torch.int64, device="cuda"))
    for k in KEYS_OUT:
        assert torch.equal(a[k], c[k]), k
    no = [i for i, cs in enumerate(meta["cases"]) if cs["name"] == "no_match"][0]
    for k in KEYS_OUT[:4]:
        assert not a[k][no].any(), k
    assert int(a["answer_choice"][no]) == -1


def test_free_draws_are_uniform_over_20000_steps():
    """per-candidate frequencies of every sample over 20 000 steps with fixed seeds: chi-square bound at p = 0.001 (deterministic, never flaky)"""
    meta, g = golden()
    _, _, table = case_tables(meta)
    tab = on_gpu(table)
    W, bos = A.table_dims(table)
    B, L = tab["seq_grp"].shape[0], tab["seq_grp"].shape[2]
    out = ops.answer_outputs(B, L, W, "cuda")
    got = []
    for st in range(20000):
        ops.answer_sample(tab, W, bos, A.answer_key(2024), step=st, out=out)
        got.append(out["answer_choice"].clone())
    ch = torch.stack(got).cpu().numpy()
    n = table["meta"][:, 0].numpy()
    crit = {9: 27.88, 13: 34.53, 16: 39.25, 29: 58.30, 31: 61.10, 55: 93.17, 71: 113.58, 4: 18.47, 6: 22.46, 2: 13.82, 1: 10.83}
    for b in range(B):
        if n[b] == 0:
            assert (ch[:, b] == -1).all()
            continue
        assert ((ch[:, b] >= 0) & (ch[:, b] < n[b])).all()
        if n[b] == 1:
            continue
        cnt = np.bincount(ch[:, b], minlength=n[b])
        e = 20000 / n[b]
        chi2 = (((cnt - e) ** 2) / e).sum()
        df = n[b] - 1
        bound = crit[df]                                                             # chi2.ppf(0.999, df)
        assert chi2 < bound, (meta["cases"][b]["name"], n[b], chi2, bound)
    want = np.stack([A.draw_choices(A.answer_key(2024), st, n) for st in range(0, 20000, 997)])
    np.testing.assert_array_equal(ch[::997], want)


# ---------------------------------------------------------------------------------------------- Trainer
def small_model():
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    torch.manual_seed(0)
    mcfg = M.BertConfig.from_dict(mmt_config_dict(3, ("n", "s")))
    tcfg = M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1))
    return M.SAM4C(mcfg, tcfg, num_answers=200, bos_idx=1)


def batches(B=4):
    """a synthetic batch without its answer half, plus the collated answer table of B samples at the model's width (200 words + 50 OCR slots)"""
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=200, device="cuda", seed=3)
    for k in ("targets", "train_prev_inds", "train_loss_mask"):
        del bd[k]
    _, tabs = A.make_answer_tables(B, num_vocab=200, n_ocr=50, seed=5)
    return bd, A.collate_answer_tables(tabs)


def with_inputs(bd, **extra):
    from sam_textvqa_amd.synthetic import clone_batch
    out = clone_batch(bd)
    out.update(extra)
    return out


@pytest.mark.parametrize("mode", ["eager", "graph", "graph_pipelined"])
def test_trainer_with_answer_table_equals_trainer_fed_the_dense_draws(mode):
    from sam_textvqa_amd.trainer import Trainer
    kw = dict(eager=dict(use_graph=False), graph=dict(use_graph=True, pipeline_update=False), graph_pipelined=dict(use_graph=True, pipeline_update=True))[mode]
    bd, table = batches()
    n = table["meta"][:, 0].numpy()
    # one after the other: the dropout clock is process-wide, and each Trainer re-seeds it, so B replays A's dropout stream exactly
    ta = Trainer(small_model(), seed=7, **kw)
    losses, seen, dense_steps = [], [], []
    for step in range(4):
        losses.append(ta.step(with_inputs(bd, answer_table=table)))
        got = ta.sampled_answers()
        ch = got["answer_choice"].clone()
        np.testing.assert_array_equal(ch.cpu().numpy(), A.draw_choices(A.answer_key(7, 0), step, n))       # every replay draws afresh, as the twin says
        dense = A.sample_answers_torch({k: v.cuda() for k, v in table.items()}, ch)
        for k in KEYS_OUT:
            assert torch.equal(got[k], dense[k]), k
        dense_steps.append(dense)
        seen.append(ch.cpu().numpy())
    ta.flush_update()
    tb = Trainer(small_model(), seed=7, **kw)
    for step, dense in enumerate(dense_steps):
        lb = tb.step(with_inputs(bd, targets=dense["targets"], train_prev_inds=dense["train_prev_inds"], train_loss_mask=dense["train_loss_mask"]))
        la_, lb_ = losses[step].item(), lb.item()
        assert abs(la_ - lb_) <= 1e-6 * abs(la_), (mode, step, la_, lb_)
    tb.flush_update()
    torch.cuda.synchronize()
    # not bit for bit: two fresh Trainers on the same inputs agree to a few fp32 ulps only (the single-process word-embedding scatter adds with atomics,
    # and a fresh Trainer's first step is not bit-identical to a running one's: tests/test_model_gpu.py's resume test, test_fc7_encoder_gpu.py)
    assert (ta.flat.flat - tb.flat.flat).abs().max().item() < 1e-5
    multi = n > 1
    assert any((seen[i][multi] != seen[i + 1][multi]).any() for i in range(len(seen) - 1))
    if mode != "eager":
        assert ta._graph is not None and tb._graph is not None


def test_graph_replays_resample_every_step():
    from sam_textvqa_amd.trainer import Trainer
    bd, table = batches(B=8)
    n = table["meta"][:, 0].numpy()
    tr = Trainer(small_model(), seed=3, use_graph=True)
    tr.step(with_inputs(bd, answer_table=table))
    tr.step(with_inputs(bd, answer_table=table))
    assert tr._graph is not None
    prev = None
    for step in range(2, 8):
        tr.step(with_inputs(bd, answer_table=table))
        ch = tr.sampled_answers()["answer_choice"].cpu().numpy()
        np.testing.assert_array_equal(ch, A.draw_choices(A.answer_key(3, 0), step, n))
        if prev is not None:
            assert (ch[n > 1] != prev[n > 1]).any()
        prev = ch


def test_a_batch_without_answer_table_launches_and_draws_nothing_extra():
    from sam_textvqa_amd.autograd import dropout_clock
    from sam_textvqa_amd.synthetic import make_batch
    from sam_textvqa_amd.trainer import Trainer
    bd, table = batches()
    dense = A.sample_answers_torch({k: v.cuda() for k, v in table.items()}, torch.zeros(4, dtype=torch.int32, device="cuda"))
    dense_bd = with_inputs(bd, targets=dense["targets"], train_prev_inds=dense["train_prev_inds"], train_loss_mask=dense["train_loss_mask"])
    calls, offsets = {}, {}
    for name, batch in (("dense", dense_bd), ("table", with_inputs(bd, answer_table=table))):
        tr = Trainer(small_model(), seed=7, use_graph=False)
        capi.profiler = []
        try:
            tr.step(batch)
            torch.cuda.synchronize()
            calls[name] = [c[0] for c in capi.profiler]
        finally:
            capi.profiler = None
        offsets[name] = dropout_clock.offset
        if name == "dense":
            assert tr.sampled_answers() is None and tr._answer_out is None
    assert "sam_answer_sample" not in calls["dense"]
    assert calls["table"].count("sam_answer_sample") == 1 and calls["table"][0] == "sam_answer_sample"
    assert [c for c in calls["table"] if c != "sam_answer_sample"] == calls["dense"]
    assert offsets["dense"] == offsets["table"]
    with pytest.raises(ValueError, match="both"):
        Trainer(small_model(), seed=7).step(with_inputs(bd, answer_table=table, targets=dense["targets"]))


def test_public_sample_answers_fills_the_batch_dict():
    bd, table = batches()
    d = {"answer_table": table}
    out = A.sample_answers(d, step=5, seed=7)
    for k in KEYS_OUT:
        assert d[k] is out[k]
    np.testing.assert_array_equal(out["answer_choice"].cpu().numpy(), A.draw_choices(A.answer_key(7, 0), 5, table["meta"][:, 0].numpy()))
    d2 = {"answer_table": table}
    A.sample_answers(d2, step=0, seed=0, choice=out["answer_choice"].cpu())
    for k in KEYS_OUT:
        assert torch.equal(d2[k], out[k]), k
