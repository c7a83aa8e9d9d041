"""GPU: the metrics' score tables from text (csrc/score_text.hip, sam_score_table_from_text) against the host twin
metrics.score_tables_from_text_host, bit for bit on all eight tensors and on status -- the twin itself is held against collate_score_tables of
build_score_table by tests/test_score_text_cpu.py, on the same batches.  Then the contract around the launch: row strides, poisoned outputs between guard
rows, repeated launches, the status sample, both op routes, and the table's two consumers (score_predictions against the reference's recorded scores,
Trainer(metric=...))."""
import numpy as np
import pytest
import torch

from sam_textvqa_amd import _capi as capi
from sam_textvqa_amd import metrics as M
from sam_textvqa_amd import ops
from tests.test_metrics_cpu import check_scores, golden  # noqa: F401
from tests.test_score_text_cpu import GOLDEN_CAPS, SHAPES, assert_same_table, corner_batch, golden_text, pack, status_batch

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A


def on_gpu(bd):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in bd.items()}


def assert_equals_twin(bd, caps, what=""):
    want, wst = M.score_tables_from_text_host(bd, caps)
    got, st = M.score_tables_from_text(on_gpu(bd), caps, check=False)
    assert torch.equal(st.cpu(), wst), (what, st.tolist(), wst.tolist())
    assert_same_table(got, want, what)
    return got, want


def test_kernel_equals_the_twin_on_the_golden_cases_as_one_batch():
    g, answers, tokens = golden_text()
    assert_equals_twin(pack(answers, tokens, GOLDEN_CAPS, n_ocr=g["max_ocr_tokens"]), GOLDEN_CAPS, "golden")


def test_kernel_equals_the_twin_on_the_rich_synthetic_batch():
    voc, answers, tokens = M.make_score_text(8, rich=True)
    got, want = assert_equals_twin(pack(answers, tokens), M.DEFAULT_SCORE_CAPS, "rich")
    assert_same_table(got, M.collate_score_tables(M.make_score_tables(8, rich=True)[2]), "rich, host-built")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-A%d-La%d-No%d-Lw%d-Lg%d" % s[:6])
def test_kernel_equals_the_twin_on_the_corner_shapes(shape):
    caps, answers, tokens, bd = corner_batch(*shape)
    assert_equals_twin(bd, caps, str(shape))


def test_row_strides_larger_than_the_width():
    """ld_answer = La + 3 and ld_ocr = Lw + 5, the columns behind the width poisoned: the ctypes route, which takes the strides as they are"""
    shape = SHAPES[2]
    B, A_, La, No, Lw, Lg, counts = shape
    caps, answers, tokens, bd = corner_batch(*shape)
    want, wst = M.score_tables_from_text_host(bd, caps)
    at = torch.full((B, A_, La + 3), POISON, dtype=torch.int32)
    at[:, :, :La] = bd["answer_text"]
    ot = torch.full((B, No, Lw + 5), POISON, dtype=torch.int32)
    ot[:, :, :Lw] = bd["ocr_text"]
    at, ot, al, ol, cnt = at.cuda(), ot.cuda(), bd["answer_text_len"].cuda(), bd["ocr_text_len"].cuda(), bd["ocr_count"].cuda()
    out = M.score_table_outputs(B, No, caps, "cuda")
    capi.call("sam_score_table_from_text", capi.ptr(at), La + 3, capi.ptr(al), capi.ptr(ot), Lw + 5, capi.ptr(ol), capi.ptr(cnt), B, A_, La, No, Lw, Lg,
              *[capi.ptr(out[k]) for k in M.SCORE_TABLE_KEYS], capi.ptr(out["status"]), capi.stream_handle())
    assert torch.equal(out["status"].cpu(), wst)
    assert_same_table(out, want, "strided")


def test_every_output_element_is_written_the_guards_are_not_and_a_second_launch_agrees():
    voc, answers, tokens = M.make_score_text(8, rich=True)
    bd = pack(answers, tokens)
    want, wst = M.score_tables_from_text_host(bd)
    gbd = on_gpu(bd)
    fresh = M.score_table_outputs(8, 50, M.DEFAULT_SCORE_CAPS, "cuda")
    bufs, out = {}, {}
    for k, t in fresh.items():          # one guard row of the same shape in front of and behind every output
        bufs[k] = torch.full((10,) + tuple(t.shape[1:]), POISON, dtype=torch.int32, device="cuda").view(t.dtype)
        out[k] = bufs[k][1:9]
        assert out[k].is_contiguous() and out[k].shape == t.shape
    runs = []
    for _ in range(2):
        table, st = M.score_tables_from_text(gbd, out=out, check=False)
        assert all(table[k].data_ptr() == out[k].data_ptr() for k in M.SCORE_TABLE_KEYS)
        runs.append({k: v.clone() for k, v in out.items()})
        assert torch.equal(st.cpu(), wst)
        assert_same_table(table, want, "poisoned")          # the twin holds no poison: every element inside was overwritten
        for k, v in bufs.items():
            guards = torch.cat([v[:1].reshape(-1), v[9:].reshape(-1)]).view(torch.int32)
            assert bool((guards == POISON).all()), k
            assert not bool((out[k].reshape(-1).view(torch.int32) == POISON).any()), k
        for k in out:
            out[k].view(torch.int32).fill_(POISON)
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k


def test_the_status_sample_between_clean_neighbours():
    answers, tokens, bd = status_batch()
    got, want = assert_equals_twin(bd, M.DEFAULT_SCORE_CAPS, "status")
    table, st = M.score_tables_from_text(on_gpu(bd), check=False)
    assert st.is_cuda and st.tolist() == [0, M.STATUS_LG, 0]
    for k in M.SCORE_TABLE_KEYS:
        assert not table[k][1].any() and table[k][0].any(), k
    with pytest.raises(ValueError, match="sample 1.*Lg = 128"):
        M.score_tables_from_text(on_gpu(bd))


def test_counts_come_from_the_mask_rows_when_the_batch_is_not_ragged():
    voc, answers, tokens = M.make_score_text(4, num_vocab=200, seed=5)
    bd = pack(answers, tokens)
    want, _ = M.score_tables_from_text_host(bd)
    cnt = bd.pop("ocr_count")
    with pytest.raises(ValueError, match="ocr_count"):
        M.score_tables_from_text(on_gpu(bd))
    bd["pad_ocr_mask"] = (torch.arange(50)[None, :] < cnt[:, None]).long()
    assert_same_table(M.score_tables_from_text(on_gpu(bd)), want, "mask rows")


def test_both_op_routes_agree(monkeypatch):
    caps, answers, tokens, bd = corner_batch(*SHAPES[5])
    gbd, out = on_gpu(bd), {}
    for route in ("1", "0"):
        monkeypatch.setenv("SAM_COARSE_OPS", route)
        table, st = M.score_tables_from_text(gbd, caps, check=False)
        out[route] = dict(table, status=st)
    raw = M.score_table_outputs(3, 50, caps, "cuda")
    torch.ops.sam_hip.score_table_from_text(gbd["answer_text"], gbd["answer_text_len"], gbd["ocr_text"], gbd["ocr_text_len"], gbd["ocr_count"],
                                            [raw[k] for k in M.SCORE_TABLE_KEYS] + [raw["status"]])
    for k in out["1"]:
        assert torch.equal(out["1"][k].view(torch.int32), out["0"][k].view(torch.int32)), k
        assert torch.equal(out["1"][k].view(torch.int32), raw[k].view(torch.int32)), k
    with pytest.raises(capi.SamHipError, match="at most 64"):
        ops.score_table_from_text(torch.zeros((1, 65, 4), dtype=torch.int32, device="cuda"), torch.zeros((1, 65), dtype=torch.int32, device="cuda"),
                                  gbd["ocr_text"][:1], gbd["ocr_text_len"][:1], gbd["ocr_count"][:1], M.score_table_outputs(1, 50, M.ScoreTableCaps(65, 32, 8), "cuda"))


def test_score_predictions_on_the_device_built_table_gives_the_references_scores(golden):
    g, answers, tokens = golden_text()
    bd = on_gpu(pack(answers, tokens, GOLDEN_CAPS, n_ocr=g["max_ocr_tokens"]))
    table = M.score_tables_from_text(bd, GOLDEN_CAPS)
    ids = torch.as_tensor(golden["ids"]).cuda()
    sc, fl = M.score_predictions(ids, table, golden["vt"], return_flags=True)
    assert not fl.any()
    check_scores(sc.cpu().numpy(), golden["cases"])
    sc_host, fl_host = M.score_predictions(ids, golden["table"], golden["vt"], return_flags=True)
    assert torch.equal(sc.view(torch.int32), sc_host.view(torch.int32)) and torch.equal(fl, fl_host)


def test_trainer_metric_on_the_device_built_table_equals_the_host_built_one():
    """one eager step of the smallest model of tests/test_metrics_gpu.py's Trainer test, its score table built from text in front of the step"""
    from sam_textvqa_amd import answers as A
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_answers_gpu import batches, small_model, with_inputs
    bd, table = batches()
    voc, answers, tokens = M.make_score_text(4, num_vocab=200, n_ocr=50, seed=5)
    _, a_tabs, s_tabs = M.make_score_tables(4, num_vocab=200, n_ocr=50, seed=5)
    assert all(torch.equal(v, A.collate_answer_tables(a_tabs)[k]) for k, v in table.items())       # the same samples
    vt, text = M.vocab_text(voc), on_gpu(pack(answers, tokens))
    assert M.check_score_text(text)
    got = {}
    for name in ("host", "text"):
        stab = M.collate_score_tables(s_tabs) if name == "host" else M.score_tables_from_text(text)
        tr = Trainer(small_model(), seed=7, base_lr=1e-3, use_graph=False, answer_targets="table", predictions=True, metric="textvqa", metric_vocab=vt)
        loss = tr.step(with_inputs(bd, answer_table=table, score_table=stab)).clone()
        got[name] = (loss.cpu(), tr.batch_scores().cpu(), tr.score_flags().cpu(), tr.predictions().cpu())
    assert torch.equal(got["host"][3], got["text"][3]) and torch.equal(got["host"][0], got["text"][0])
    assert torch.equal(got["host"][1].view(torch.int32), got["text"][1].view(torch.int32)) and torch.equal(got["host"][2], got["text"][2])
    want = M.score_answers_host(got["text"][3].numpy(), M.collate_score_tables(s_tabs), vt)
    assert np.array_equal(got["text"][1].numpy().view(np.int32), want.view(np.int32))
