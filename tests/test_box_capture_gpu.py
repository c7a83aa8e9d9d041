"""GPU: Trainer(capture_box_batches=True) -- the captured training step on batches that set "spatial_from_boxes" (DESIGN.md section 3.13).

Every comparison of two training runs is captured against captured (an eager and a captured run draw different dropout masks by design,
Trainer.GRAPH_OFFSET_STRIDE) and exact (torch.equal): the Trainers run with answer_targets="table", whose loss is summed in a fixed order.  Shapes: the
table model and the B = 4 batches of tests/test_mask_boxes_gpu.py's training test (c3 token layout, one TextBert layer, MMT n,s)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ORDER = (0, 1, 2, 0, 1, 2)             # warm-up, capture + replay, four more replays, rotating over three batches
T, N_OBJ, N_OCR, N_DEC, HEADS, QUADS, CONTEXT = 20, 100, 50, 12, 12, (1, 2), 3


@functools.lru_cache(maxsize=None)
def box_batches():
    """three from-boxes batches with different boxes (no dense answer half) + one collated answer table; built once, never written to"""
    from sam_textvqa_amd.synthetic import make_batch
    from tests.test_answers_gpu import batches
    _, table = batches()
    out = []
    for seed in (3, 4, 5):
        bd = make_batch(4, vocab=200, device="cuda", seed=seed, spatial="boxes")
        for k in ("targets", "train_prev_inds", "train_loss_mask"):
            del bd[k]
        out.append(bd)
    return tuple(out), table


def allow_bits(bd, thr=0.5):
    """the per-head allow bits the spatial layer of the table model reads for this batch"""
    from sam_textvqa_amd import ops
    kv = ops.pack_masks(bd["question_mask"], bd["pad_obj_mask"], bd["pad_ocr_mask"])[0]
    return ops.mask_bits_from_boxes(ops.mask_bits_prefix_lm(kv, N_DEC), bd["pad_obj_bboxes"], bd["pad_ocr_bboxes"], T, HEADS, QUADS, CONTEXT, thr)


def box_trainer(**kw):
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_answers_gpu import small_model as table_model
    args = dict(seed=7, base_lr=1e-3, use_graph=True, capture_box_batches=True, answer_targets="table", predictions=True)
    args.update(kw)
    return Trainer(table_model(), **args)


def captured_on(batches, table, steps=2):
    """a Trainer whose graph was captured on `batches` (step 0 warms up, step 1 captures and replays)"""
    from tests.test_answers_gpu import with_inputs
    tr = box_trainer()
    for i in range(steps):
        tr.step(with_inputs(batches[i % len(batches)], answer_table=table))
    assert tr._graph is not None
    return tr


class CountingGraph:
    """stands in for Trainer._graph: counts the replays it passes on"""

    def __init__(self, graph):
        self.graph, self.replays = graph, 0

    def replay(self):
        self.replays += 1
        self.graph.replay()


def count_replays(tr, monkeypatch):
    tr._graph = CountingGraph(tr._graph)
    monkeypatch.setattr(tr, "_capture", lambda *a, **k: pytest.fail("a second capture was attempted"))
    return tr._graph


@pytest.mark.parametrize("form", ["padded", "ragged"])
def test_captured_steps_from_boxes_equal_the_relation_tensor_form_bit_for_bit(form):
    """six captured-mode steps over three rotating batches, from boxes against the same batches carrying the relation tensor of their boxes (two-kernel path):
    losses, flat parameters and predictions are bit-identical.  Ragged: the boxes the captured mask launch reads are the ones sam_ragged_expand wrote inside
    the same replay.  The batches' allow bits differ, so bits kept from the warm-up or the capture would show on the replays of the other batches."""
    from sam_textvqa_amd import ragged as R
    from tests.test_answers_gpu import with_inputs
    from tests.test_mask_boxes_gpu import with_adjacency
    boxes, table = box_batches()
    bits = [allow_bits(b) for b in boxes]
    for i in range(3):
        assert not torch.equal(boxes[i]["pad_obj_bboxes"], boxes[(i + 1) % 3]["pad_obj_bboxes"])
        assert not torch.equal(bits[i], bits[(i + 1) % 3]), "batches %d and %d have the same allow bits: a stale mask would pass" % (i, (i + 1) % 3)
    adjacency = [with_adjacency(b) for b in boxes]
    if form == "ragged":
        boxes, adjacency = ([R.from_padded(b, feature_dtype=torch.float32) for b in bs] for bs in (boxes, adjacency))
    runs = {}
    for name, batches in (("boxes", boxes), ("adjacency", adjacency)):
        tr = box_trainer()
        losses, graphs = [], []
        for i in ORDER:
            losses.append(tr.step(with_inputs(batches[i], answer_table=table)).clone())
            graphs.append(tr._graph)
        assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[2:]), name
        bufs = tr.input_buffers()
        if name == "boxes":
            assert bufs["spatial_from_boxes"] is True and "spatial_adj_matrices" not in bufs and "spatial_distance_threshold" not in bufs
        else:
            assert "spatial_from_boxes" not in bufs and bufs["spatial_adj_matrices"][str(CONTEXT)].dtype == torch.int8
        assert (set(R.RAGGED_KEYS) <= set(bufs) and not set(R.PADDED_KEYS) & set(bufs)) if form == "ragged" else "pad_obj_bboxes" in bufs
        tr.flush_update()
        torch.cuda.synchronize()
        runs[name] = (torch.stack(losses).cpu(), tr.flat.flat.clone(), tr.predictions().clone())
        del tr
    (la, pa, qa), (lb, pb, qb) = runs["adjacency"], runs["boxes"]
    print("%s captured losses: adjacency %r, boxes %r; parameters differ in %d places, predictions in %d" % (
        form, la.tolist(), lb.tolist(), (pa != pb).sum().item(), (qa != qb).sum().item()))
    assert torch.isfinite(la).all() and len(set(la.tolist())) == len(ORDER)
    assert torch.equal(la, lb), (la.tolist(), lb.tolist())
    assert torch.equal(pa, pb) and torch.equal(qa, qb)


def test_matching_batches_replay_the_graph_once_per_step(monkeypatch):
    from sam_textvqa_amd import ops
    from tests.test_answers_gpu import with_inputs
    boxes, table = box_batches()
    launches = []
    real = ops.mask_bits_from_boxes
    monkeypatch.setattr(ops, "mask_bits_from_boxes", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    tr = captured_on(boxes, table)
    assert len(launches) == 2                                  # the warm-up step's launch and the one recorded into the graph
    g = count_replays(tr, monkeypatch)
    losses = []
    for n, i in enumerate((2, 0, 1), 1):
        losses.append(tr.step(with_inputs(boxes[i], answer_table=table)).item())
        assert g.replays == n and tr._graph is g
    assert len(launches) == 2                                  # no launch issued from Python any more: the replays carry it
    assert all(np.isfinite(losses)) and len(set(losses)) == 3


def test_a_batch_in_another_form_runs_eagerly_and_the_graph_survives(monkeypatch):
    """graph captured on (flag, no threshold): another threshold, the flag switched off next to relation tensors, and no flag at all (a batch without the
    flag needs the relation tensors to run) each take the eager step; the graph stays and serves the next matching batch"""
    from tests.test_answers_gpu import with_inputs
    from tests.test_mask_boxes_gpu import with_adjacency
    boxes, table = box_batches()
    tr = captured_on(boxes, table)
    g = count_replays(tr, monkeypatch)
    assert not torch.equal(allow_bits(boxes[2], 0.35), allow_bits(boxes[2]))       # the other threshold asks for other bits
    others = (dict(boxes[2], spatial_distance_threshold=0.35), dict(with_adjacency(boxes[2]), spatial_from_boxes=False), with_adjacency(boxes[2]))
    for n, other in enumerate(others, 1):
        step = tr.global_step
        loss = tr.step(with_inputs(other, answer_table=table)).item()
        assert np.isfinite(loss) and g.replays == 0 and tr._graph is g and tr.global_step == step + 1, n
    assert tr.input_buffers()["spatial_from_boxes"] is True and "spatial_distance_threshold" not in tr.input_buffers()
    loss = tr.step(with_inputs(boxes[0], answer_table=table)).item()
    assert np.isfinite(loss) and g.replays == 1 and tr._graph is g


def host_samples(bd):
    """the unpadded per-sample tensors a dataset hands collate_ragged, cut out of a padded CPU batch"""
    out = []
    for b in range(bd["pad_obj_mask"].shape[0]):
        n, m = int(bd["pad_obj_mask"][b].sum()), int(bd["pad_ocr_mask"][b].sum())
        out.append(dict(obj_features=bd["pad_obj_features"][b, :n], obj_bboxes=bd["pad_obj_bboxes"][b, :n], ocr_features=bd["pad_ocr_features"][b, :m],
                        ocr_fasttext=bd["ocr_fasttext"][b, :m], ocr_phoc=bd["ocr_phoc"][b, :m], ocr_bboxes=bd["pad_ocr_bboxes"][b, :m]))
    return out


def test_a_collated_ragged_batch_uploaded_into_the_input_buffers_is_stepped_without_staging(monkeypatch):
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.modules import spatial_box_items
    from sam_textvqa_amd.synthetic import make_batch
    from tests.test_answers_gpu import with_inputs
    _, table = box_batches()
    hosts = []
    for seed in (3, 4, 5):
        bd = make_batch(4, vocab=200, device="cpu", seed=seed, spatial="boxes")
        host = R.collate_ragged(host_samples(bd), N_OBJ, N_OCR, spatial_from_boxes=True)           # fp16 rows
        host.update(question_indices=bd["question_indices"], question_mask=bd["question_mask"])
        hosts.append(host)
    assert not torch.equal(hosts[1]["ocr_count"], hosts[2]["ocr_count"])
    on_gpu = lambda h: {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in h.items()}
    a, b = captured_on([on_gpu(h) for h in hosts], table), captured_on([on_gpu(h) for h in hosts], table)
    bufs = a.input_buffers()
    assert spatial_box_items(bufs) == spatial_box_items(hosts[2]) == (("spatial_from_boxes", True),)
    assert bufs["obj_rows"].dtype == torch.float16 and "spatial_adj_matrices" not in bufs and not set(R.PADDED_KEYS) & set(bufs)
    assert R.upload(hosts[2], bufs) is bufs
    staged = a.input_buffers()
    assert all(v.data_ptr() == dst.data_ptr() for (_, _, v), dst in zip(a._flatten(staged), a._static_in))       # what _graph_step compares: nothing is stale
    g = count_replays(a, monkeypatch)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "_foreach_copy_", lambda *x, **k: pytest.fail("an input was staged"))
        la = a.step(staged)
    assert g.replays == 1
    lb = b.step(with_inputs(on_gpu(hosts[2]), answer_table=table))
    torch.cuda.synchronize()
    print("loss through input_buffers() %r, through step(batch) %r" % (la.item(), lb.item()))
    assert torch.isfinite(la) and torch.equal(la, lb)


def test_the_constructor_default_leaves_box_batches_uncaptured(monkeypatch):
    """Trainer(use_graph=True) without the new argument: what tests/test_mask_boxes_gpu.py::test_a_batch_from_boxes_is_never_captured pins, restated here"""
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_mask_boxes_gpu import small_batch, small_model
    tr = Trainer(small_model(), base_lr=1e-3, seed=3, use_graph=True)
    assert tr.use_graph and tr.capture_box_batches is False
    monkeypatch.setattr(tr, "_capture", lambda *a, **k: pytest.fail("a capture was attempted"))
    bd = small_batch(21, n=4)
    losses = [tr.step(clone_batch(bd)).item() for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[0] != losses[1]
    assert tr._graph is None and not tr._graph_warm and tr.use_graph and tr.input_buffers() is None
