"""GPU: sam_mask_bits_from_boxes (csrc/mask_boxes.hip, include/sam_hip_pipeline.h) and the batch opt-in "spatial_from_boxes" through the model, eager
training steps and the decoders.

The entry point is defined by equivalence with the two launches it replaces, so every comparison here is exact (torch.equal): no tolerance anywhere.
Kernel shapes (B, T, n_obj, n_ocr, n_dec): N = 21 (one word, T not a multiple of 4), 82 (two ballot passes), 182 (the c3 layout), 270 (12-word row stride
of which 9 are used: the padding words must read 0).  The model / trainer / decoder cases run the small configuration of tests/test_ragged_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests.util import unpack_bits

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(2, 5, 7, 6, 3), (2, 20, 40, 10, 12), (1, 20, 100, 50, 12), (1, 20, 180, 58, 12)]
QUADRANT_SETS = [(), (1, 2), (1, 2, 4, 7, 8, 9)]
ZERO_OBJ, MASKED_OBJ, ZERO_OCR = 4, 5, 2                      # all-zero rows in the middle of both groups; a valid box whose key the base bits mask

# groups of boxes that must share a sample (xyxy); all pairs of a sample are classified, these guarantee the named relations exist
SPECIAL = [
    [(0.10, 0.10, 0.60, 0.60), (0.20, 0.20, 0.40, 0.40)],     # a covers b / b inside a (codes 1 and 2)
    [(0.50, 0.50, 0.70, 0.70), (0.52, 0.50, 0.72, 0.70)],     # IoU 0.82, neither covers (code 3)
    [(0.30, 0.62, 0.36, 0.68), (0.30, 0.62, 0.36, 0.68)],     # two identical boxes: IoU 1 (code 3)
    [(0.77, 0.33, 0.77, 0.33), (0.77, 0.33, 0.77, 0.33)],     # two identical boxes of zero area: IoU = 0/0 is no match, coincident centres -> code 4 both ways
    [(0.375, 0.125, 0.625, 0.25), (0.46875, 0.0, 0.53125, 0.375)],     # a cross: coincident centres (exact in binary), IoU 0.17 -> code 4
    [(0.01, 0.01, 0.05, 0.05), (0.90, 0.90, 0.99, 0.99)],     # centres 1.29 apart: beyond the limit 0.5 * sqrt(2) (code 0)
    [(0.10, 0.80, 0.20, 0.90), (0.50, 0.80, 0.60, 0.90)],     # same centre height: axis-aligned, on a sector boundary
    [(0.80, 0.10, 0.90, 0.20), (0.80, 0.50, 0.90, 0.60)],     # same centre column
    [(0.05, 0.30, 0.15, 0.40), (0.25, 0.50, 0.35, 0.60)],     # 45 degrees
    [(0.60, 0.30, 0.70, 0.40), (0.40, 0.50, 0.50, 0.60)],     # 135 degrees
]


def _ops():
    from sam_textvqa_amd import ops
    return ops


def hand_built_boxes(shape):
    """float64 [B, n_obj + n_ocr, 4] (numpy) with values fp32 cannot hold + the validity of every row as the base bits will see it"""
    B, T, n_obj, n_ocr, n_dec = shape
    n_oo = n_obj + n_ocr
    rng = np.random.RandomState(sum(shape))
    xy = rng.rand(B, n_oo, 2) * 0.8
    boxes = np.concatenate([xy, np.minimum(xy + 0.01 + rng.rand(B, n_oo, 2) * 0.2, 1.0)], -1)
    free = [j for j in range(n_oo) if j not in (ZERO_OBJ, MASKED_OBJ, n_obj + ZERO_OCR)]
    at = [0] * B
    for gi, group in enumerate(SPECIAL):                      # groups alternate over the samples; a sample's specials fill its free slots from the front,
        b = gi % B                                            # so at the smallest shape a pair straddles the object / OCR border
        for box in group:
            # (shifted off the fp32 grid, except the two coincident-centre groups: theirs must stay exact)
            boxes[b, free[at[b]]] = np.asarray(box) + (0.0 if gi in (3, 4) else (1.0 / 3.0) * 2.0 ** -30)
            at[b] += 1
    assert max(at) <= len(free)
    boxes[:, ZERO_OBJ] = 0.0
    boxes[:, n_obj + ZERO_OCR] = 0.0
    valid = (np.abs(boxes).sum(-1) != 0)
    valid[:, MASKED_OBJ] = False
    return boxes, valid


@functools.lru_cache(maxsize=None)
def problem(shape):
    """hand-built boxes + masks of a shape, on the device: float64 boxes [B, n, 4], their fp32 rounding with row stride 5 (the batch's pad_*_bboxes),
    key_valid, and the base bits.  Built once per shape."""
    ops = _ops()
    B, T, n_obj, n_ocr, n_dec = shape
    boxes, valid = hand_built_boxes(shape)
    n_txt = [T - (b % 2) * 2 for b in range(B)]
    kv = np.concatenate([np.arange(T)[None, :] < np.asarray(n_txt)[:, None], valid], 1).astype(np.uint8)
    b64 = torch.from_numpy(boxes).cuda()
    b32 = b64.float()
    area = ((b32[..., 2] - b32[..., 0]) * (b32[..., 3] - b32[..., 1])).unsqueeze(-1)
    b32 = torch.cat([b32, area], -1).contiguous()             # [B, n, 5]
    assert not torch.equal(b32[..., :4].double(), b64)
    key_valid = torch.from_numpy(kv).cuda()
    base = ops.mask_bits_prefix_lm(key_valid, n_dec)
    return dict(B=B, T=T, n_obj=n_obj, n_ocr=n_ocr, n_dec=n_dec, N=T + n_obj + n_ocr + n_dec, b64=b64, b32=b32, key_valid=key_valid, base=base)


def two_kernel(pr, boxes, ctx, heads, quads, thr=0.5):
    """the parent's path: relation tensor of float64(cat(obj, ocr)), then the packer"""
    ops = _ops()
    adj = ops.spatial_relation_tensor(boxes[..., :4].double().contiguous(), ctx, thr)
    return adj, ops.mask_bits_spatial(pr["base"], adj, pr["T"], heads, quads)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["N21", "N82", "N182", "N270"])
def test_one_launch_equals_the_two_kernel_path(shape):
    ops = _ops()
    pr = problem(shape)
    n_obj = pr["n_obj"]
    seen = set()
    for name, boxes in (("fp32 ld 5", pr["b32"]), ("f64", pr["b64"])):
        obj, ocr = boxes[:, :n_obj].contiguous(), boxes[:, n_obj:].contiguous()
        for ctx in (1, 3, 9):
            for heads in (12, 16):
                for quads in QUADRANT_SETS:
                    adj, want = two_kernel(pr, boxes, ctx, heads, quads)
                    out = torch.full((pr["B"], heads, pr["N"], pr["base"].shape[-1]), -1, dtype=torch.int32, device="cuda")          # 0xFFFFFFFF everywhere
                    got = ops.mask_bits_from_boxes(pr["base"], obj, ocr, pr["T"], heads, quads, ctx, out=out)
                    assert got is out
                    assert torch.equal(got, want), "%s ctx %d H %d quadrants %s" % (name, ctx, heads, quads)
            if ctx == 1:
                codes = adj.to(torch.int64).argmax(-1)[adj.any(-1)] + 1
                seen |= set(codes.unique().tolist())
        # the padding words of the row stride read 0 (N = 270: words 9..11), the rest is not all-zero
        nw = pr["base"].shape[-1]
        assert (unpack_bits(got, nw * 32)[..., pr["N"]:] == 0).all() and got.ne(0).any()
    assert seen == set(range(1, 13)), "the hand-built boxes must produce every relation code, got %s" % sorted(seen)
    # another distance limit, and no `out`
    obj, ocr = pr["b32"][:, :n_obj].contiguous(), pr["b32"][:, n_obj:].contiguous()
    _, want = two_kernel(pr, pr["b32"], 3, 12, (1, 2), thr=0.2)
    assert torch.equal(ops.mask_bits_from_boxes(pr["base"], obj, ocr, pr["T"], 12, (1, 2), 3, distance_threshold=0.2), want)
    assert not torch.equal(want, two_kernel(pr, pr["b32"], 3, 12, (1, 2))[1])


def test_the_hand_built_relations_are_where_they_were_put():
    """the boxes of the smallest shape, read back through the relation kernel the equivalence is defined by (context 1: one channel per pair)"""
    pr = problem(KERNEL_SHAPES[0])
    adj, _ = two_kernel(pr, pr["b64"], 1, 12, ())
    code = lambda b, i, j: (int(adj[b, i, j].to(torch.int64).argmax()) + 1) if bool(adj[b, i, j].any()) else 0
    # sample 0 holds groups 0, 2, 4, 6, 8 in free slots 0, 1 | 2, 3 | 6, 7 | 8, 10 | 11, 12; sample 1 groups 1, 3, 5, 7, 9 likewise
    assert (code(0, 0, 1), code(0, 1, 0)) == (1, 2)
    assert (code(0, 2, 3), code(0, 3, 2)) == (3, 3)
    assert (code(0, 6, 7), code(0, 7, 6)) == (4, 4)                      # the cross straddles the object / OCR border (n_obj = 7)
    assert (code(1, 0, 1), code(1, 1, 0)) == (3, 3)
    assert (code(1, 2, 3), code(1, 3, 2)) == (4, 4)                      # identical zero-area boxes
    assert (code(1, 6, 7), code(1, 7, 6)) == (0, 0)                      # beyond the limit
    assert code(0, 0, 0) == 12 and code(0, ZERO_OBJ, ZERO_OBJ) == 0 and code(0, MASKED_OBJ, MASKED_OBJ) == 12
    assert not adj[:, ZERO_OBJ].any() and not adj[:, :, 7 + ZERO_OCR].any()


def test_allow_bits_from_golden_boxes_equal_the_reference():
    """the reference's own graphs (tests/golden/spatial_graph.npz): unpacked bits == the oracle's mask algebra over the golden relation tensor.  `grid` has
    pairs exactly on sector boundaries, where the reference's own libm decides (test_spatial_graph_kernel_matches_reference_goldens): it is compared with
    the two-kernel GPU path, which shares the device code."""
    from oracle import sa_m4c_oracle as O
    from tests import oracle_cases as OC
    ops = _ops()
    g = OC.load("spatial_graph")
    T = 3
    for nm in ("known6", "rnd60", "cross", "grid"):
        boxes = torch.from_numpy(g[nm + ".boxes"])[None].cuda()                    # f64 [1, n, 4]; one tensor, no OCR group
        n = boxes.shape[1]
        key_valid = torch.ones(1, T + n, dtype=torch.uint8)
        base = ops.mask_bits_prefix_lm(key_valid.cuda(), 0)
        for ctx in (1, 3, 5, 7, 9):
            for quads in ((), (1, 2)):
                out = torch.full((1, 12, T + n, base.shape[-1]), -1, dtype=torch.int32, device="cuda")
                got = ops.mask_bits_from_boxes(base, boxes, None, T, 12, quads, ctx, out=out)
                if nm == "grid":
                    want = ops.mask_bits_spatial(base, ops.spatial_relation_tensor(boxes, ctx), T, 12, quads)
                    assert torch.equal(got, want), "%s ctx%d" % (nm, ctx)
                else:
                    ref = O.allow_mask(key_valid, T, n, 0, torch.from_numpy(g["%s.ctx%d" % (nm, ctx)])[None], quads, 12)
                    assert torch.equal(unpack_bits(got, T + n), ref), "%s ctx%d quadrants %s" % (nm, ctx, quads)
                    assert (unpack_bits(got, got.shape[-1] * 32)[..., T + n:] == 0).all()


# ------------------------------------------------------------------------------------------ model, trainer, decoders
SHAPES = (7, 20, 9, 3)                 # (T, n_obj, n_ocr, n_dec): the small configuration of tests/test_ragged_gpu.py


def small_batch(seed, n=3, spatial="boxes"):
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(n, *SHAPES, vocab=300, context=3, device="cuda", seed=seed, spatial=spatial)
    bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
    return bd


def with_adjacency(bd, contexts=(3,), thr=0.5):
    """the same batch in the form the dataset ships: no flag, the relation tensors of float64(the batch's fp32 boxes)"""
    ops = _ops()
    out = {k: v for k, v in bd.items() if k not in ("spatial_from_boxes", "spatial_distance_threshold")}
    boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    out["spatial_adj_matrices"] = {str(c): ops.spatial_relation_tensor(boxes, c, thr) for c in contexts}
    return out


def small_model(layers=("n", "s"), mix=None, seed=0):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    T, n_obj, n_ocr, n_dec = SHAPES
    md = mmt_config_dict(3, layers, n_dec=n_dec, T=T, n_obj=n_obj, n_ocr=n_ocr)
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0)
    if mix is not None:
        md["mix_list"] = list(mix)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=500)
    torch.manual_seed(seed)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=300, bos_idx=1)


def test_model_scores_from_boxes_equal_the_adjacency_form(monkeypatch):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    model = small_model(("s", "n", "s", "s"), ("share3", "none", "share3", "share5")).cuda().train()
    prepare(model)
    bd = small_batch(11)
    bd["spatial_distance_threshold"] = 0.35
    launches = []
    real = ops.mask_bits_from_boxes
    monkeypatch.setattr(ops, "mask_bits_from_boxes", lambda *a, **k: (launches.append((a[6], a[7] if len(a) > 7 else k.get("distance_threshold"))), real(*a, **k))[1])
    a = clone_batch(bd)
    with torch.no_grad():
        got = model(a)["textvqa_scores"]
        want = model(clone_batch(with_adjacency(bd, (3, 5), 0.35)))["textvqa_scores"]
    assert launches == [(3, 0.35), (5, 0.35)]                  # two layers of one context share a launch; a second context costs a second
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert "spatial_adj_matrices" not in a
    with torch.no_grad():                                      # the threshold is read: the default gives other bits on this batch, hence other scores
        other = model(clone_batch(with_adjacency(bd, (3, 5), 0.5)))["textvqa_scores"]
    assert not torch.equal(other, want)
    with pytest.raises(ValueError, match="spatial_from_boxes"):
        model(dict(with_adjacency(bd, (3, 5)), spatial_from_boxes=True))


def table_batches():
    """two batches of tests/test_answers_gpu.py's kind (c3 shapes, no dense answer half) with different boxes, from boxes, + one collated answer table"""
    from sam_textvqa_amd.synthetic import make_batch
    from tests.test_answers_gpu import batches
    _, table = batches()
    out = []
    for seed in (3, 4):
        bd = make_batch(4, vocab=200, device="cuda", seed=seed, spatial="boxes")
        for k in ("targets", "train_prev_inds", "train_loss_mask"):
            del bd[k]
        out.append(bd)
    assert not torch.equal(out[0]["pad_obj_bboxes"], out[1]["pad_obj_bboxes"])
    return out, table


def test_eager_training_steps_from_boxes_equal_the_adjacency_form_bit_for_bit():
    """two eager Trainer steps over two batches with different boxes: from boxes against the adjacency form, and the ragged form of each (the boxes the launch
    reads are then the ones sam_ragged_expand wrote a moment earlier; compared with its own adjacency form, the ragged operand coming out of another kernel).
    Losses and flat parameters are bit-identical.  The Trainers run with answer_targets="table", whose loss is summed in a fixed order (csrc/bce_table.hip;
    tests/test_metrics_gpu.py holds two fresh Trainers of this kind to torch.equal): sam_bce_loss of the dense path adds its blocks' partial sums with fp32
    atomics, so its loss scalar differs in the last bit from run to run whatever feeds it."""
    from sam_textvqa_amd import ragged as R
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_answers_gpu import small_model as table_model, with_inputs
    boxes, table = table_batches()
    adjacency = [with_adjacency(b) for b in boxes]
    ragged = lambda bs: [R.from_padded(b, feature_dtype=torch.float32) for b in bs]
    runs = {}
    for name, batches in (("boxes", boxes), ("adjacency", adjacency), ("ragged boxes", ragged(boxes)), ("ragged adjacency", ragged(adjacency))):
        tr = Trainer(table_model(), seed=7, base_lr=1e-3, use_graph=False, answer_targets="table", predictions=True)
        losses = torch.stack([tr.step(with_inputs(batches[i], answer_table=table)).clone() for i in (0, 1)]).cpu()
        torch.cuda.synchronize()
        runs[name] = (losses, tr.flat.flat.clone())
        del tr
    print("eager losses: %r" % {k: v[0].tolist() for k, v in runs.items()})
    for name, ref in (("boxes", "adjacency"), ("ragged boxes", "ragged adjacency")):
        (la, pa), (lb, pb) = runs[ref], runs[name]
        assert torch.isfinite(la).all() and la[0] != la[1]
        print("%s: max |d loss| %.3e, parameters differ in %d places (max %.3e)" % (name, (la - lb).abs().max().item(), (pa != pb).sum().item(), (pa - pb).abs().max().item()))
        assert torch.equal(la, lb), (name, la.tolist(), lb.tolist())
        assert torch.equal(pa, pb), name


def test_a_batch_from_boxes_is_never_captured(monkeypatch):
    """Trainer(use_graph=True): the captured step keeps only a batch's tensors, so a batch that sets the flag takes the eager step -- no warm-up
    for a capture, no capture, and the Trainer stays able to capture other batches"""
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    tr = Trainer(small_model(), base_lr=1e-3, seed=3, use_graph=True)
    assert tr.use_graph
    monkeypatch.setattr(tr, "_capture", lambda *a, **k: pytest.fail("a capture was attempted"))
    bd = small_batch(21, n=4)
    losses = [tr.step(clone_batch(bd)).item() for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[0] != losses[1]
    assert tr._graph is None and not tr._graph_warm and tr.use_graph and tr.input_buffers() is None


def test_ops_wrapper_rejects_an_illegal_quadrant():
    ops = _ops()
    pr = problem(KERNEL_SHAPES[0])
    obj, ocr = pr["b32"][:, :pr["n_obj"]].contiguous(), pr["b32"][:, pr["n_obj"]:].contiguous()
    for quads in ((3,), (1, 5), (6,), (10,)):
        with pytest.raises(ValueError, match="quadrant"):
            ops.mask_bits_from_boxes(pr["base"], obj, ocr, pr["T"], 12, quads, 3)


@pytest.mark.parametrize("env", [{}, {"SAM_DECODE_FUSED": "0", "SAM_BEAM_SHARED": "0"}], ids=["fused-shared", "fallback-expanded"])
def test_greedy_and_beam_decoding_equal_the_adjacency_form(env, monkeypatch):
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.registry import registry
    from sam_textvqa_amd.synthetic import clone_batch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = small_model().cuda().eval()
    prepare(model)
    bd = small_batch(23, n=4)
    bd["train_prev_inds"] = torch.zeros_like(bd["train_prev_inds"])
    bd["train_prev_inds"][:, 0] = 1
    adj = with_adjacency(bd)
    monkeypatch.setattr(registry, "EOS_IDX", 2, raising=False)
    monkeypatch.setattr(registry, "BOS_IDX", 1, raising=False)
    model.set_beam_size(3)
    with torch.no_grad():
        a, b = clone_batch(bd), clone_batch(adj)
        sa, sb = model(a)["textvqa_scores"], model(b)["textvqa_scores"]
        assert torch.isfinite(sa[sa > -9000]).all()
        assert torch.equal(a["train_prev_inds"], b["train_prev_inds"]) and torch.equal(sa, sb)
        ba, bb = model(clone_batch(bd), use_beam_search=True), model(clone_batch(adj), use_beam_search=True)
        assert ba["complete_seqs"].reshape(-1, SHAPES[3]).shape[0] == 4 * 3
        assert torch.equal(ba["complete_seqs"], bb["complete_seqs"]) and torch.equal(ba["topkscores"], bb["topkscores"])
        assert torch.equal(ba["textvqa_scores"], bb["textvqa_scores"])
