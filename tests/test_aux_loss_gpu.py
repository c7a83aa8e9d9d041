"""GPU: the spatial aux heads' loss (csrc/aux_loss.hip) on the MI355X -- relation codes from boxes against the relation tensor, the
fused loss and its gradients against the float64 host twin (with the composition sam_aux_pair_fwd -> torch BCE -> sam_aux_pair_bwd as the yardstick of
what fp32 achieves), masked rows, reproducibility, and SAM4C.spatial_aux_loss.

Shapes: the forward tiles are 64 j x 16 i, the backward's 64 i x 32 j.  n = 7 (3 obj + 4 ocr: one partial tile), 70 (crosses 64; 70 % 32, 70 % 16 != 0),
129 (one past 128).  B = 3: sample 0 has some padded object and OCR rows, sample 1 no valid OCR row, sample 2 is entirely padded."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C
from tests.test_aux_heads_gpu import L, rel, within

pytestmark = pytest.mark.gpu

SHAPES = {7: (3, 4), 70: (40, 30), 129: (100, 29)}          # n -> (n_obj, n_ocr)
ULP32 = 2.0 ** -23


def _case(n, seed, b=3):
    """O, D, W, bias on the GPU, codes and valid as described above"""
    n_obj, n_ocr = SHAPES[n]
    g = torch.Generator(device="cpu").manual_seed(seed)
    o, d = torch.randn(b, n, 32, generator=g), torch.randn(b, n, 32, generator=g)
    w, bias = torch.randn(12, 32, generator=g) * 0.2, torch.randn(12, generator=g) * 0.1
    codes = torch.randint(0, 13, (b, n, n), generator=g).to(torch.uint8)
    valid = torch.zeros(b, n, dtype=torch.uint8)
    valid[0, : n_obj - 1] = 1
    valid[0, n_obj: n_obj + max(1, n_ocr // 2)] = 1
    if b > 1:
        valid[1, :n_obj] = 1                                  # no valid OCR row
    return [t.cuda() for t in (o, d, w, bias, codes, valid)]


_REF = {}


def _host(n, seed, fusion, b=3):
    """float64 twin: (loss, dO, dD, dW, dbias), computed once per case"""
    key = (n, seed, fusion, b)
    if key not in _REF:
        from sam_textvqa_amd import ops
        o, d, w, bias, codes, valid = _case(n, seed, b)
        od, dd, wd, bd = (t.double().cpu().requires_grad_(True) for t in (o, d, w, bias))
        loss, _ = ops.aux_loss_host(od, dd, wd, bd, codes, valid, fusion)
        loss.backward()
        _REF[key] = tuple(t.detach() for t in (loss, od.grad, dd.grad, wd.grad, bd.grad))
    return _REF[key]


def _fused(o, d, w, bias, codes, valid, fusion, grad_out=None):
    from sam_textvqa_amd import ops
    loss, count = ops.aux_pair_loss(o, d, w, bias, codes, valid, fusion)
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    d_o, d_d = ops.aux_pair_loss_bwd(grad_out, count, o, d, w, bias, codes, valid, dw, db, fusion, accumulate=False)
    return loss, count, d_o, d_d, dw, db


def _composition(o, d, w, bias, codes, valid, fusion):
    """the route available without the fused node: dense fp32 logits, torch BCE, autograd's dense gradient into sam_aux_pair_bwd"""
    from sam_textvqa_amd import ops
    s = ops.aux_pair_fwd(o, d, w, bias, fusion).requires_grad_(True)
    y = (codes.unsqueeze(-1).long() == torch.arange(1, 13, device="cuda")).float()
    m = (valid.bool().unsqueeze(2) & valid.bool().unsqueeze(1)).float()
    loss = (F.binary_cross_entropy_with_logits(s, y, reduction="none").sum(-1) * m).sum() / m.sum().clamp(min=1)
    loss.backward()
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    d_o, d_d = ops.aux_pair_bwd(s.grad, o, d, w, dw, db, fusion, accumulate=False)
    return loss.detach(), d_o, d_d, dw, db


# ---------------------------------------------------------------------------------------------- codes from boxes
def _codes_via_tensor(boxes64):
    from sam_textvqa_amd import ops
    return ops.codes_from_relation_tensor(ops.spatial_relation_tensor(boxes64.contiguous(), 1))


@pytest.mark.parametrize("name", ["known6", "grid", "rnd60", "cross"])
def test_codes_from_golden_boxes_equal_the_relation_tensors_codes(name):
    from sam_textvqa_amd import ops
    g = np.load(os.path.join(C.GOLDEN_DIR, "spatial_graph.npz"))
    boxes = torch.from_numpy(g[name + ".boxes"]).cuda().unsqueeze(0)
    k = boxes.shape[1] // 2
    got = ops.relation_codes_from_boxes(boxes[:, :k], boxes[:, k:])
    assert got.dtype == torch.uint8 and torch.equal(got, _codes_via_tensor(boxes))
    # (how the relation tensor itself compares with the reference on pairs that sit on a sector boundary is tests/test_spatial_graph*'s subject)
    assert torch.equal(ops.relation_codes_from_boxes(boxes), got)                  # no OCR group


@pytest.mark.parametrize("f64", [False, True])
def test_codes_from_random_coincident_and_degenerate_boxes(f64):
    from sam_textvqa_amd import ops
    gen = torch.Generator().manual_seed(5)
    b, n_obj, n_ocr = 3, 37, 33
    xy = torch.rand(b, n_obj + n_ocr, 2, generator=gen) * 0.8
    wh = 0.01 + torch.rand(b, n_obj + n_ocr, 2, generator=gen) * 0.2
    boxes = torch.cat([xy, xy + wh, wh[..., :1] * wh[..., 1:]], -1)              # [B, n, 5] as pad_*_bboxes: xyxy + area
    boxes[:, 5] = boxes[:, 4]                                                     # coincident boxes
    boxes[:, 40] = boxes[:, 3]                                                    # ... across the two groups
    boxes[:, 7, 2:4] = boxes[:, 7, 0:2]                                           # zero area
    boxes[:, 8, 2] = boxes[:, 8, 0]                                               # zero width
    boxes[:, 9, :4] = boxes[:, 10, :4] = torch.tensor([0.25, 0.25, 0.5, 0.5])     # same centre as ...
    boxes[:, 11, :4] = torch.tensor([0.125, 0.125, 0.625, 0.625])                 # ... a box that covers them
    boxes[1, 20:30] = 0                                                           # padding rows
    boxes[2, n_obj:] = 0                                                          # no OCR box at all
    boxes = (boxes.double() if f64 else boxes).cuda()
    got = ops.relation_codes_from_boxes(boxes[:, :n_obj], boxes[:, n_obj:])
    want = _codes_via_tensor(boxes[..., :4].double())
    assert torch.equal(got, want)
    assert int(got.max()) == 12 and bool((got[1, 20:30] == 0).all()) and bool((got[1, :, 20:30] == 0).all()) and len(got.unique()) >= 12


# ---------------------------------------------------------------------------------------------- loss and gradients
@pytest.mark.parametrize("fusion", ["mul", "add"])
@pytest.mark.parametrize("n", [7, 70, 129])
def test_fused_loss_and_gradients_vs_the_float64_twin(fusion, n):
    args = _case(n, 100 + n)
    ref = _host(n, 100 + n, fusion)
    comp = _composition(*args, fusion)
    loss, count, d_o, d_d, dw, db = _fused(*args, fusion)
    valid = args[5]
    assert count.item() == float((valid.sum(1).double() ** 2).sum().item())
    e_comp, e_fused = abs(comp[0].item() - ref[0].item()), abs(loss.item() - ref[0].item())
    bound = 4 * e_comp + ULP32 * abs(ref[0].item())
    print("loss %s n=%d: twin %.9g fused %.9g (err %.3g) composition %.9g (err %.3g) bound %.3g" % (fusion, n, ref[0].item(), loss.item(), e_fused, comp[0].item(), e_comp, bound))
    assert e_fused <= bound, (e_fused, bound)
    for name, got, cmp_, r in (("dO", d_o, comp[1], ref[1]), ("dD", d_d, comp[2], ref[2]), ("dW", dw, comp[3], ref[3]), ("dbias", db, comp[4], ref[4])):
        print("composition %s rel err %.3g" % (name, rel(cmp_, r)))
        within("loss bwd %s %s n=%d" % (name, fusion, n), rel(got, r), L["pair_bwd"])


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_all_padded_batch_gives_zero_loss_and_zero_gradients(fusion):
    o, d, w, bias, codes, valid = _case(70, 9, b=1)
    valid.zero_()
    loss, count, d_o, d_d, dw, db = _fused(o, d, w, bias, codes, valid, fusion)
    assert loss.item() == 0.0 and count.item() == 0.0
    for t in (d_o, d_d, dw, db):
        assert bool((t == 0).all())


@pytest.mark.parametrize("fusion", ["mul", "add"])
@pytest.mark.parametrize("n", [70, 129])
def test_padded_rows_get_zero_gradients_and_their_values_are_never_used(fusion, n):
    o, d, w, bias, codes, valid = _case(n, 200 + n)
    a = _fused(o, d, w, bias, codes, valid, fusion)
    pad = valid == 0
    assert bool(pad.any()) and bool((a[2][pad] == 0).all()) and bool((a[3][pad] == 0).all())
    for poison in (float("nan"), 1e30, -1e30):
        o2, d2 = o.clone(), d.clone()
        o2[pad], d2[pad] = poison, poison
        b = _fused(o2, d2, w, bias, codes, valid, fusion)
        for x, y in zip(a, b):
            assert torch.equal(x, y), poison


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_bit_identical_across_runs_and_cu_reserve_and_exact_power_of_two_scaling(fusion):
    from sam_textvqa_amd import ops
    args = _case(129, 11)
    a, b = _fused(*args, fusion), _fused(*args, fusion)
    was = ops.cu_reserve()
    ops.set_cu_reserve(32)
    try:
        c = _fused(*args, fusion)
    finally:
        ops.set_cu_reserve(was)
    one = _fused(*args, fusion, grad_out=torch.ones(1, device="cuda"))
    quarter = _fused(*args, fusion, grad_out=torch.full((1,), 0.25, device="cuda"))
    torch.cuda.synchronize()
    for x, y, z, u, q in zip(a, b, c, one, quarter):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, u)
    for x, q in zip(a[2:], quarter[2:]):
        assert torch.equal(x * 0.25, q) and float(x.abs().max()) > 0


def test_wrappers_reject_bad_shapes_and_codes():
    from sam_textvqa_amd import _capi, ops
    o, d, w, bias, codes, valid = _case(7, 1)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_loss(o, d, w, bias, codes[:, :6], valid)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_loss(o, d, w, bias, codes.int(), valid)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_loss(o, d, w, bias, codes, valid[:, :6])
    with pytest.raises(ValueError):
        ops.check_relation_codes(torch.full_like(codes, 13))


# ---------------------------------------------------------------------------------------------- module surface (hidden width 768, the real SimpleClassifiers)
def _model(fusion, aux=True, **kw):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"), n_dec=3, T=7, n_obj=20, n_ocr=9)
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0)
    if aux:
        md.update(use_aux_heads=True, aux_spatial_fusion=fusion)
    torch.manual_seed(0)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=60, bos_idx=1, **kw).cuda().train()


def _batch(spatial="adjacency"):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(3, 7, 20, 9, 3, vocab=60, context=3, device="cuda", seed=4, spatial=spatial)
    boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    if spatial == "adjacency":
        bd["spatial_adj_matrices"]["1"] = ops.spatial_relation_tensor(boxes, 1)
    return bd, boxes


AUX = ("origin_transform", "dest_transform", "spatial_classifier")


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_module_loss_and_head_gradients_vs_the_composition(fusion):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    model = _model(fusion)
    fp = prepare(model)
    batch, boxes = _batch()
    seq_w = model.mmt.encoder.spatial_layers[0].output.dense.weight

    def grads(use_fused):
        fp.zero_grad()
        bd = clone_batch(batch)
        model(bd)
        valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], -1).ne(0)
        if use_fused:
            loss = model.spatial_aux_loss(bd)
        else:
            s = bd["spatial_head_out"]
            y = batch["spatial_adj_matrices"]["1"].float()
            m = (valid.unsqueeze(2) & valid.unsqueeze(1)).float()
            loss = (F.binary_cross_entropy_with_logits(s, y, reduction="none").sum(-1) * m).sum() / m.sum().clamp(min=1)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters() if k.startswith(AUX)}, seq_w.grad.clone(), bd

    l_f, g_f, gs_f, bd = grads(True)
    l_c, g_c, gs_c, _ = grads(False)
    assert l_f.dim() == 0 and l_f.dtype == torch.float32
    # the float64 twin on the very O, D the model computed
    o, d = (t.detach() for t in bd["_sam_aux_od"])
    valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], -1).ne(0).to(torch.uint8)
    codes = ops.codes_from_relation_tensor(batch["spatial_adj_matrices"]["1"])
    twin, _ = ops.aux_loss_host(o, d, model.spatial_classifier.weight.detach(), model.spatial_classifier.bias.detach(), codes, valid, fusion)
    e_c, e_f = abs(l_c.item() - twin.item()), abs(l_f.item() - twin.item())
    print("module loss %s: twin %.9g fused err %.3g composition err %.3g" % (fusion, twin.item(), e_f, e_c))
    assert e_f <= 4 * e_c + ULP32 * abs(twin.item())
    # the two routes hand dO / dD that agree to fp32 rounding into the same bf16 GEMM backward: one bf16 ulp of the largest gradient element
    for k in g_f:
        assert float(g_f[k].abs().max()) > 0, k
        within("module grad %s %s" % (k, fusion), rel(g_f[k], g_c[k]), 2.0 ** -8)
    assert float(gs_f.abs().max()) > 0
    within("module MMT grad %s" % fusion, rel(gs_f, gs_c), 2.0 ** -8)


def test_module_without_the_dense_logits_gives_the_same_loss_bits_and_box_batches_work():
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    losses = []
    for mat in (True, False):
        model = _model("mul", materialize_spatial_head_out=mat)
        prepare(model).zero_grad()
        batch, boxes = _batch()
        bd = clone_batch(batch)
        model(bd)
        assert ("spatial_head_out" in bd) == mat
        losses.append(model.spatial_aux_loss(bd).detach().clone())
        model.eval()
        with torch.no_grad():
            bd_e = clone_batch(batch)
            model(bd_e)
        assert tuple(bd_e["spatial_head_out"].shape) == (3, 29, 29, 12)          # decoding forwards produce it whatever the switch says
    assert torch.equal(losses[0], losses[1])
    # a batch that carries boxes in place of relation tensors: the codes come from the boxes, equal to the tensor's
    batch_b, boxes = _batch("boxes")
    assert torch.equal(ops.relation_codes_from_boxes(batch_b["pad_obj_bboxes"], batch_b["pad_ocr_bboxes"]), ops.codes_from_relation_tensor(ops.spatial_relation_tensor(boxes, 1)))
    model.train()
    bd = clone_batch(batch_b)
    model(bd)
    loss = model.spatial_aux_loss(bd)
    o, d = (t.detach() for t in bd["_sam_aux_od"])
    valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], -1).ne(0).to(torch.uint8)
    want, _ = ops.aux_pair_loss(o.contiguous(), d.contiguous(), model.spatial_classifier.weight.data, model.spatial_classifier.bias.data,
                                ops.codes_from_relation_tensor(ops.spatial_relation_tensor(boxes, 1)), valid, "mul")
    assert torch.equal(loss.detach().reshape(1), want) and loss.item() > 0
    loss.backward()
    assert float(model.spatial_classifier.weight.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="use_aux_heads"):
        _model("mul", aux=False).spatial_aux_loss(bd)


def test_ragged_batch_gives_the_padded_batches_loss():
    """obj_count / ocr_count in place of the padded features: the forward writes pad_obj_mask / pad_ocr_mask from the counts and the loss reads them.
    The two forms hold the same fp32 rows, which both reach the encoders as bf16: the losses agree to one bf16 ulp (2^-8 relative) at the worst."""
    from sam_textvqa_amd import ops, ragged as R
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    model = _model("mul")
    prepare(model).zero_grad()
    batch, boxes = _batch()
    bd_p = clone_batch(batch)
    model(bd_p)
    loss_p = model.spatial_aux_loss(bd_p).detach()
    bd_r = R.from_padded(clone_batch(batch), feature_dtype=torch.float32)
    assert "obj_count" in bd_r and "pad_obj_mask" not in bd_r and "pad_ocr_features" not in bd_r
    model(bd_r)
    assert torch.equal(bd_r["pad_obj_mask"].ne(0), batch["pad_obj_mask"].ne(0)) and torch.equal(bd_r["pad_ocr_mask"].ne(0), batch["pad_ocr_mask"].ne(0))
    loss_r = model.spatial_aux_loss(bd_r)
    o, d = (t.detach().contiguous() for t in bd_r["_sam_aux_od"])
    n_ocr = batch["pad_ocr_mask"].size(1)
    valid = torch.cat([torch.ones_like(batch["pad_obj_mask"]), torch.arange(n_ocr, device="cuda").unsqueeze(0) < bd_r["ocr_count"].unsqueeze(1)], 1).to(torch.uint8)
    want, count = ops.aux_pair_loss(o, d, model.spatial_classifier.weight.data, model.spatial_classifier.bias.data,
                                    ops.codes_from_relation_tensor(batch["spatial_adj_matrices"]["1"]), valid, "mul")
    assert torch.equal(loss_r.detach().reshape(1), want) and count.item() == float(((20 + bd_r["ocr_count"].double()) ** 2).sum().item())
    print("ragged %.9g padded %.9g" % (loss_r.item(), loss_p.item()))
    assert abs(loss_r.item() - loss_p.item()) <= 2.0 ** -8 * abs(loss_p.item())
    loss_r.backward()
    assert float(model.origin_transform.logit_fc[0].weight.grad.abs().max()) > 0


def test_decoding_forwards_leave_no_new_key_and_the_loss_refuses_them():
    from sam_textvqa_amd.synthetic import clone_batch
    model = _model("mul").eval()
    batch, _ = _batch()
    bd = clone_batch(batch)
    with torch.no_grad():
        model(bd)
    assert "_sam_aux_od" not in bd and "spatial_head_out" in bd
    with pytest.raises(ValueError, match="training forward"):
        model.spatial_aux_loss(bd)


# ---------------------------------------------------------------------------------------------- torch.ops.sam_hip.*
@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_torch_ops_equal_the_ctypes_route_bit_for_bit(fusion):
    from sam_textvqa_amd import ops, torchops
    ns = torchops.ns()
    o, d, w, bias, codes, valid = _case(70, 31)
    a = _fused(o, d, w, bias, codes, valid, fusion, grad_out=torch.full((1,), 0.5, device="cuda"))
    loss, count = ns.aux_pair_loss(o, d, w, bias, codes, valid, ops.AUX_FUSIONS[fusion])
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    d_o, d_d = ns.aux_pair_loss_bwd(torch.full((1,), 0.5, device="cuda"), count, o, d, w, bias, codes, valid, dw, db, ops.AUX_FUSIONS[fusion], False)
    for x, y in zip(a, (loss, count, d_o, d_d, dw, db)):
        assert torch.equal(x, y)
    d_o2, _ = ns.aux_pair_loss_bwd(None, count, o, d, w, bias, codes, valid, dw, db, ops.AUX_FUSIONS[fusion], True)
    assert torch.equal(d_o2, d_o * 2) and torch.allclose(dw, a[4] * 3, rtol=1e-6, atol=0)          # accumulate adds onto what is there
    boxes = torch.rand(2, 9, 5, generator=torch.Generator().manual_seed(2)).cuda()
    boxes[..., 2:4] += boxes[..., 0:2]
    assert torch.equal(ns.relation_codes_from_boxes(boxes[:, :5], boxes[:, 5:], 0.5), ops.relation_codes_from_boxes(boxes[:, :5], boxes[:, 5:]))
    assert torch.equal(ns.relation_codes_from_boxes(boxes, None, 0.5), ops.relation_codes_from_boxes(boxes))
    with pytest.raises(RuntimeError):
        ns.aux_pair_loss(o, d, w, bias, codes[:, :5], valid, 0)


# ---------------------------------------------------------------------------------------------- Trainer
def _trainer_model(aux=True, dropout=True, seed=0):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"), n_dec=3, T=7, n_obj=20, n_ocr=9)
    td = dict(text_bert_config_dict(), num_hidden_layers=1)
    if not dropout:
        md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0)
        td.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    if aux:
        md.update(use_aux_heads=True)
    torch.manual_seed(seed)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=60, bos_idx=1)


def test_trainer_without_the_weight_is_bit_identical_to_a_trainer_built_without_the_argument():
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    batch, _ = _batch()
    runs = []
    for kw in ({}, {"aux_loss_weight": None}):
        model = _trainer_model()
        tr = Trainer(model, seed=1, **kw)
        losses = [tr.step(clone_batch(batch)) for _ in range(3)]
        torch.cuda.synchronize()
        assert tr.aux_loss() is None
        runs.append((torch.stack(losses), tr.flat.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_trainer_with_the_weight_trains_the_aux_heads():
    import logging
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer, masked_bce_loss
    from sam_textvqa_amd.params import prepare
    batch, _ = _batch()
    model = _trainer_model(dropout=False)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    logging.getLogger("sam_textvqa_amd.trainer").addHandler(handler)
    try:
        tr = Trainer(model, seed=1, aux_loss_weight=0.5, use_graph=True)            # asked for capture: runs eagerly and says so once
        aux0 = [p.detach().clone() for p in model.aux_parameters()]
        total1 = tr.step(clone_batch(batch))
        aux1 = tr.aux_loss().clone()
        g_fused = {k: v.grad.clone() for k, v in model.named_parameters() if k.startswith(AUX)}
        for _ in range(2):
            tr.step(clone_batch(batch))
        torch.cuda.synchronize()
    finally:
        logging.getLogger("sam_textvqa_amd.trainer").removeHandler(handler)
    assert tr._graph is None and sum("eagerly" in r.getMessage() for r in records) == 1
    assert aux1.dim() == 0 and aux1.is_cuda and 0.3 < aux1.item() / 12 < 3.0 and total1.item() > 0.5 * aux1.item()
    assert tr.global_step == 3 and all(not torch.equal(a, p.detach()) for a, p in zip(aux0, model.aux_parameters()))
    ck = tr.state_dict()
    opt_ids = ck["optimizer_state_dict"]["param_groups"][0]["params"]
    g0 = model.get_optimizer_parameters(1e-4)[0]["params"]
    aux_ids = [opt_ids[i] for i, p in enumerate(g0) if any(p is q for q in model.aux_parameters())]
    state = ck["optimizer_state_dict"]["state"]
    assert len(aux_ids) == 14
    for i in aux_ids:
        assert float(state[i]["exp_avg"].abs().max()) > 0 and float(state[i]["exp_avg_sq"].abs().max()) > 0 and int(state[i]["step"]) == 3
    # the first step's aux gradients by the composition route, from the same weights: dense spatial_head_out, torch BCE, sam_aux_pair_bwd
    ref = _trainer_model(dropout=False)
    ref.load_state_dict(sd0)
    ref.cuda().train()
    fp = prepare(ref)
    fp.zero_grad()
    bd = clone_batch(batch)
    ref(bd)
    valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], -1).ne(0)
    m = (valid.unsqueeze(2) & valid.unsqueeze(1)).float()
    comp = (F.binary_cross_entropy_with_logits(bd["spatial_head_out"], batch["spatial_adj_matrices"]["1"].float(), reduction="none").sum(-1) * m).sum() / m.sum().clamp(min=1)
    (masked_bce_loss(bd) + 0.5 * comp).backward()
    torch.cuda.synchronize()
    assert abs(comp.item() - aux1.item()) <= 4 * ULP32 * abs(comp.item()) + ULP32 * abs(comp.item())     # both are fp32 sums of the same logits' BCE
    for k, v in ref.named_parameters():
        if k.startswith(AUX):
            within("trainer step-1 grad %s" % k, rel(g_fused[k], v.grad), 2.0 ** -8)                      # one bf16 ulp, as in the module test


def test_trainer_option_is_checked():
    from sam_textvqa_amd.trainer import Trainer
    with pytest.raises(ValueError, match="use_aux_heads"):
        Trainer(_trainer_model(aux=False), aux_loss_weight=0.5)
    with pytest.raises(ValueError, match="> 0"):
        Trainer(_trainer_model(), aux_loss_weight=0.0)
