"""GPU: sam_aux_targets -- the relation tensor and the padding masks to the aux loss's codes and valid flags in one launch, bit for
bit against the torch twin; the torch op; SAM4C.spatial_aux_loss against the composition it replaces."""
import pytest
import torch

from tests.test_aux_targets_cpu import as_dtype, make_case

pytestmark = pytest.mark.gpu

GUARD, POISON = 0xA5, 0x7F
SHAPES = [(3, 5, 4), (2, 100, 50), (1, 1, 0)]          # 243 pairs (not a multiple of 4, odd n) | the workload's n | the smallest shape


def run_guarded(rel, om, cm):
    """ops.aux_targets with its outputs allocated inside guard bytes: -> (codes or None, valid), after checking the bytes behind them"""
    from sam_textvqa_amd import _capi as capi, ops
    om, ld_obj = ops._aux_mask_rows(om, "obj_mask")
    cm, ld_ocr = ops._aux_mask_rows(cm, "ocr_mask")
    b, n_obj, n_ocr = om.shape[0], om.shape[1], cm.shape[1]
    n = n_obj + n_ocr
    pad = 64
    vbuf = torch.full((b * n + pad,), GUARD, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((b * n * n + pad,), GUARD, dtype=torch.uint8, device="cuda")
    capi.call("sam_aux_targets", capi.ptr(rel), capi.ptr(om) if n_obj else None, ld_obj, n_obj, capi.ptr(cm) if n_ocr else None, ld_ocr, n_ocr, om.element_size(),
              b, n, capi.ptr(cbuf) if rel is not None else None, capi.ptr(vbuf), capi.stream_handle())
    torch.cuda.synchronize()
    assert bool((vbuf[b * n:] == GUARD).all()), "bytes behind valid were written"
    assert bool((cbuf[b * n * n if rel is not None else 0:] == GUARD).all()), "bytes behind codes were written"
    return (cbuf[:b * n * n].view(b, n, n) if rel is not None else None), vbuf[:b * n].view(b, n)


def at_offset(rel, off):
    """the same tensor at `off` bytes into a larger int8 buffer whose base is 16-byte aligned"""
    buf = torch.zeros(rel.numel() + 32, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[off: off + rel.numel()].view(rel.shape)
    out.copy_(rel)
    assert out.data_ptr() % 16 == off and out.is_contiguous()
    return out


@pytest.mark.parametrize("off", [0, 4, 1])
@pytest.mark.parametrize("b,n_obj,n_ocr", SHAPES)
def test_kernel_equals_the_twin_bit_for_bit(b, n_obj, n_ocr, off):
    """every shape at the three alignments of `rel` (16-byte loads, dword loads, byte loads), every mask dtype, poisoned invalid pairs, guard bytes"""
    from sam_textvqa_amd import ops
    rel, om, cm = make_case(b, n_obj, n_ocr, seed=7 + b)
    if n_obj + n_ocr == 1:
        om[:] = 3
    want_codes, want_valid = ops.aux_targets_host(rel, om, cm)
    pair = (want_valid.unsqueeze(2) & want_valid.unsqueeze(1)).bool()
    if b > 1:
        assert not bool(want_valid[-1].any()) and bool(((rel.sum(-1) > 1) & pair).any())       # an all-invalid sample and multi-hot rows are in the case
    poisoned = rel.clone()
    poisoned[~pair] = POISON                                    # the 12 bytes of a pair with an invalid row may hold anything
    for src in (rel, poisoned):
        dev = at_offset(src.cuda(), off)
        for dtype in (torch.bool, torch.uint8, torch.int32, torch.int64):
            codes, valid = run_guarded(dev, as_dtype(om, dtype).cuda(), as_dtype(cm, dtype).cuda())
            assert torch.equal(valid.cpu(), want_valid), dtype
            assert torch.equal(codes.cpu(), want_codes), (dtype, off)
    # the public wrapper allocates its own outputs: same bytes
    codes, valid = ops.aux_targets(at_offset(rel.cuda(), off), om.cuda(), cm.cuda())
    assert codes.dtype == valid.dtype == torch.uint8 and torch.equal(codes.cpu(), want_codes) and torch.equal(valid.cpu(), want_valid)


@pytest.mark.parametrize("b,n_obj,n_ocr", SHAPES)
def test_strided_masks_and_no_relation_tensor(b, n_obj, n_ocr):
    from sam_textvqa_amd import ops
    rel, om, cm = make_case(b, n_obj, n_ocr, seed=11)
    want_codes, want_valid = ops.aux_targets_host(rel, om, cm)
    wide = torch.full((b, n_obj + n_ocr + 7), 9, dtype=torch.int64)           # the masks as column slices of one wider tensor: non-zero all around them
    wide[:, 2: 2 + n_obj], wide[:, 2 + n_obj: 2 + n_obj + n_ocr] = om, cm
    wide = wide.cuda()
    so, sc = wide[:, 2: 2 + n_obj], wide[:, 2 + n_obj: 2 + n_obj + n_ocr]
    assert b == 1 or not so.is_contiguous()
    codes, valid = run_guarded(rel.cuda(), so, sc)
    assert torch.equal(codes.cpu(), want_codes) and torch.equal(valid.cpu(), want_valid)
    none, valid = run_guarded(None, so, sc)                       # rel = NULL: only valid is written (the guard check covers all of the codes buffer)
    assert none is None and torch.equal(valid.cpu(), want_valid)
    none, valid = ops.aux_targets(None, so.to(torch.int32), sc.to(torch.int32))
    assert none is None and torch.equal(valid.cpu(), want_valid)


def test_wrapper_rejects_what_the_kernel_does_not_take():
    from sam_textvqa_amd import _capi as capi, ops
    rel, om, cm = (t.cuda() for t in make_case(2, 5, 4, seed=1))
    with pytest.raises(capi.SamHipError):
        ops.aux_targets(rel, om.float(), cm.float())
    with pytest.raises(capi.SamHipError):
        ops.aux_targets(rel, om, cm.to(torch.int32))
    with pytest.raises(capi.SamHipError):
        ops.aux_targets(rel[:, :8], om, cm)
    with pytest.raises(capi.SamHipError):
        ops.aux_targets(rel.to(torch.int16), om, cm)
    assert ops.aux_targets_fusable(rel, om, cm) and not ops.aux_targets_fusable(rel, om.float(), cm.float()) and not ops.aux_targets_fusable(rel.long(), om, cm)


# ---------------------------------------------------------------------------------------------- torch.ops.sam_hip.*
@pytest.mark.parametrize("b,n_obj,n_ocr", SHAPES)
def test_torch_op_equals_the_ctypes_route_bit_for_bit(b, n_obj, n_ocr):
    from sam_textvqa_amd import ops, torchops
    ns = torchops.ns()
    rel, om, cm = (t.cuda() for t in make_case(b, n_obj, n_ocr, seed=5))
    for dtype in (torch.bool, torch.int64):
        o, c = as_dtype(om, dtype), as_dtype(cm, dtype)
        codes, valid = ops.aux_targets(rel, o, c)
        t_codes, t_valid = ns.aux_targets(rel, o, c)
        assert t_codes.dtype == torch.uint8 and torch.equal(t_codes, codes) and torch.equal(t_valid, valid)
        e_codes, e_valid = ns.aux_targets(None, o, c)               # no relation tensor: the codes come back empty, as the file's other absent outputs
        assert e_codes.numel() == 0 and torch.equal(e_valid, valid)
    with pytest.raises(RuntimeError):
        ns.aux_targets(rel, om.float(), cm.float())
    with pytest.raises(RuntimeError):
        ns.aux_targets(rel.to(torch.int16), om, cm)


# ---------------------------------------------------------------------------------------------- SAM4C.spatial_aux_loss
AUX = ("origin_transform", "dest_transform", "spatial_classifier")


@pytest.mark.parametrize("spatial", ["adjacency", "boxes"])
@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_module_loss_and_gradients_equal_the_old_composition_bit_for_bit(fusion, spatial, monkeypatch):
    """spatial_aux_loss through the one launch against autograd.aux_pair_loss fed by codes_from_relation_tensor and the torch `valid`: the loss, the three
    heads' gradients and mmt_seq_output's are torch.equal (the routes differ only in the codes of pairs the loss kernels never read)"""
    from sam_textvqa_amd import autograd, ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    from tests.test_aux_loss_gpu import _batch, _model
    model = _model(fusion)
    fp = prepare(model)
    batch, boxes = _batch(spatial)
    assert bool((batch["pad_ocr_mask"] == 0).any())                # padded rows: the two routes' codes differ
    launches = []
    real = ops.aux_targets
    monkeypatch.setattr(ops, "aux_targets", lambda *a: (launches.append(a[0] is None), real(*a))[1])

    def run(new):
        fp.zero_grad()
        bd = clone_batch(batch)
        model(bd)
        seq = bd["mmt_seq_output"]
        seq.retain_grad()
        if new:
            loss = model.spatial_aux_loss(bd)
        else:
            o, d = bd["_sam_aux_od"]
            valid = torch.cat([bd["pad_obj_mask"], bd["pad_ocr_mask"]], dim=-1).ne(0).to(torch.uint8)
            rel = bd["spatial_adj_matrices"]["1"] if spatial == "adjacency" else ops.spatial_relation_tensor(boxes, 1)
            codes = ops.codes_from_relation_tensor(rel, check=False).contiguous()
            loss = autograd.aux_pair_loss(o, d, model.spatial_classifier, codes, valid, model.aux_spatial_fusion)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters() if k.startswith(AUX)}, seq.grad.clone()

    l_new, g_new, s_new = run(True)
    assert launches == [spatial == "boxes"]                        # the one launch, without a relation tensor for a batch from boxes
    l_old, g_old, s_old = run(False)
    assert l_new.item() > 0 and torch.equal(l_new, l_old)
    assert len(g_new) == 14 and all(float(g.abs().max()) > 0 for g in g_new.values())
    for k in g_new:
        assert torch.equal(g_new[k], g_old[k]), k
    assert float(s_new.abs().max()) > 0 and torch.equal(s_new, s_old)


def test_float_masks_and_cpu_relations_keep_the_torch_route(monkeypatch):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    from tests.test_aux_loss_gpu import _batch, _model
    model = _model("mul")
    prepare(model).zero_grad()
    batch, _ = _batch()
    monkeypatch.setattr(ops, "aux_targets", lambda *a: pytest.fail("the fused launch was taken"))
    bd = clone_batch(batch)
    model(bd)
    want = None
    for change in ("float", "cpu"):
        b2 = dict(bd)
        if change == "float":
            b2["pad_obj_mask"], b2["pad_ocr_mask"] = bd["pad_obj_mask"].float(), bd["pad_ocr_mask"].float()
        else:
            b2["spatial_adj_matrices"] = dict(bd["spatial_adj_matrices"], **{"1": bd["spatial_adj_matrices"]["1"].cpu()})
        loss = model.spatial_aux_loss(b2).detach().clone()
        want = loss if want is None else want
        assert loss.item() > 0 and torch.equal(loss, want)
    b3 = dict(bd, spatial_adj_matrices={"1": bd["spatial_adj_matrices"]["1"][:, :5]})
    with pytest.raises(ValueError, match="relations of shape"):
        model.spatial_aux_loss(b3)
