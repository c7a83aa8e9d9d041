"""CPU: the spatial aux heads' loss without a GPU -- relation codes <-> the 12-channel tensor on the reference's own graphs, the
float64 host twin against torch's BCE-with-logits on the reference's spatial_head_out, the C ABI's argument checks and the binding."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import common as C
from tests.test_aux_heads_cpu import GOLDEN_SHAPES, forward_aux_ref, golden, golden_params, simple_classifier_ref

GRAPHS = ("known6", "grid", "rnd60", "cross")


def spatial_golden():
    return np.load(os.path.join(C.GOLDEN_DIR, "spatial_graph.npz"))


# ---------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("name", GRAPHS)
def test_codes_and_the_relation_tensor_round_trip_on_the_reference_graphs(name):
    from sam_textvqa_amd import ops
    g = spatial_golden()
    adj = torch.from_numpy(g[name + ".ctx1"])                      # torch_broadcast_adj_matrix of the reference's own adjacency
    code = torch.from_numpy(g[name + ".code1"]).to(torch.uint8)    # the adjacency itself
    got = ops.codes_from_relation_tensor(adj)
    assert got.dtype == torch.uint8 and torch.equal(got, code)
    assert torch.equal(got, (adj.long() * torch.arange(1, 13)).sum(-1).to(torch.uint8))
    back = ops.relation_tensor_from_codes(got)
    assert back.dtype == torch.int8 and torch.equal(back, adj)
    assert bool((code == 0).any()) and bool((back[code == 0] == 0).all())          # a zero code is an all-zero row


def test_bad_codes_and_tensors_raise_value_error():
    from sam_textvqa_amd import ops
    assert torch.equal(ops.relation_tensor_from_codes(torch.tensor([0, 12], dtype=torch.uint8)).sum(-1), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="13"):
        ops.relation_tensor_from_codes(torch.tensor([[1, 13]], dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.check_relation_codes(torch.tensor([1], dtype=torch.int64))
    ctx3 = torch.from_numpy(spatial_golden()["rnd60.ctx3"])        # a wider context sets neighbouring sectors too: not a one-hot
    with pytest.raises(ValueError, match="one-hot"):
        ops.codes_from_relation_tensor(ctx3)
    with pytest.raises(ValueError):
        ops.codes_from_relation_tensor(torch.zeros(3, 3, 11, dtype=torch.int8))


# ---------------------------------------------------------------------------------------------- host twin
def _golden_scores(fusion):
    """(O, D, W, bias, S) in float64 from the golden's hidden rows and parameters; S is checked against the reference's recorded spatial_head_out"""
    g = golden()
    p = {k: v.double() for k, v in golden_params(GOLDEN_SHAPES).items()}
    seq = torch.from_numpy(g["seq"]).double()
    t0, n = 4, 150                                                  # the golden's layout: 4 text rows | 150 object / OCR rows | decoder rows
    s = forward_aux_ref(seq, p, t0, n, fusion)
    ref = torch.from_numpy(g[fusion + ".out"]).double()
    assert ((s[:, list(g["rows"])] - ref).abs().max() / ref.abs().max()).item() < 1e-5         # the reference ran in fp32
    x = seq[:, t0: t0 + n]
    return (simple_classifier_ref(x, p, "origin_transform"), simple_classifier_ref(x, p, "dest_transform"), p["spatial_classifier.weight"],
            p["spatial_classifier.bias"], s)


def _labels(b, n, seed):
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 13, (b, n, n), generator=gen).to(torch.uint8)
    valid = (torch.rand(b, n, generator=gen) < 0.7).to(torch.uint8)
    return codes, valid


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_host_twin_equals_torch_bce_on_the_reference_scores(fusion):
    from sam_textvqa_amd import ops
    o, d, w, bias, s = _golden_scores(fusion)
    b, n = o.shape[:2]
    codes, valid = _labels(b, n, 3)
    if b > 1:
        valid[-1] = 0                                               # one sample entirely padded
    y = (codes.unsqueeze(-1).long() == torch.arange(1, 13)).double()
    m = (valid.bool().unsqueeze(2) & valid.bool().unsqueeze(1)).double()
    want = (F.binary_cross_entropy_with_logits(s, y, reduction="none").sum(-1) * m).sum() / m.sum().clamp(min=1)
    loss, count = ops.aux_loss_host(o, d, w, bias, codes, valid, fusion)
    assert loss.dtype == torch.float64 and count.item() == m.sum().item() and count.item() > 0
    assert abs(loss.item() - want.item()) <= 1e-13 * abs(want.item())
    assert 0.3 < loss.item() / 12 < 3.0                             # per-logit BCE of untrained heads: of the order of log 2


def test_host_twin_all_padded_is_zero_and_ignores_the_padded_rows():
    from sam_textvqa_amd import ops
    gen = torch.Generator().manual_seed(0)
    o, d = torch.randn(2, 9, 32, generator=gen).double(), torch.randn(2, 9, 32, generator=gen).double()
    w, bias = torch.randn(12, 32, generator=gen).double(), torch.randn(12, generator=gen).double()
    codes, valid = _labels(2, 9, 1)
    loss, count = ops.aux_loss_host(o, d, w, bias, codes, torch.zeros_like(valid), "mul")
    assert loss.item() == 0.0 and count.item() == 0.0
    ref, _ = ops.aux_loss_host(o, d, w, bias, codes, valid, "add")
    o2, d2 = o.clone(), d.clone()
    o2[valid == 0], d2[valid == 0] = float("nan"), 1e30
    got, _ = ops.aux_loss_host(o2, d2, w, bias, codes, valid, "add")
    assert got.item() == ref.item()
    with pytest.raises(ValueError):
        ops.aux_loss_host(o, d, w, bias, torch.full_like(codes, 13), valid, "mul")


# ---------------------------------------------------------------------------------------------- C ABI
def test_loss_entry_points_are_bound_and_reject_bad_arguments_without_a_gpu():
    import ctypes
    from sam_textvqa_amd import _build, _capi, ops
    names = ["sam_aux_pair_loss_fwd_ws_bytes", "sam_aux_pair_loss_fwd", "sam_aux_pair_loss_bwd_ws_bytes", "sam_aux_pair_loss_bwd", "sam_relation_codes_from_boxes"]
    assert list(_capi.PART_SIGNATURES) == list(_build.ABI_PARTS) == ["aux_loss"] and list(_capi.PART_SIGNATURES["aux_loss"]) == names
    assert not set(names) & set(_capi.SIGNATURES) and all(not set(names) & set(t) for t in _capi.HEADER_SIGNATURES.values())
    assert _capi.PART_VALUES == {names[0], names[2]} and not set(names) & _capi.NO_STATUS
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _capi.PART_SIGNATURES["aux_loss"]["sam_aux_pair_loss_bwd"] == [vp] * 8 + [i] * 3 + [vp] * 4 + [i, vp, ctypes.c_int64, vp]
    assert '#include "sam_hip_aux_loss.h"' in open(_build.HEADER).read()           # a C caller gets them from sam_hip.h
    lib = _capi.lib()
    assert lib.sam_aux_pair_loss_fwd.argtypes == _capi.PART_SIGNATURES["aux_loss"]["sam_aux_pair_loss_fwd"] and lib.sam_aux_pair_loss_fwd_ws_bytes.restype is ctypes.c_int64
    assert _capi.call("sam_aux_pair_loss_fwd_ws_bytes", 64, 150) == 64 * 3 * 10 * 8
    assert _capi.call("sam_aux_pair_loss_bwd_ws_bytes", 64, 150) == _capi.call("sam_aux_pair_bwd_ws_bytes", 64, 150)
    assert _capi.call("sam_aux_pair_loss_fwd_ws_bytes", 0, 150) == 0 and _capi.call("sam_aux_pair_loss_bwd_ws_bytes", 3, -1) == 0
    fake = 1 << 20            # never dereferenced: the checks reject the call before any launch
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_aux_pair_loss_fwd", fake, fake, fake, fake, None, fake, 2, 5, 0, fake, fake, fake, 1 << 20, None)
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_aux_pair_loss_bwd", None, None, fake, fake, fake, fake, fake, fake, 2, 5, 0, fake, fake, fake, fake, 1, fake, 1 << 20, None)
    for b, n in ((0, 5), (-1, 5), (2, 0)):
        with pytest.raises(_capi.SamHipError, match="empty shape"):
            _capi.call("sam_aux_pair_loss_fwd", fake, fake, fake, fake, fake, fake, b, n, 0, fake, fake, fake, 1 << 20, None)
        with pytest.raises(_capi.SamHipError, match="empty shape"):
            _capi.call("sam_aux_pair_loss_bwd", None, fake, fake, fake, fake, fake, fake, fake, b, n, 0, fake, fake, fake, fake, 1, fake, 1 << 20, None)
    with pytest.raises(_capi.SamHipError, match="unknown fusion"):
        _capi.call("sam_aux_pair_loss_fwd", fake, fake, fake, fake, fake, fake, 2, 5, 2, fake, fake, fake, 1 << 20, None)
    with pytest.raises(_capi.SamHipError, match="unknown fusion"):
        _capi.call("sam_aux_pair_loss_bwd", None, fake, fake, fake, fake, fake, fake, fake, 2, 5, -1, fake, fake, fake, fake, 1, fake, 1 << 20, None)
    with pytest.raises(_capi.SamHipError, match="workspace"):
        _capi.call("sam_aux_pair_loss_fwd", fake, fake, fake, fake, fake, fake, 2, 150, 0, fake, fake, fake, 16, None)
    with pytest.raises(_capi.SamHipError, match="workspace"):
        _capi.call("sam_aux_pair_loss_bwd", None, fake, fake, fake, fake, fake, fake, fake, 2, 150, 0, fake, fake, fake, fake, 1, fake, 16, None)
    with pytest.raises(_capi.SamHipError, match="null pointer"):
        _capi.call("sam_relation_codes_from_boxes", None, 5, 3, None, 0, 0, 0, 2, 0.5, fake, None)
    with pytest.raises(_capi.SamHipError, match="empty batch"):
        _capi.call("sam_relation_codes_from_boxes", fake, 5, 3, None, 0, 0, 0, 0, 0.5, fake, None)
    with pytest.raises(_capi.SamHipError, match="stride"):
        _capi.call("sam_relation_codes_from_boxes", fake, 3, 3, None, 0, 0, 0, 2, 0.5, fake, None)
    with pytest.raises(_capi.SamHipError, match="ocr_boxes is NULL"):
        _capi.call("sam_relation_codes_from_boxes", fake, 5, 3, None, 5, 4, 0, 2, 0.5, fake, None)
    # the Python wrappers: CPU tensors are refused, no fallback
    o = torch.zeros(2, 5, 32)
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_loss(o, o, torch.zeros(12, 32), torch.zeros(12), torch.zeros(2, 5, 5, dtype=torch.uint8), torch.ones(2, 5, dtype=torch.uint8))
    with pytest.raises(_capi.SamHipError):
        ops.relation_codes_from_boxes(torch.zeros(2, 5, 5))


def test_module_surface_without_a_gpu():
    import inspect
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    assert inspect.signature(M.SAM4C.__init__).parameters["materialize_spatial_head_out"].default is True
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3, ("n", "s"))), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1)), num_answers=50, bos_idx=1)
    with pytest.raises(ValueError, match="use_aux_heads"):
        model.spatial_aux_loss({})


def test_torch_ops_are_registered_without_a_gpu():
    from sam_textvqa_amd import torchops
    ns = torchops.ns()
    for op in ("aux_pair_loss", "aux_pair_loss_bwd", "relation_codes_from_boxes"):
        assert hasattr(ns, op), op
    schema = str(torch.ops.sam_hip.aux_pair_loss_bwd.default._schema)
    assert "Tensor? grad_out" in schema and "Tensor(a!) dw" in schema and "bool accumulate" in schema


def test_trainer_rejects_the_weight_without_aux_heads_or_not_positive():
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    import inspect
    assert inspect.signature(Trainer.__init__).parameters["aux_loss_weight"].default is None
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3, ("n", "s"))), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1)), num_answers=50, bos_idx=1)
    with pytest.raises(ValueError, match="use_aux_heads"):
        Trainer(model, aux_loss_weight=0.5)
    with pytest.raises(ValueError, match="> 0"):
        Trainer(model, aux_loss_weight=-1.0)
