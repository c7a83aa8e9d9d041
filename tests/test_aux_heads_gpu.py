"""GPU: the spatial auxiliary heads (use_aux_heads, sam/sa_m4c.py:173-177, 316-347) on the MI355X -- the pair kernels (csrc/aux_heads.hip) against fp64
torch math on the same operands, the module against the reference golden, the whole model against the fp32 oracle's encoder rows, greedy / beam
decoding, the Trainer (aux parameters never move, carry no optimizer state, sit inside the reducer's head region)."""
import os

import numpy as np
import pytest
import torch

from oracle import sa_m4c_oracle as O
from tests.golden import common as C
from tests.test_aux_heads_cpu import AUX, GOLDEN_SHAPES, forward_aux_ref, golden, golden_params, pair_ref

pytestmark = pytest.mark.gpu

# limits: about twice what the path achieves (printed by every comparison)
L = dict(pair_fwd=7e-7, pair_bwd=1e-6,                                     # achieved 3.2e-7 / 4.3e-7 (fp32 vs fp64)
         golden_out=0.007, golden_dseq=0.015, golden_pgrad=0.013,           # 0.29 % / 0.71 % / 0.62 %: bf16 GEMM operands inside SimpleClassifier
         model_out=0.03, model_pgrad=0.035)                                 # 1.44 % / 1.69 %: + the bf16 encoder rows of the whole model


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def within(name, err, limit):
    print("%-40s rel err %.3g (limit %.3g)" % (name, err, limit))
    assert err <= limit, (name, err, limit)


# ---------------------------------------------------------------------------------------------- kernels
def _operands(b, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    o = torch.randn(b, n, 32, generator=g)
    d = torch.randn(b, n, 32, generator=g)
    w = torch.randn(12, 32, generator=g) * 0.2
    bias = torch.randn(12, generator=g) * 0.1
    gup = torch.randn(b, n, n, 12, generator=g)
    return [t.cuda() for t in (o, d, w, bias, gup)]


@pytest.mark.parametrize("fusion", ["mul", "add"])
@pytest.mark.parametrize("n", [1, 37, 150, 200])
@pytest.mark.parametrize("b", [1, 3, 64])
def test_pair_kernels_vs_fp64_math(fusion, n, b):
    from sam_textvqa_amd import ops
    o, d, w, bias, gup = _operands(b, n, 1000 * n + b)
    out = ops.aux_pair_fwd(o, d, w, bias, fusion)
    od, dd, wd, bd = (t.double().requires_grad_(True) for t in (o, d, w, bias))
    ref = pair_ref(od, dd, wd, bd, fusion)
    within("pair fwd %s n=%d B=%d" % (fusion, n, b), rel(out, ref), L["pair_fwd"])
    (ref * gup.double()).sum().backward()
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    d_o, d_d = ops.aux_pair_bwd(gup, o, d, w, dw, db, fusion, accumulate=False)
    for name, got, r in (("dO", d_o, od.grad), ("dD", d_d, dd.grad), ("dW", dw, wd.grad), ("dbias", db, bd.grad)):
        within("pair bwd %s %s n=%d B=%d" % (name, fusion, n, b), rel(got, r), L["pair_bwd"])
    # accumulate adds onto what is there
    dw2, db2 = dw.clone(), db.clone()
    ops.aux_pair_bwd(gup, o, d, w, dw2, db2, fusion, accumulate=True)
    assert torch.allclose(dw2, 2 * dw, rtol=1e-6, atol=0) and torch.allclose(db2, 2 * db, rtol=1e-6, atol=0)


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_pair_backward_is_bit_identical_across_runs_and_cu_reserve(fusion):
    from sam_textvqa_amd import ops
    o, d, w, bias, gup = _operands(64, 150, 7)

    def run():
        dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
        d_o, d_d = ops.aux_pair_bwd(gup, o, d, w, dw, db, fusion, accumulate=False)
        return [t.clone() for t in (ops.aux_pair_fwd(o, d, w, bias, fusion), d_o, d_d, dw, db)]

    a, b = run(), run()
    was = ops.cu_reserve()
    ops.set_cu_reserve(32)
    try:
        c = run()
    finally:
        ops.set_cu_reserve(was)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_pair_wrappers_reject_bad_shapes():
    from sam_textvqa_amd import _capi, ops
    o = torch.zeros(2, 5, 32, device="cuda")
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_fwd(o, torch.zeros(2, 6, 32, device="cuda"), torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda"))
    with pytest.raises(_capi.SamHipError):
        ops.aux_pair_fwd(torch.zeros(2, 0, 32, device="cuda"), torch.zeros(2, 0, 32, device="cuda"), torch.zeros(12, 32, device="cuda"),
                         torch.zeros(12, device="cuda"))


# ---------------------------------------------------------------------------------------------- module vs the reference golden
def _golden_heads(fusion):
    """the golden's three heads at hidden size 32 on this package's modules, driven by SAM4C._forward_aux itself"""
    import sam_textvqa_amd.modules as M
    from torch import nn

    class Heads(M._HipModule):
        _forward_aux = M.SAM4C._forward_aux

    heads = Heads()
    heads.origin_transform = M.SimpleClassifier(32, 128, 32)
    heads.dest_transform = M.SimpleClassifier(32, 128, 32)
    heads.spatial_classifier = nn.Linear(32, 12)
    heads.aux_spatial_fusion = fusion
    params = golden_params(GOLDEN_SHAPES)
    with torch.no_grad():
        for n, p in heads.named_parameters():
            p.copy_(params[n])
    return heads.cuda(), golden()


@pytest.mark.parametrize("fusion", ["mul", "add"])
def test_module_vs_reference_golden(fusion):
    from sam_textvqa_amd.params import prepare
    model, g = _golden_heads(fusion)
    fp = prepare(model)
    fp.zero_grad()
    seq = torch.from_numpy(g["seq"]).cuda().to(torch.bfloat16).requires_grad_(True)       # the MMT hands its rows over in bf16
    b = seq.shape[0]
    bd = {"question_mask": torch.ones(b, 4, device="cuda"), "pad_obj_mask": torch.ones(b, 100, device="cuda"),
          "pad_ocr_mask": torch.ones(b, 50, device="cuda"), "mmt_seq_output": seq}
    model._forward_aux(bd)
    out = bd["spatial_head_out"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (b, 150, 150, 12)
    ref = torch.from_numpy(g[fusion + ".out"])
    within("golden out %s" % fusion, rel(out[:, list(g["rows"])], ref), L["golden_out"])
    gup = torch.from_numpy(C.det_uniform("aux.G", tuple(out.shape))).cuda()
    (out * gup).sum().backward()
    within("golden d_seq %s" % fusion, rel(seq.grad.float(), torch.from_numpy(g[fusion + ".d_seq"])), L["golden_dseq"])
    for n, p in model.named_parameters():
        if n.startswith(AUX):
            within("golden grad %s %s" % (n, fusion), rel(p.grad, torch.from_numpy(g[fusion + ".g." + n])), L["golden_pgrad"])


# ---------------------------------------------------------------------------------------------- whole model
def _aux_model(ctx, layers, shapes, fusion="mul", vocab=300, seed=0, aux=True):
    """(hip model with aux heads, fp32 oracle) sharing every weight; dropout off (tests/test_model_gpu.py::_small_full_model plus the heads)"""
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    T, n_obj, n_ocr, n_dec = shapes
    md = mmt_config_dict(ctx, layers, n_dec=n_dec, T=T, n_obj=n_obj, n_ocr=n_ocr)
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=500)
    torch.manual_seed(seed)
    ref = O.SAM4C(O.BertConfig.from_dict(md), O.BertConfig.from_dict(td), num_answers=vocab)
    with torch.no_grad():
        for _, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    if aux:
        md.update(use_aux_heads=True, aux_spatial_fusion=fusion)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=vocab, bos_idx=1)
    sd = dict(model.state_dict())
    sd.update(ref.state_dict())
    if aux:
        gen = torch.Generator().manual_seed(seed + 1)
        for k in sd:
            if k.startswith(AUX):
                sd[k] = (1.0 + 0.1 * torch.randn(sd[k].shape, generator=gen)) if ("logit_fc.2" in k and k.endswith("weight")) else \
                    0.1 * torch.randn(sd[k].shape, generator=gen)
    model.load_state_dict(sd)
    return model, ref


def _batch(shapes, batch=3, vocab=300, ctx=3, seed=11):
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(batch, *shapes, vocab=vocab, context=ctx, device="cpu", seed=seed)
    bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
    return bd


def _cuda(bd):
    return {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in bd.items()}


@pytest.mark.parametrize("fusion,shapes", [("mul", (20, 100, 50, 12)), ("add", (13, 37, 21, 5)), ("mul", (7, 20, 9, 3))])
def test_whole_model_aux_vs_restatement_on_oracle_rows(fusion, shapes):
    """training forward: spatial_head_out and the aux parameter gradients of a user loss on it vs the fp32 restatement applied to the ORACLE's
    last-layer rows (n = 150, and two n != 150); with that loss added to the TextVQA loss the gradient reaches the MMT"""
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import masked_bce_loss
    model, ref = _aux_model(3, ("n", "s"), shapes, fusion)
    bd_cpu = _batch(shapes)
    ref.train()
    rbd = clone_batch(bd_cpu)
    ref(rbd)
    T, n = shapes[0], shapes[1] + shapes[2]
    p = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items() if k.startswith(AUX)}
    seq_o = rbd["mmt_seq_output"].detach().double()
    out_ref = forward_aux_ref(seq_o, p, T, n, fusion)
    model.cuda().train()
    fp = prepare(model)
    fp.zero_grad()
    bd = _cuda(bd_cpu)
    model(bd)
    out = bd["spatial_head_out"]
    assert tuple(out.shape) == (3, n, n, 12) and out.dtype == torch.float32 and out.requires_grad
    within("model out %s n=%d" % (fusion, n), rel(out, out_ref), L["model_out"])
    gup = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (out_ref * gup.double()).sum().backward()
    loss_aux = (out * gup.cuda()).sum() * 1e-3
    mmt_w = model.mmt.encoder.spatial_layers[0].output.dense.weight
    loss = masked_bce_loss(bd) + loss_aux
    loss.backward()
    torch.cuda.synchronize()
    for k, v in model.named_parameters():
        if k.startswith(AUX):
            within("model grad %s %s" % (k, fusion), rel(v.grad / 1e-3, p[k].grad), L["model_pgrad"])
    g_with = mmt_w.grad.clone()
    # the same step without the aux loss: the MMT's gradient differs -> the aux loss reached the MMT rows
    fp.zero_grad()
    bd = _cuda(bd_cpu)
    model(bd)
    masked_bce_loss(bd).backward()
    torch.cuda.synchronize()
    assert not torch.equal(g_with, mmt_w.grad)
    assert all(bool((v.grad == 0).all()) for k, v in model.named_parameters() if k.startswith(AUX))   # TextVQA loss alone: aux heads get nothing


# ---------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("fused", ["0", "1"])
def test_greedy_decoding_sets_spatial_head_out_and_leaves_scores_unchanged(fused, monkeypatch):
    monkeypatch.setenv("SAM_DECODE_FUSED", fused)
    shapes = (20, 100, 50, 12)
    model, _ = _aux_model(3, ("n", "s"), shapes)
    plain, _ = _aux_model(3, ("n", "s"), shapes, aux=False)
    bd_cpu = _batch(shapes)
    model.cuda()
    plain.cuda()
    with torch.no_grad():
        model.train()                                 # dropout is off in this config: the training forward's encoder rows are the eval ones
        bd_t = _cuda(bd_cpu)
        model(bd_t)
        model.eval()
        bd_e = _cuda(bd_cpu)
        scores = model(bd_e)["textvqa_scores"]
        plain.eval()
        scores_plain = plain(_cuda(bd_cpu))["textvqa_scores"]
    torch.cuda.synchronize()
    out_e, out_t = bd_e["spatial_head_out"], bd_t["spatial_head_out"]
    assert tuple(out_e.shape) == (3, 150, 150, 12)
    within("greedy (fused=%s) vs training forward" % fused, rel(out_e, out_t), 1e-5)
    assert torch.equal(scores, scores_plain)


def test_beam_search_emits_one_row_per_sample(monkeypatch):
    from sam_textvqa_amd.registry import registry
    monkeypatch.setattr(registry, "EOS_IDX", 2, raising=False)
    shapes = (20, 100, 50, 12)
    model, _ = _aux_model(3, ("n", "s"), shapes)
    bd_cpu = _batch(shapes, batch=2)
    model.cuda().eval()
    with torch.no_grad():
        bd_g = _cuda(bd_cpu)
        model(bd_g)
        model.set_beam_size(3)
        bd_b = _cuda(bd_cpu)
        model(bd_b, use_beam_search=True)
    torch.cuda.synchronize()
    assert tuple(bd_b["spatial_head_out"].shape) == (2, 150, 150, 12)
    within("beam vs greedy spatial_head_out", rel(bd_b["spatial_head_out"], bd_g["spatial_head_out"]), 1e-5)


# ---------------------------------------------------------------------------------------------- trainer
def _trainer_model(aux):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"))
    if aux:
        md.update(use_aux_heads=True)
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1)), num_answers=200, bos_idx=1)
    return model


def test_trainer_leaves_aux_params_alone_and_tracks_the_run_without_them(tmp_path):
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    from sam_textvqa_amd.trainer import Trainer
    plain, withaux = _trainer_model(False), _trainer_model(True)
    sd = withaux.state_dict()
    sd.update(plain.state_dict())
    withaux.load_state_dict(sd)
    aux0 = [p.detach().clone() for p in withaux.aux_parameters()]
    assert len(aux0) == 14
    batch = make_batch(4, vocab=200, device="cuda", seed=3)
    tp = Trainer(plain, seed=1)                                   # (each Trainer re-seeds the dropout clock: build the second after the first has run)
    lp = [tp.step(clone_batch(batch)).item() for _ in range(3)]
    ta = Trainer(withaux, seed=1)
    la = [ta.step(clone_batch(batch)).item() for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(aux0, withaux.aux_parameters()):
        assert torch.equal(a, b.detach().cpu())                   # g = m = v = 0: Adam's update is exactly 0
    assert float(ta.exp_avg.abs().sum()) > 0
    names_a = dict(withaux.named_parameters())
    worst = 0.0
    for n, p in plain.named_parameters():
        q = names_a[n].detach()
        worst = max(worst, ((q - p.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30)).item())
    print("losses", lp, la, "worst param rel diff %.3g" % worst)
    # the aux ranges move the MMT group's offsets: the gradient-norm reduction may sum in another order (a few ulps of the clip factor)
    assert worst <= 1e-5 and all(abs(x - y) <= 1e-5 * abs(x) for x, y in zip(lp, la)), (worst, lp, la)
    # checkpoint: no optimizer state for the aux parameters, global_step restored
    ck = ta.state_dict()
    opt_ids = ck["optimizer_state_dict"]["param_groups"][0]["params"]
    g0 = withaux.get_optimizer_parameters(1e-4)[0]["params"]
    aux_ids = {opt_ids[i] for i, p in enumerate(g0) if any(p is q for q in withaux.aux_parameters())}
    assert len(aux_ids) == 14 and not (aux_ids & set(ck["optimizer_state_dict"]["state"]))
    path = tmp_path / "ck.pt"
    torch.save(ck, path)
    withaux2 = _trainer_model(True)
    t2 = Trainer(withaux2, seed=1)
    t2.load_checkpoint(str(path))
    assert t2.global_step == 3
    for (n, p), (n2, p2) in zip(withaux.named_parameters(), withaux2.named_parameters()):
        assert n == n2 and torch.equal(p.detach(), p2.detach())
    assert torch.equal(t2.exp_avg, ta.exp_avg) and torch.equal(t2.exp_avg_sq, ta.exp_avg_sq)


_DIST_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, os.environ["SAM_REPO"])
os.environ["SAM_FORCE_DIST"] = "1"; os.environ["SAM_REDUCER_CHECK"] = "1"
from sam_textvqa_amd import parallel
import sam_textvqa_amd.modules as M
from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
from sam_textvqa_amd.trainer import Trainer
parallel.init_distributed()
md = mmt_config_dict(3, ("n", "s"))
md.update(use_aux_heads=True)
torch.manual_seed(0)
model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1)), num_answers=200, bos_idx=1)
tr = Trainer(model, seed=1)
assert tr.reducer is not None and tr.reducer.check
lo = min(p._sam_index for p in model.aux_parameters()); hi = max(p._sam_index for p in model.aux_parameters())
a_lo, a_hi = tr.flat.layout[lo][0], tr.flat.layout[hi + 1][0]
units = sorted(tr._units(), key=lambda u: -u[0])
expect = tr.flat.numel
for l, h, t in units:                  # Trainer._register_regions' walk from the top of the buffer
    if h != expect:
        break
    if l <= a_lo and a_hi <= h:
        assert t == "head", t
    expect = l
print("AUX", a_lo, a_hi, "WALK_REACHES", expect)
assert expect <= a_lo                  # the walk passes the aux range: nothing above it is left to finish()
aux0 = [p.detach().clone() for p in model.aux_parameters()]
batch = make_batch(4, vocab=200, device="cuda", seed=3)
losses = [tr.step(clone_batch(batch)).item() for _ in range(2)]
torch.cuda.synchronize()
assert all(tr.reducer.done)
assert all(torch.equal(a, p.detach()) for a, p in zip(aux0, model.aux_parameters()))
print("LOSSES", losses)
print("AUX_DIST_OK")
"""


@pytest.mark.transport
def test_reducer_check_with_aux_heads():
    """SAM_FORCE_DIST=1 SAM_REDUCER_CHECK=1 in a 1-rank group: the aux range lies inside the head unit, every bucket verifies, the heads do not move"""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAM_REPO=root, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from tests.util import run_child
    run_child([sys.executable, "-c", _DIST_SCRIPT], env, "AUX_DIST_OK", "aux_reducer_check", timeout=600)
