"""GPU: Faster R-CNN fc7 fine-tuning of the object / OCR encoders (frcn_encoder_type "finetune_faster_rcnn_fpn_fc7") on the MI355X -- the four launches
(GEMM with SAM_EPI_BIAS_RELU + bf16 pack, dgrad slice, fused normalize / ReLU backward, wgrad) against fp32 / fp64 torch on the same bf16 operands at
full size, bit-identical backward, the module against the reference golden, the whole model against the fp32 oracle with fc7 applied outside it, the
Trainer (graph replay, lr_scale_frcn, checkpoints), greedy / beam decoding and the data-parallel regions."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sa_m4c_oracle as O
from tests import oracle_cases as OC
from tests.golden import common as C
from tests.test_fc7_encoder_cpu import FC6, NAME, fc7_model, golden
from tests.util import assert_close_bf16

pytestmark = pytest.mark.gpu

# limits: about twice what the path achieves (printed by every comparison)
L = dict(golden_enc=0.03, golden_pgrad=0.05,
         sam4c_scores=0.004, sam4c_loss=5e-5, sam4c_pgrad=0.017)      # whole model: tests/test_model_gpu.py's bounds


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def within(name, err, limit):
    print("%-50s rel err %.3g (limit %.3g)" % (name, err, limit))
    assert err <= limit, (name, err, limit)


# ---------------------------------------------------------------------------------------------- kernels at full size
CASES = {"obj": (6400, 0, 2048), "ocr": (3200, 904, 3008), "ocr_nophoc": (3200, 0, 2104)}     # rows, fc7 column, K-padded encoder width


def _operands(rows, k_pad, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    fc6 = torch.rand(rows, FC6, generator=g) * 2 - 1
    w = torch.randn(2048, FC6, generator=g) * 0.03
    b = torch.randn(2048, generator=g) * 0.1
    dza = torch.randn(rows, 768, generator=g)
    wa = torch.randn(768, k_pad, generator=g) * 0.03
    return fc6.to("cuda", torch.bfloat16), w.to("cuda", torch.bfloat16), b.cuda(), dza.to("cuda", torch.bfloat16), wa.to("cuda", torch.bfloat16)


def _fc7_chain(fc6, w, b, dza, wa, col0, k_pad, normalize):
    from sam_textvqa_amd import _capi, ops
    y = ops.gemm(fc6, w, epilogue=_capi.EPI_BIAS_RELU, bias=b)
    feat = torch.full((fc6.shape[0], k_pad), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.l2norm_pack_bf16(y, feat, col0, normalize, zero_upto=k_pad)
    g7 = ops.gemm(dza, wa[:, col0: col0 + 2048], b_kcontig=False)
    dz = ops.fc7_bwd_rows(g7, y, normalize)
    dw = torch.zeros(2048, FC6, device="cuda")
    db = torch.zeros(2048, device="cuda")
    ops.gemm(dz, fc6, a_kcontig=False, b_kcontig=False, out=dw, accumulate=True, split_k=-1, bias_grad=db)
    return y, feat, g7, dz, dw, db


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fc7_kernels_vs_fp32_torch_at_full_size(case, normalize):
    rows, col0, k_pad = CASES[case]
    fc6, w, b, dza, wa = _operands(rows, k_pad, 5)
    y, feat, g7, dz, dw, db = _fc7_chain(fc6, w, b, dza, wa, col0, k_pad, normalize)
    torch.cuda.synchronize()
    ref_y = torch.relu(fc6.float() @ w.float().t() + b)
    e = [assert_close_bf16(y, ref_y, name="fc7 forward GEMM (BIAS_RELU)")]
    assert 0.2 < (y > 0).float().mean().item() < 0.8                  # both sides of the ReLU are exercised
    yd = y.double().cpu()
    ref_pack = F.normalize(yd, dim=-1) if normalize else yd
    e.append(assert_close_bf16(feat[:, col0: col0 + 2048], ref_pack, name="pack"))
    assert (feat[:, col0 + 2048:] == 0).all() and (feat[:, :col0] == 7.0).all()
    ref_g = dza.float() @ wa[:, col0: col0 + 2048].float()
    e.append(assert_close_bf16(g7, ref_g, name="dgrad slice"))
    yv = yd.clone().requires_grad_(True)
    (F.normalize(yv, dim=-1) if normalize else yv).backward(g7.double().cpu())
    ref_dz = yv.grad * (yd > 0)
    e.append(assert_close_bf16(dz, ref_dz, frac=2e-3, name="normalize + ReLU backward"))
    ref_dw = dz.float().t() @ fc6.float()
    e.append(assert_close_bf16(dw, ref_dw, name="wgrad"))
    e.append(assert_close_bf16(db, dz.float().sum(0), name="bias grad"))
    print("%s normalize=%d: fwd %.3g pack %.3g dgrad %.3g rows %.3g wgrad %.3g db %.3g" % ((case, normalize) + tuple(e)))


def test_fc7_backward_is_bit_identical_across_runs_and_cu_reserve():
    from sam_textvqa_amd import ops
    rows, col0, k_pad = CASES["ocr"]
    ops_in = _operands(rows, k_pad, 9)
    a = _fc7_chain(*ops_in, col0, k_pad, True)
    b = _fc7_chain(*ops_in, col0, k_pad, True)
    was = ops.cu_reserve()
    ops.set_cu_reserve(32)
    try:
        c = _fc7_chain(*ops_in, col0, k_pad, True)
    finally:
        ops.set_cu_reserve(was)
    torch.cuda.synchronize()
    for x, y_, z in zip(a, b, c):
        assert torch.equal(x, y_) and torch.equal(x, z)


# ---------------------------------------------------------------------------------------------- module vs the reference golden
def _golden_batch():
    d = C.SAM4C_CASES[NAME]["dims"]
    bd = OC.sam4c_batch(NAME, torch.from_numpy(OC.load(NAME)["adj"]))
    bd["pad_obj_features"] = torch.from_numpy(C.det_uniform(NAME + ".fc6_obj", (d["B"], d["n_obj"], FC6), -1.0, 1.0))
    bd["pad_ocr_features"] = torch.from_numpy(C.det_uniform(NAME + ".fc6_ocr", (d["B"], d["n_ocr"], FC6), -1.0, 1.0))
    return {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in bd.items()}


def test_module_vs_reference_golden(tmp_path):
    """the two encoder nodes (fc7 + normalize + pack + projection + LayerNorms) of the golden model, forward and backward from the loss gradient the
    reference's own model delivers to obj_mmt_in / ocr_mmt_in.  (The golden's hidden size 96 has 8-wide heads, which the attention kernels do not take:
    the rest of the model is covered at 64-wide heads against the oracle below.)"""
    from sam_textvqa_amd.params import prepare
    g = golden()
    model = fc7_model(tmp_path)
    C.fill_state_dict(model, C.SAM4C_CASES[NAME]["dims"]["ws"], prefix=NAME + ".")
    model.cuda().train()
    fp = prepare(model)
    fp.zero_grad()
    bd = _golden_batch()
    model._forward_obj_encoding(bd)
    model._forward_ocr_encoding(bd)
    torch.autograd.backward([bd["obj_mmt_in"], bd["ocr_mmt_in"]],
                            [torch.from_numpy(g["d_obj_mmt_in"]).cuda().to(bd["obj_mmt_in"].dtype), torch.from_numpy(g["d_ocr_mmt_in"]).cuda().to(bd["ocr_mmt_in"].dtype)])
    torch.cuda.synchronize()
    within("golden obj_mmt_in", rel(bd["obj_mmt_in"], torch.from_numpy(g["obj_mmt_in"])), L["golden_enc"])
    within("golden ocr_mmt_in", rel(bd["ocr_mmt_in"], torch.from_numpy(g["ocr_mmt_in"])), L["golden_enc"])
    params = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("g."):
            within("golden grad " + k[2:], rel(params[k[2:]].grad, torch.from_numpy(g[k])), L["golden_pgrad"])


# ---------------------------------------------------------------------------------------------- whole model vs the fp32 oracle
def _fc7_full_model(ctx, layers, shapes, vocab=300, seed=0, **extra):
    """(hip model with fc7 fine-tuning, fp32 oracle without it) sharing every other weight; dropout off.  fc7 keeps nn.Linear's init (no files: out 2048)"""
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    T, n_obj, n_ocr, n_dec = shapes
    md = mmt_config_dict(ctx, layers, n_dec=n_dec, T=T, n_obj=n_obj, n_ocr=n_ocr)
    md.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0, **extra)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=500)
    torch.manual_seed(seed)
    ref = O.SAM4C(O.BertConfig.from_dict(md), O.BertConfig.from_dict(td), num_answers=vocab)
    with torch.no_grad():
        for _, p in ref.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    md.update(frcn_encoder_type="finetune_faster_rcnn_fpn_fc7")
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=vocab, bos_idx=1)
    sd = dict(model.state_dict())
    sd.update(ref.state_dict())
    gen = torch.Generator().manual_seed(seed + 7)
    for k in sd:
        if "faster_rcnn_fc7" in k:          # bf16-exact values: the oracle sees the operands the fc7 GEMM sees (see _batch)
            sd[k] = ((torch.rand(sd[k].shape, generator=gen) * 2 - 1) * (0.04 if k.endswith("weight") else 0.1)).bfloat16().float()
    model.load_state_dict(sd)
    return model, ref


def _batch(shapes, batch=3, vocab=300, ctx=3, seed=11):
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(batch, *shapes, vocab=vocab, context=ctx, device="cpu", seed=seed)
    bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
    # fc6 features that bf16 represents exactly: the fc7 GEMM's operand is the bf16 cast, and a ReLU whose input sits within bf16 rounding of 0 would
    # otherwise flip between the two sides -- a difference of inputs, not of the path under test
    for k in ("pad_obj_features", "pad_ocr_features"):
        bd[k] = bd[k].bfloat16().float()
    return bd


def _cuda(bd):
    return {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in bd.items()}


@pytest.mark.parametrize("phoc", [True, False])
def test_whole_model_vs_oracle_with_fc7_applied_outside(phoc):
    from sam_textvqa_amd.params import prepare
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import masked_bce_loss
    shapes = (20, 100, 50, 12)
    extra = {} if phoc else dict(use_phoc_fasttext=False, ocr_feature_size=2048 + 50)
    model, ref = _fc7_full_model(3, ("n", "s"), shapes, **extra)
    bd_cpu = _batch(shapes)
    fc7 = {w: (getattr(model, w + "_faster_rcnn_fc7").module.lc.weight.detach().clone().requires_grad_(True),
               getattr(model, w + "_faster_rcnn_fc7").module.lc.bias.detach().clone().requires_grad_(True)) for w in ("obj", "ocr")}
    ref.train()
    bd_ref = clone_batch(bd_cpu)
    for w, key in (("obj", "pad_obj_features"), ("ocr", "pad_ocr_features")):
        bd_ref[key] = torch.relu(F.linear(bd_ref[key].float(), *fc7[w]))        # fc7 outside the oracle; its `normalize` follows (sa_m4c.py:217-220, 236-238)
    out_ref = ref(bd_ref)["textvqa_scores"]
    loss_ref = O.m4c_decoding_bce_with_mask_loss(out_ref, bd_cpu["targets"], bd_cpu["train_loss_mask"])
    loss_ref.backward()
    model.cuda().train()
    fp = prepare(model)
    fp.zero_grad()
    bd = _cuda(bd_cpu)
    out = model(bd)["textvqa_scores"]
    loss = masked_bce_loss(bd)
    loss.backward()
    torch.cuda.synchronize()
    within("fc7 model scores (phoc=%d)" % phoc, rel(out, out_ref), L["sam4c_scores"] * 5)
    within("fc7 model loss (phoc=%d)" % phoc, abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), L["sam4c_loss"] * 4)
    within("fc7 obj_mmt_in (phoc=%d)" % phoc, rel(bd["obj_mmt_in"], bd_ref["obj_mmt_in"]), 0.02)
    within("fc7 ocr_mmt_in (phoc=%d)" % phoc, rel(bd["ocr_mmt_in"], bd_ref["ocr_mmt_in"]), 0.02)
    for w in ("obj", "ocr"):
        lc = getattr(model, w + "_faster_rcnn_fc7").module.lc
        for got, r, nm in ((lc.weight.grad, fc7[w][0].grad, "weight"), (lc.bias.grad, fc7[w][1].grad, "bias")):
            e = ((got.cpu().double() - r.double()).norm() / r.double().norm()).item()
            within("fc7 %s %s grad norm err (phoc=%d)" % (w, nm, phoc), e, L["sam4c_pgrad"])


# ---------------------------------------------------------------------------------------------- decoding
def test_greedy_and_beam_decoding_with_fc7(monkeypatch):
    from sam_textvqa_amd.registry import registry
    monkeypatch.setattr(registry, "EOS_IDX", 2, raising=False)
    shapes = (20, 100, 50, 12)
    model, _ = _fc7_full_model(3, ("n", "s"), shapes)
    bd_cpu = _batch(shapes, batch=2)
    model.cuda().eval()
    with torch.no_grad():
        bd_c = _cuda(bd_cpu)
        cached = model(bd_c)["textvqa_scores"]
        model.decode_cache = False
        bd_u = _cuda(bd_cpu)
        uncached = model(bd_u)["textvqa_scores"]
        model.decode_cache = True
        model.set_beam_size(3)
        res = model(_cuda(bd_cpu), use_beam_search=True)
    torch.cuda.synchronize()
    assert torch.equal(cached.argmax(-1), uncached.argmax(-1))       # the same answers
    within("greedy cached vs uncached scores", rel(cached, uncached), 0.02)
    assert torch.isfinite(res["textvqa_scores"]).all() and res["complete_seqs"].numel() > 0


# ---------------------------------------------------------------------------------------------- trainer
def _trainer_model(seed=0, **extra):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import mmt_config_dict, text_bert_config_dict
    md = mmt_config_dict(3, ("n", "s"))
    md.update(frcn_encoder_type="finetune_faster_rcnn_fpn_fc7", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_drop=0.0, ocr_drop=0.0, **extra)
    td = dict(text_bert_config_dict(), num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(seed)          # (dropout off: steps of two Trainers are comparable bit for bit whatever the shared dropout clock holds)
    return M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(td), num_answers=200, bos_idx=1)


def test_trainer_graph_vs_eager_lr_scale_and_checkpoint(tmp_path):
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    from sam_textvqa_amd.trainer import Trainer
    batch = make_batch(4, vocab=200, device="cuda", seed=3)
    m_e, m_g = _trainer_model(), _trainer_model()
    m_g.load_state_dict(m_e.state_dict())
    fc7_0 = [p.detach().clone() for e in m_e.fc7_modules() for p in e.parameters()]
    mmt_0 = [p.detach().clone() for p in m_e.mmt.parameters()]
    te = Trainer(m_e, seed=1, use_graph=False)
    le = [te.step(clone_batch(batch)).item()]
    torch.cuda.synchronize()
    # first Adam step: |dp| = lr_group * |g| / (|g| + eps) -- lr_scale_frcn (0.1) x the MMT group's (lr_scale_mmt 1.0) for every clearly non-zero gradient
    d7 = torch.cat([(a - p.detach().cpu()).abs().flatten() for a, p in zip(fc7_0, [p for e in m_e.fc7_modules() for p in e.parameters()])])
    dm = torch.cat([(a - p.detach().cpu()).abs().flatten() for a, p in zip(mmt_0, m_e.mmt.parameters())])
    r7, rm = d7.max().item(), dm.max().item()
    within("fc7 step / (0.1 x MMT step)", abs(r7 / (0.1 * rm) - 1.0), 0.02)
    assert (d7 > 0).float().mean().item() > 0.3                      # the fc7 layers do move
    le += [te.step(clone_batch(batch)).item() for _ in range(2)]
    tg = Trainer(m_g, seed=1, use_graph=True)
    lg = [tg.step(clone_batch(batch)).item() for _ in range(3)]
    torch.cuda.synchronize()
    print("eager", le, "graph", lg)
    assert all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(le, lg)), (le, lg)
    for (n, p), (_, q) in zip(m_e.named_parameters(), m_g.named_parameters()):
        if "faster_rcnn_fc7" in n:          # (replay and eager sum the gradient norm in another order: a few ulps of the clip factor; 4-7e-5 achieved)
            within("graph vs eager " + n, rel(q, p), 3e-4)
    # checkpoint round trip: the reference's dict layout, resume bit-identical (with and without the DataParallel prefix)
    ck = te.state_dict()
    msd = ck["model_state_dict"]
    assert "obj_faster_rcnn_fc7.module.lc.weight" in msd and "ocr_faster_rcnn_fc7.module.lc.bias" in msd
    for prefix in ("", "module."):
        ck2 = dict(ck, model_state_dict={prefix + k: v for k, v in msd.items()})
        path = tmp_path / ("ck%s.pt" % prefix)
        torch.save(ck2, path)
        m2 = _trainer_model(seed=5)
        t2 = Trainer(m2, seed=1)
        t2.load_checkpoint(str(path))
        assert t2.global_step == 3
        for (n, p), (_, q) in zip(m_e.named_parameters(), m2.named_parameters()):
            assert torch.equal(p.detach(), q.detach()), n
        assert torch.equal(t2.exp_avg, te.exp_avg) and torch.equal(t2.exp_avg_sq, te.exp_avg_sq)
    m3 = _trainer_model(seed=5)
    t3 = Trainer(m3, seed=1)
    t3.load_checkpoint(str(tmp_path / "ck.pt"))
    # the step after the checkpoint against the uninterrupted run: the restored state is bit-identical (above); the resumed step's loss agrees to 8e-8
    # (a fresh Trainer's first step is not bit-identical to a running one's), so the bounds are a few fp32 ulps
    l_a = te.step(clone_batch(batch)).item()
    l_b = t3.step(clone_batch(batch)).item()
    torch.cuda.synchronize()
    within("resumed step loss", abs(l_a - l_b) / abs(l_a), 1e-6)
    for (n, p), (_, q) in zip(m_e.named_parameters(), m3.named_parameters()):
        if "faster_rcnn_fc7" in n:
            within("resumed step " + n, rel(q, p), 3e-4)


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
md.update(frcn_encoder_type="finetune_faster_rcnn_fpn_fc7")
torch.manual_seed(0)
model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(dict(text_bert_config_dict(), num_hidden_layers=1)), num_answers=200, bos_idx=1)
tr = Trainer(model, seed=1)
red = tr.reducer
assert red is not None and red.check
for enc in model.fc7_modules():
    rng = tr.flat.range_of(enc)
    rid = enc._sam_region_id                  # a region of its own, closed by the encoder node's backward
    assert red.regions[rid] == rng, (red.regions[rid], rng)
marks = []
orig = red.mark_done
def spy(rid):
    marks.append((rid, len(marks)))
    return orig(rid)
red.mark_done = spy
batch = make_batch(4, vocab=200, device="cuda", seed=3)
losses = [tr.step(clone_batch(batch)).item() for _ in range(2)]
torch.cuda.synchronize()
assert all(red.done)
fc7_ids = {enc._sam_region_id for enc in model.fc7_modules()}
assert fc7_ids <= {r for r, _ in marks}, (fc7_ids, marks)
print("LATE_BUCKETS", red.late_buckets, "LOSSES", losses)
print("FC7_DIST_OK")
"""


@pytest.mark.transport
def test_reducer_check_with_fc7():
    """SAM_FORCE_DIST=1 SAM_REDUCER_CHECK=1 in a 1-rank group: every bucket verifies, the fc7 ranges are regions of their own, closed by mark_done
    in the encoder node's backward (before finish())"""
    import socket
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAM_REPO=root, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from tests.util import run_child
    run_child([sys.executable, "-c", _DIST_SCRIPT], env, "FC7_DIST_OK", "fc7_reducer_check", timeout=600)
