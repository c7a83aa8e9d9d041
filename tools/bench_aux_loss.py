#!/usr/bin/env python
"""The spatial aux heads' loss at B = 64, n = 150: the fused route (sam_aux_pair_loss_fwd + _bwd) against the composition sam_aux_pair_fwd -> fp32 torch
BCE -> autograd -> sam_aux_pair_bwd, both fusions: EAGER CALL time (launches issued by the host one after the other, allocator calls and workspace
queries included: what an eager training step pays, not a kernel-to-kernel comparison -- the composition issues more launches), in windows of at
least 0.1 s that alternate between the two routes; peak memory of each route; both routes' errors against the float64 host twin; and the eager Trainer
step with the loss, with the heads but no loss, and without the heads.

    python tools/bench_aux_loss.py [--iters 500] [--steps 20] [--batch 64] [--n 150] [--out profiles/aux_loss_bench.txt]      (--out is rewritten)
"""
import os
import sys

import measure
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import ops  # noqa: E402


def trainer_ms(steps, batch, aux, weight):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    md = mmt_config_dict(3)
    if aux:
        md.update(use_aux_heads=True)
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, aux_loss_weight=weight, use_graph=False)
    bd = make_batch(batch, vocab=5000, device="cuda", seed=3)
    boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    bd["spatial_adj_matrices"]["1"] = ops.spatial_relation_tensor(boxes, 1)
    for _ in range(3):
        tr.step(clone_batch(bd))
    return measure.window(lambda: tr.step(clone_batch(bd)), steps) / 1e3


def main():
    ap = measure.arg_parser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=150)
    a = ap.parse_args()
    b, n = a.batch, a.n
    g = torch.Generator().manual_seed(0)
    o, d = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, n, 32, generator=g).cuda()
    w, bias = (torch.randn(12, 32, generator=g) * 0.2).cuda(), (torch.randn(12, generator=g) * 0.1).cuda()
    codes = torch.randint(0, 13, (b, n, n), generator=g).to(torch.uint8).cuda()
    valid = (torch.arange(n).unsqueeze(0) < torch.randint(n // 2, n + 1, (b, 1), generator=g)).to(torch.uint8).cuda()
    y = (codes.unsqueeze(-1).long() == torch.arange(1, 13, device="cuda")).float()
    m = (valid.bool().unsqueeze(2) & valid.bool().unsqueeze(1)).float()
    dw, db = torch.zeros(12, 32, device="cuda"), torch.zeros(12, device="cuda")
    lines = ["# tools/bench_aux_loss.py --iters %d --steps %d on one MI355X; B = %d, n = %d.  EAGER CALL times (device events around host-issued calls, 3 alternating windows of"
             % (a.iters, a.steps, b, n), "# --iters calls per route, median window): they include launch gaps, allocator calls and workspace queries, of which the composition has more"]
    for fusion in ("mul", "add"):
        def fused():
            loss, count = ops.aux_pair_loss(o, d, w, bias, codes, valid, fusion)
            return (loss,) + ops.aux_pair_loss_bwd(None, count, o, d, w, bias, codes, valid, dw, db, fusion, accumulate=False)

        def composition():
            s = ops.aux_pair_fwd(o, d, w, bias, fusion).requires_grad_(True)
            loss = (F.binary_cross_entropy_with_logits(s, y, reduction="none").sum(-1) * m).sum() / m.sum().clamp(min=1)
            loss.backward()
            return (loss.detach(),) + ops.aux_pair_bwd(s.grad, o, d, w, dw, db, fusion, accumulate=False)

        od, dd, wd, bd = (t.double().cpu().requires_grad_(True) for t in (o, d, w, bias))
        twin, _ = ops.aux_loss_host(od, dd, wd, bd, codes, valid, fusion)
        twin.backward()
        rel = lambda got, ref: ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()
        times = measure.timed_alternating([fused, composition], a.iters)
        for (name, fn), t in zip((("fused", fused), ("composition", composition)), times):
            mem = measure.peak(fn)
            out = fn()
            dwc, dbc = dw.clone(), db.clone()
            lines.append("%-4s %-12s %8.1f us per eager fwd+bwd call   peak %7.1f MB   loss err %.3g   dO %.3g dD %.3g dW %.3g dbias %.3g (rel. to fp64)"
                         % (fusion, name, t, mem, abs(out[0].item() - twin.item()), rel(out[1], od.grad), rel(out[2], dd.grad), rel(dwc, wd.grad), rel(dbc, bd.grad)))
    for name, aux, weight in (("aux_loss_weight=0.5", True, 0.5), ("heads on, no aux loss", True, None), ("heads off", False, None)):
        lines.append("eager Trainer step, %-24s %7.3f ms (mean of %d steps, B = %d)" % (name + ":", trainer_ms(a.steps, b, aux, weight), a.steps, b))
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()
