#!/usr/bin/env python
"""The spatial aux heads' confusion counts at B = 64, n_obj = 100, n_ocr = 50 (c3 shapes), device-event timing:

  1. ops.aux_pair_stats (sam_aux_pair_stats: the counting launch and its reduction) against the composition it replaces -- sam_aux_pair_fwd writing the dense
     fp32 [B, n, n, 12] scores, then ops.aux_stats_from_logits on the GPU -- on the same tensors, both fusions, as EAGER CALLS (host-issued launches, allocator
     calls and the workspace query included) in windows that alternate between the two routes; the counts of the two routes must be equal;
  2. peak memory of each route;
  3. the eager Trainer step with aux_loss_weight=0.5, alone and followed by model.spatial_aux_stats on its batch into resident totals, ONE trainer in one
     process, the two forms taking turns.

No graph is captured here.

    python tools/bench_aux_stats.py [--iters 300] [--steps 30] [--batch 64] [--out profiles/aux_stats_bench.txt]      (--out is rewritten)
"""
import os
import sys

import measure
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import ops  # noqa: E402

N_OBJ, N_OCR = 100, 50


def make_trainer(batch):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    md = mmt_config_dict(3)
    md.update(use_aux_heads=True)
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, aux_loss_weight=0.5, use_graph=False)
    bd = make_batch(batch, vocab=5000, device="cuda", seed=3)
    boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    bd["spatial_adj_matrices"]["1"] = ops.spatial_relation_tensor(boxes, 1)
    for _ in range(3):
        tr.step(clone_batch(bd))
    torch.cuda.synchronize()

    totals = ops.new_aux_stats()

    def step(stats):
        def fn():
            batch = clone_batch(bd)
            loss = tr.step(batch)
            if stats:
                model.spatial_aux_stats(batch, into=totals)      # reads the O, D the step's forward left in the batch
            return loss
        return fn
    return totals, step(True), step(False)


def main():
    ap = measure.arg_parser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    b, n = a.batch, N_OBJ + N_OCR
    g = torch.Generator().manual_seed(0)
    o, d = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, n, 32, generator=g).cuda()
    w, bias = (torch.randn(12, 32, generator=g) * 0.2).cuda(), (torch.randn(12, generator=g) * 0.1).cuda()
    codes = torch.randint(0, 13, (b, n, n), generator=g).to(torch.uint8).cuda()
    valid = torch.cat([torch.ones(b, N_OBJ, dtype=torch.uint8), (torch.arange(N_OCR).unsqueeze(0) < torch.randint(1, N_OCR + 1, (b, 1), generator=g)).to(torch.uint8)], 1).cuda()
    pairs = int((valid.long().sum(1) ** 2).sum())
    nbytes = ops.C.c_int64(0)
    ops.capi.call("sam_aux_pair_stats_ws_bytes", b, n, ops.C.byref(nbytes))
    lines = ["# tools/bench_aux_stats.py --iters %d --steps %d on one MI355X; B = %d, n_obj = %d, n_ocr = %d (%d valid pairs of %d); device events, 3 alternating windows per route, median window"
             % (a.iters, a.steps, b, N_OBJ, N_OCR, pairs, b * n * n),
             "# bytes: dense scores %.1f MB; fused route reads O / D %.2f MB, codes %.2f MB, workspace %.2f MB" % (b * n * n * 48 / 1e6, 2 * o.numel() * 4 / 1e6, codes.numel() / 1e6, nbytes.value / 1e6)]
    totals = ops.new_aux_stats()
    for fusion in ("mul", "add"):
        fused = lambda: ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion)                                       # noqa: E731
        resident = lambda: ops.aux_pair_stats(o, d, w, bias, codes, valid, fusion, into=totals)                      # noqa: E731
        comp = lambda: ops.aux_stats_from_logits(ops.aux_pair_fwd(o, d, w, bias, fusion), codes, valid)              # noqa: E731
        got, want = fused(), comp()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int(got[0].sum()) == pairs, "the two routes disagree"
        t_f, t_r, t_c = measure.timed_alternating([fused, resident, comp], a.iters)
        m_f, m_c = measure.peak(fused), measure.peak(comp)
        lines.append("%-4s sam_aux_pair_stats          %8.1f us per eager call (%.1f us into resident totals)   peak %7.2f MB   accuracy of the random heads %.4f"
                     % (fusion, t_f, t_r, m_f, float(got[0].diagonal().sum()) / pairs))
        lines.append("%-4s dense scores + torch twin   %8.1f us per eager call                                   peak %7.2f MB   same counts" % (fusion, t_c, m_c))
    totals, with_stats, without = make_trainer(b)
    t_w, t_wo = measure.timed_alternating([with_stats, without], a.steps)
    lines.append("eager Trainer step, aux_loss_weight=0.5, + spatial_aux_stats:   %7.3f ms   (%d pairs counted)" % (t_w / 1e3, int(totals[0].sum())))
    lines.append("eager Trainer step, aux_loss_weight=0.5, alone:                 %7.3f ms   (difference %+.1f %%; the box-to-box spread is +-3 %%)" % (t_wo / 1e3, 100.0 * (t_w - t_wo) / t_wo))
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()
