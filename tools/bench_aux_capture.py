#!/usr/bin/env python
"""The aux loss's targets launch at B = 64, n_obj = 100, n_ocr = 50 (c3 shapes), device-event timing:

  1. sam_aux_targets alone against the torch composition it replaces (codes_from_relation_tensor(check=False) + cat / ne / to of the masks: what
     SAM4C.spatial_aux_loss ran before), on the same tensors: as eager calls (host-issued, launch gaps and allocator calls included) and as nodes of a
     replayed graph of --chain calls (device time per call with no host in between), in windows that alternate between the two routes;
  2. the eager Trainer step with the aux loss: the targets launch against the torch composition (ops.aux_targets_fusable forced to False: the route of
     the step before this launch existed), alternating windows in one process;
  3. the captured step with the heads on and no loss, for scale (the aux step itself is not captured: DESIGN.md section 3.23).

    python tools/bench_aux_capture.py [--iters 300] [--steps 30] [--batch 64] [--out profiles/aux_capture_bench.txt]      (--out is rewritten)
"""
import os
import sys

import measure
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam_textvqa_amd import ops  # noqa: E402

N_OBJ, N_OCR = 100, 50


def composition(rel, obj_mask, ocr_mask):
    valid = torch.cat([obj_mask, ocr_mask], dim=-1).to(device=rel.device).ne(0).to(torch.uint8)
    return ops.codes_from_relation_tensor(rel.to(rel.device), check=False).contiguous(), valid


def chained(fn, chain):
    """a graph of `chain` calls of fn on a side stream -> its replay (us per replay = chain calls back to back on the device)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def body():                                  # (each call's outputs are dropped before the next: the calls share one block of the graph's pool)
        for _ in range(chain):
            fn()
    return measure.graph_of(body)[0].replay


def make_trainer(batch, weight, graph):
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, make_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    md = mmt_config_dict(3)
    md.update(use_aux_heads=True)
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(md), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=5000, bos_idx=1)
    tr = Trainer(model, seed=1, aux_loss_weight=weight, use_graph=graph)
    bd = make_batch(batch, vocab=5000, device="cuda", seed=3)
    boxes = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    bd["spatial_adj_matrices"]["1"] = ops.spatial_relation_tensor(boxes, 1)
    for _ in range(4):
        tr.step(clone_batch(bd))                 # (warm-up, capture, two replays)
    torch.cuda.synchronize()
    if graph and weight is None:
        assert tr._graph is not None, "the step was not captured"
        bd = tr.input_buffers()                  # (a batch that lives in the graph's own buffers: no staging copy per step)
        return lambda: tr.step(bd)
    return lambda: tr.step(clone_batch(bd))


def main():
    ap = measure.arg_parser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    b, n = a.batch, N_OBJ + N_OCR
    g = torch.Generator().manual_seed(0)
    rel = (torch.randint(0, 13, (b, n, n), generator=g).unsqueeze(-1) == torch.arange(1, 13)).to(torch.int8).cuda()
    obj_mask = torch.ones(b, N_OBJ, dtype=torch.int64).cuda()
    ocr_mask = (torch.arange(N_OCR).unsqueeze(0) < torch.randint(1, N_OCR + 1, (b, 1), generator=g)).long().cuda()
    full = torch.ones_like(ocr_mask)
    lines = ["# tools/bench_aux_capture.py --iters %d --steps %d --chain %d on one MI355X; B = %d, n_obj = %d, n_ocr = %d; device events, 3 alternating windows per route, median window"
             % (a.iters, a.steps, a.chain, b, N_OBJ, N_OCR),
             "# bytes: rel %.2f MB in, codes %.2f MB + valid %.1f KB out; streaming floor at 8 TB/s %.2f us" % (rel.numel() / 1e6, b * n * n / 1e6, b * n / 1e3, (rel.numel() + b * n * n) / 8e6)]
    for name, cm in (("synthetic batch masks (OCR rows padded)", ocr_mask), ("no padding (every pair valid)", full)):
        codes, valid = ops.aux_targets(rel, obj_mask, cm)
        want_codes, want_valid = ops.aux_targets_host(rel, obj_mask, cm)
        assert torch.equal(codes, want_codes) and torch.equal(valid, want_valid)
        new, old = (lambda: ops.aux_targets(rel, obj_mask, cm)), (lambda: composition(rel, obj_mask, cm))
        t_new, t_old = measure.timed_alternating([new, old], a.iters)
        c_new, c_old = measure.timed_alternating([chained(new, a.chain), chained(old, a.chain)], max(a.iters // a.chain, 10))
        lines.append("targets, %s: %.0f %% of the pairs valid" % (name, 100.0 * float((want_valid.float().sum(1) ** 2).sum()) / (b * n * n)))
        lines.append("  sam_aux_targets     %8.1f us per eager call   %8.2f us per call inside a replayed graph" % (t_new, c_new / a.chain))
        lines.append("  torch composition   %8.1f us per eager call   %8.2f us per call inside a replayed graph" % (t_old, c_old / a.chain))
    fusable = ops.aux_targets_fusable

    def old_route(step):
        def fn():
            ops.aux_targets_fusable = lambda *args: False
            try:
                return step()
            finally:
                ops.aux_targets_fusable = fusable
        return fn

    e_new = make_trainer(b, 0.5, False)
    t_new, t_old = measure.timed_alternating([e_new, old_route(e_new)], a.steps)
    lines.append("eager Trainer step, aux_loss_weight=0.5, targets launch:       %7.3f ms" % (t_new / 1e3))
    lines.append("eager Trainer step, aux_loss_weight=0.5, torch composition:    %7.3f ms   (the step before this launch existed)" % (t_old / 1e3))
    del e_new
    c_plain = make_trainer(b, None, True)
    lines.append("captured Trainer step, heads on, no aux loss:                  %7.3f ms" % (measure.timed_alternating([c_plain], a.steps)[0] / 1e3))
    measure.finish(lines, a.out)


if __name__ == "__main__":
    main()
