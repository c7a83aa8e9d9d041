#!/usr/bin/env python3
"""Spatial allow bits from the batch's boxes at B = 64, c3 shapes (T 20, 100 objects, 50 OCR tokens, 12 decoding steps, context 3): what
the one launch costs next to what it replaces.

  launches   from boxes: sam_mask_bits_from_boxes on the batch's fp32 boxes (row stride 5).
             two launches (parent): sam_spatial_relation_tensor on float64 boxes + sam_mask_bits_spatial -- what synthetic.py chains today.
             packer alone: sam_mask_bits_spatial on a relation tensor that is already on the device -- what a training step pays today, the tensor
             having come from the host.
             Each variant: ROUNDS launch-sets captured in one graph, cycling over COPIES distinct input sets, replayed REPS times with HIP events around
             each replay, the variants ALTERNATING; median (min .. max) per set.
  copy       host-to-device of the int8 [64, 150, 150, 12] relation tensor of one context (17.3 MB, pinned) that a batch from boxes no longer ships; host
             clock around a copy that ends in a synchronise, median (min) of 10.

    python tools/bench_mask_boxes.py [--out profiles/mask_boxes_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, T, N_OBJ, N_OCR, N_DEC, CONTEXT, HEADS, QUADS = 64, 20, 100, 50, 12, 3, 12, (1, 2)
ROUNDS, COPIES, REPS = 20, 4, 15


def input_set(seed):
    from sam_textvqa_amd import ops
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, T, N_OBJ, N_OCR, N_DEC, vocab=100, context=CONTEXT, device="cuda", seed=seed, spatial="boxes")
    kv, _, _ = ops.pack_masks(bd["question_mask"], bd["pad_obj_mask"], bd["pad_ocr_mask"])
    boxes64 = torch.cat([bd["pad_obj_bboxes"][..., :4], bd["pad_ocr_bboxes"][..., :4]], 1).double().contiguous()
    return dict(base=ops.mask_bits_prefix_lm(kv, N_DEC), obj=bd["pad_obj_bboxes"], ocr=bd["pad_ocr_bboxes"], boxes64=boxes64,
                adj=ops.spatial_relation_tensor(boxes64, CONTEXT))


def from_boxes(s):
    from sam_textvqa_amd import ops
    return ops.mask_bits_from_boxes(s["base"], s["obj"], s["ocr"], T, HEADS, QUADS, CONTEXT)


def two_launches(s):
    from sam_textvqa_amd import ops
    return ops.mask_bits_spatial(s["base"], ops.spatial_relation_tensor(s["boxes64"], CONTEXT), T, HEADS, QUADS)


def packer_alone(s):
    from sam_textvqa_amd import ops
    return ops.mask_bits_spatial(s["base"], s["adj"], T, HEADS, QUADS)


def time_variants(variants, sets):
    """one graph of ROUNDS launch-sets per variant; replays alternate between the variants"""
    graphs, keep = {}, {}
    for name, fn in variants.items():
        measure.on_side_stream(lambda: [fn(s) for s in sets])
        graphs[name], keep[name] = measure.graph_of(lambda: [fn(sets[i % len(sets)]) for i in range(ROUNDS)])
        for _ in range(2):
            graphs[name].replay()
    torch.cuda.synchronize()
    return measure.timed_replays(graphs, REPS, ROUNDS)


def time_copy(adj):
    host = adj.cpu().pin_memory()
    dev = torch.empty_like(adj)
    dev.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    ms = measure.host_ms(lambda _: (dev.copy_(host, non_blocking=True), torch.cuda.synchronize()), 10)
    return ms[0], ms[1], host.numel() * host.element_size()


def main():
    args = measure.arg_parser().parse_args()
    measure.require_gpu("bench_mask_boxes.py")
    sets = [input_set(30 + i) for i in range(COPIES)]
    same = all(torch.equal(from_boxes(s), two_launches(s)) and torch.equal(from_boxes(s), packer_alone(s)) for s in sets)       # before anything is timed
    res = time_variants({"from boxes: 1 x mask_bits_from_boxes": from_boxes, "two launches (parent): relation_tensor + mask_bits_spatial": two_launches,
                         "packer alone: mask_bits_spatial (tensor from the host)": packer_alone}, sets)
    med, lo, nbytes = time_copy(sets[0]["adj"])
    lines = ["spatial allow bits, B = %d, T %d + %d objects + %d OCR + %d decoding steps, context %d, %d heads, quadrants %s" % (B, T, N_OBJ, N_OCR, N_DEC, CONTEXT, HEADS, QUADS),
             "bits of all three variants identical on %d input sets: %s" % (COPIES, same),
             "launch times: us per batch, median (min .. max) of %d replays of %d launch-sets over %d input copies, variants alternating" % (REPS, ROUNDS, COPIES)]
    for name, (m, a, z) in res.items():
        lines.append("  %-62s %8.2f us (%.2f .. %.2f)" % (name, m, a, z))
    lines.append("  host-to-device of the relation tensor a batch from boxes does not ship, pinned: %.1f MB %8.3f ms (min %.3f)" % (nbytes / 1e6, med, lo))
    measure.finish(lines, args.out, same, "the variants disagree")


if __name__ == "__main__":
    main()
