#!/usr/bin/env python3
"""Ragged region features at B = 64, c3 shapes (100 objects, 50 OCR tokens): what the expand launches cost next to the launches they
replace, and what the host-to-device copy of a batch costs in either form.

  launches   padded: modules._pack_features on padded fp32 rows, objects + OCR (four sam_l2norm_pack_bf16 launches; the `.float()` casts in front of them
             are no-ops on fp32 input) -- what the parent commit runs per step.  ragged: two sam_ragged_expand launches (mask + boxes + bf16 operand per
             group) from fp32 rows and from fp16 rows.  Each variant: ROUNDS launches-sets captured in one graph, cycling over COPIES distinct input sets
             (more bytes than the 256 MB Infinity Cache holds, so rows come from HBM as in a training step), replayed REPS times with HIP events around
             each replay, the variants ALTERNATING; median (min .. max) per set.  At full counts and at a mixed-count batch (objects U{10..100}, OCR U{1..50}).
  copies     host-to-device: the padded fp32 batch (eight pinned tensors, copy_ each) against ragged.upload of the pinned fp16 ragged batch; host clock
             around copies that end in a synchronise, median (min) of 10.

    python tools/bench_ragged.py [--out profiles/ragged_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, N_OBJ, N_OCR, DF = 64, 100, 50, 2048
ROUNDS, COPIES, REPS = 20, 4, 15
BF16 = torch.bfloat16


def padded_batch(counts_obj, counts_ocr, seed):
    g = torch.Generator().manual_seed(seed)
    ar = lambda n: torch.arange(n)[None, :]
    mo, mc = (ar(N_OBJ) < counts_obj[:, None]).long(), (ar(N_OCR) < counts_ocr[:, None]).long()
    z = lambda x, m: x * m[..., None].float()
    return dict(pad_obj_features=z(torch.randn(B, N_OBJ, 2048, generator=g), mo), pad_obj_bboxes=z(torch.rand(B, N_OBJ, 5, generator=g), mo), pad_obj_mask=mo,
                pad_ocr_features=z(torch.randn(B, N_OCR, DF, generator=g), mc), ocr_fasttext=z(torch.randn(B, N_OCR, 300, generator=g), mc),
                ocr_phoc=z(torch.rand(B, N_OCR, 604, generator=g), mc), pad_ocr_bboxes=z(torch.rand(B, N_OCR, 5, generator=g), mc), pad_ocr_mask=mc)


def launch_padded(bd):
    from sam_textvqa_amd.modules import _pack_features
    return _pack_features([bd["pad_obj_features"]], True, 0), _pack_features([bd["ocr_fasttext"], bd["ocr_phoc"], bd["pad_ocr_features"]], True, 50)


def launch_ragged(bd):
    from sam_textvqa_amd import ops
    outs = []
    for which, n, blocks, n_zero in (("obj", N_OBJ, ["obj_rows"], 0), ("ocr", N_OCR, ["ocr_ft_rows", "ocr_phoc_rows", "ocr_rows"], 50)):
        k_pad = (sum(bd[k].shape[1] for k in blocks) + n_zero + 7) // 8 * 8
        feat = torch.empty((B * n, k_pad), dtype=BF16, device="cuda")
        boxes = torch.empty((B * n, 5), dtype=torch.float32, device="cuda")
        mask = torch.empty((B, n), dtype=torch.int64, device="cuda")
        parts, col = [(bd[which + "_box_rows"], boxes, 0, False, 0)], 0
        for i, k in enumerate(blocks):
            parts.append((bd[k], feat, col, True, k_pad if i == len(blocks) - 1 else 0))
            col += bd[k].shape[1]
        ops.ragged_expand(bd[which + "_count"], n, parts, mask=mask)
        outs.append((feat, boxes, mask))
    return outs


def time_variants(variants):
    """variants: name -> (fn, [input sets]).  One graph of ROUNDS sets per variant; replays alternate between the variants."""
    graphs, keep = {}, {}
    for name, (fn, sets) in variants.items():
        measure.on_side_stream(lambda: [fn(s) for s in sets])
        graphs[name], keep[name] = measure.graph_of(lambda: [fn(sets[i % len(sets)]) for i in range(ROUNDS)])
        for _ in range(2):
            graphs[name].replay()
    torch.cuda.synchronize()
    return measure.timed_replays(graphs, REPS, ROUNDS)


def time_copies(pad_cpu, rag_cpu):
    from sam_textvqa_amd import ragged as R
    pin = lambda bd: {k: v.pin_memory() for k, v in bd.items()}
    pad_h, rag_h = pin(pad_cpu), pin(rag_cpu)
    pad_d = {k: torch.empty_like(v, device="cuda") for k, v in pad_h.items()}
    rag_d = {k: torch.zeros_like(v, device="cuda") for k, v in rag_h.items()}

    def copy_padded():
        for k, v in pad_h.items():
            pad_d[k].copy_(v, non_blocking=True)
    res = {}
    for name, fn in (("padded fp32", copy_padded), ("ragged fp16 (upload)", lambda: R.upload(rag_h, rag_d))):
        fn()
        torch.cuda.synchronize()
        res[name] = measure.host_ms(lambda _: (fn(), torch.cuda.synchronize()), 10)[:2]
    nbytes = lambda bd: sum(v.numel() * v.element_size() for v in bd.values())
    total = {c: int(rag_cpu[c].sum()) for c in ("obj_count", "ocr_count")}
    moved = sum((total["obj_count" if k.startswith("obj") else "ocr_count"] * v.shape[1] if v.dim() == 2 else v.numel()) * v.element_size() for k, v in rag_cpu.items())
    return res, nbytes(pad_cpu), moved


def main():
    args = measure.arg_parser().parse_args()
    measure.require_gpu("bench_ragged.py")
    from sam_textvqa_amd import ragged as R
    g = torch.Generator().manual_seed(1)
    cases = {"full counts": (torch.full((B,), N_OBJ), torch.full((B,), N_OCR)),
             "mixed counts": (torch.randint(10, N_OBJ + 1, (B,), generator=g), torch.randint(1, N_OCR + 1, (B,), generator=g))}
    lines = ["ragged region features, B = %d, %d objects x 2048, %d OCR tokens x (300 | 604 | %d), boxes x 5" % (B, N_OBJ, N_OCR, DF),
             "launch times: us per set of launches (both groups), median (min .. max) of %d replays of %d sets over %d input copies, variants alternating" % (REPS, ROUNDS, COPIES)]
    cuda = lambda bd: {k: v.cuda() for k, v in bd.items()}
    for cname, (co, cc) in cases.items():
        pads = [padded_batch(co, cc, 10 + i) for i in range(COPIES)]
        variants = {"padded fp32: 4 x l2norm_pack (parent)": (launch_padded, [cuda(p) for p in pads]),
                    "ragged fp32: 2 x ragged_expand": (launch_ragged, [cuda(R.from_padded(p, feature_dtype=torch.float32)) for p in pads]),
                    "ragged fp16: 2 x ragged_expand": (launch_ragged, [cuda(R.from_padded(p, feature_dtype=torch.float16)) for p in pads])}
        # same numbers out of both paths (the operand, to one bf16 ulp of the row maximum) before anything is timed
        (fo, fc), rg = launch_padded(variants["padded fp32: 4 x l2norm_pack (parent)"][1][0]), launch_ragged(variants["ragged fp32: 2 x ragged_expand"][1][0])
        d_obj = (fo.view(-1, fo.shape[-1]).float() - rg[0][0].float()).abs().max().item()
        d_ocr = (fc.view(-1, fc.shape[-1]).float() - rg[1][0].float()).abs().max().item()
        res = time_variants(variants)
        lines.append("%s (objects %d rows, OCR %d rows valid); max |padded - ragged fp32| operand: obj %.2e ocr %.2e" % (cname, int(co.sum()), int(cc.sum()), d_obj, d_ocr))
        for name, (med, lo, hi) in res.items():
            lines.append("  %-42s %8.2f us (%.2f .. %.2f)" % (name, med, lo, hi))
        cp, n_pad, n_rag = time_copies(pads[0], R.from_padded(pads[0], feature_dtype=torch.float16))
        lines.append("  host-to-device, pinned: padded fp32 %.1f MB %8.3f ms (min %.3f)   ragged fp16 upload %.1f MB %8.3f ms (min %.3f)" %
                     (n_pad / 1e6, cp["padded fp32"][0], cp["padded fp32"][1], n_rag / 1e6, cp["ragged fp16 (upload)"][0], cp["ragged fp16 (upload)"][1]))
        del variants
        torch.cuda.empty_cache()
    measure.finish(lines, args.out)


if __name__ == "__main__":
    main()
