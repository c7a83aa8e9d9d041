#!/usr/bin/env python3
"""The training step on a batch that builds its spatial allow bits from boxes, captured against eager: B = 64, c3 shapes (T 20, 100 objects,
50 OCR tokens, 12 decoding steps, context 3, MMT n,n,s,s,s,s, TextBert 3 layers, V = 5000), dropout on -- the model and batch of bench.py.

  captured, relation tensors            Trainer(use_graph=True) on the batch bench.py uses, staged in input_buffers(): the fast path as it was.
  captured, relation tensors + copy     the same replay behind the pinned host-to-device copy of the int8 [64, 150, 150, 12] relation tensor (17.3 MB) into
                                        input_buffers(), which is what this form of batch costs a loader every step.
  captured, from boxes                  Trainer(use_graph=True, capture_box_batches=True) on the same batch with the flag and no relation tensor, staged
                                        in input_buffers(): sam_mask_bits_from_boxes is a node of the replayed graph.
  eager, from boxes                     Trainer(use_graph=True) without the argument: such a batch takes the eager step (what every Trainer did before
                                        capture_box_batches existed).

Each variant has its own model and Trainer (same seed); the variants ALTERNATE within every round; a round times STEPS steps per variant on the host clock
between two synchronisations (the eager step is host-bound, so GPU events alone would not show it); median (min .. max) ms per step over the rounds.

    python tools/bench_box_capture.py [--out profiles/box_capture_bench.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, SHAPE, CONTEXT, VOCAB, LAYERS = 64, (20, 100, 50, 12), 3, 5000, ("n", "n", "s", "s", "s", "s")
ROUNDS, STEPS, WARMUP = 7, 20, 4


def build_model():
    from sam_textvqa_amd import modules as M
    from sam_textvqa_amd import synthetic as S
    torch.manual_seed(0)
    T, n_obj, n_ocr, n_dec = SHAPE
    mcfg = M.BertConfig.from_dict(S.mmt_config_dict(CONTEXT, LAYERS, n_dec=n_dec, T=T, n_obj=n_obj, n_ocr=n_ocr))
    return M.SAM4C(mcfg, M.BertConfig.from_dict(S.text_bert_config_dict()), num_answers=VOCAB, bos_idx=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_capture.py measures on the GPU; none found")
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    from sam_textvqa_amd.trainer import Trainer
    adj_batch = make_batch(B, *SHAPE, vocab=VOCAB, context=CONTEXT, device="cuda", seed=1234)
    box_batch = make_batch(B, *SHAPE, vocab=VOCAB, context=CONTEXT, device="cuda", seed=1234, spatial="boxes")
    trainers = {"adjacency": Trainer(build_model(), seed=1234, use_graph=True),
                "boxes": Trainer(build_model(), seed=1234, use_graph=True, capture_box_batches=True),
                "eager": Trainer(build_model(), seed=1234, use_graph=True)}
    staged = {}
    for name, tr in trainers.items():
        batch = adj_batch if name == "adjacency" else box_batch
        for _ in range(WARMUP):
            tr.step(clone_batch(batch))
        torch.cuda.synchronize()
        staged[name] = tr.input_buffers() or batch
    captured = {name: tr._graph is not None for name, tr in trainers.items()}
    if captured != {"adjacency": True, "boxes": True, "eager": False}:
        raise SystemExit("unexpected step modes (captured: %r)" % (captured,))
    if staged["boxes"].get("spatial_from_boxes") is not True or "spatial_adj_matrices" in staged["boxes"]:
        raise SystemExit("the from-boxes graph's input buffers do not carry the flag")
    dev_adj = staged["adjacency"]["spatial_adj_matrices"][str(CONTEXT)]
    host_adj = dev_adj.cpu().pin_memory()

    def plain(name):
        return lambda: trainers[name].step(clone_batch(staged[name]))

    def with_copy():
        dev_adj.copy_(host_adj, non_blocking=True)
        return trainers["adjacency"].step(clone_batch(staged["adjacency"]))

    variants = {"captured, relation tensors (staged in input_buffers())": plain("adjacency"),
                "captured, relation tensors + pinned %.1f MB copy per step" % (host_adj.numel() / 1e6): with_copy,
                "captured, from boxes (capture_box_batches=True)": plain("boxes"),
                "eager, from boxes (the default for such a batch)": plain("eager")}
    ms = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            fn()                                                # (first step after another variant's: not timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                loss = fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / STEPS)
            if not torch.isfinite(loss):
                raise SystemExit("%s: loss %r" % (name, loss.item()))
    lines = ["training step, B = %d, T %d + %d objects + %d OCR + %d decoding steps, context %d, MMT %s, dropout on" % ((B,) + SHAPE + (CONTEXT, ",".join(LAYERS))),
             "ms per step on the host clock between synchronisations: median (min .. max) of %d rounds of %d steps, variants alternating within a round" % (ROUNDS, STEPS)]
    for name, v in ms.items():
        lines.append("  %-62s %7.3f ms (%.3f .. %.3f)" % (name, float(np.median(v)), min(v), max(v)))
    box, eager = ms["captured, from boxes (capture_box_batches=True)"], ms["eager, from boxes (the default for such a batch)"]
    gain, spread = float(np.median(eager)) - float(np.median(box)), max(max(box) - min(box), max(eager) - min(eager))
    lines.append("  captured from boxes against eager from boxes: %.3f ms per step less; the larger min .. max spread of the two is %.3f ms -> %s" % (
        gain, spread, "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
