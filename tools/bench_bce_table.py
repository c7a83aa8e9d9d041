#!/usr/bin/env python3
"""Answer sampling + masked BCE at B = 64, c3 (V = 5000, No = 50, 12 decoding steps): the dense pair against the answer-table pair.

  dense        sam_answer_sample (writes the dense [B, 12, W] targets) + sam_bce_loss (reads them back): the path a Trainer takes by default
  table        sam_answer_sample without targets + sam_bce_loss_table (each block rebuilds its target row in LDS from the table)
  table+pred   the same with the greedy predictions of all B * 12 rows (the masked rows' scores are then read too)

The method of tools/bench_answers.py: every variant is 50 sampler + loss pairs captured in one graph (no host in the loop, a fresh draw per pair), the
three graphs are replayed ALTERNATELY in one process, median (min) of 20 rounds, per pair.  Scores are random fp32; about half of the rows are masked, as
in training.

    python tools/bench_bce_table.py [--out profiles/bce_table_bench.txt]"""
import os
import sys

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM = 6.3e12


def capture(fn, n_pairs):
    measure.on_side_stream(lambda: [fn(i) for i in range(3)])
    g, _ = measure.graph_of(lambda: [fn(i) for i in range(n_pairs)])
    g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = measure.arg_parser()
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    args = ap.parse_args()
    from sam_textvqa_amd import answers as A
    from sam_textvqa_amd import ops
    B, V, No = 64, 5000, 50
    _, tabs = A.make_answer_tables(B, num_vocab=V, n_ocr=No, seed=B + No)
    table = A.collate_answer_tables(tabs)
    W, bos = A.table_dims(table)
    tab = {k: table[k].cuda() for k in A.TABLE_KEYS}
    L = tab["seq_grp"].shape[2]
    R = B * L
    gen = torch.Generator(device="cuda").manual_seed(0)
    fixed = torch.randn(R, V, device="cuda", generator=gen) * 3
    ocr = torch.randn(R, No, device="cuda", generator=gen) * 3
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    dense_out = ops.answer_outputs(B, L, W, "cuda")
    sparse_out = ops.answer_outputs(B, L, W, "cuda", dense=False)
    pred = torch.zeros(R, dtype=torch.int64, device="cuda")
    keep = {}

    def dense(i):
        ops.answer_sample(tab, W, bos, 1, step_dev=step_dev, step=i, out=dense_out)
        keep["dense"] = ops.bce_loss(fixed, ocr, dense_out["targets"].view(R, W), dense_out["train_loss_mask"].view(R))

    def table_pair(i, p=None):
        ops.answer_sample(tab, W, bos, 1, step_dev=step_dev, step=i, out=sparse_out)
        keep["table"] = ops.bce_loss_table(fixed, ocr, tab, sparse_out["answer_choice"], sparse_out["train_loss_mask"].view(R), pred=p)

    variants = [("dense", dense), ("table", table_pair), ("table+pred", lambda i: table_pair(i, pred))]
    graphs = {name: capture(fn, args.pairs) for name, fn in variants}
    unmasked = int(dense_out["train_loss_mask"].sum().item())
    # the same draw in all three graphs: same loss, same gradients
    ld, dfd, dod = keep["dense"]
    lt, dft, dot_, _ = keep["table"]
    same = torch.equal(dfd.view(torch.int16), dft.view(torch.int16)) and torch.equal(dod, dot_)
    times = measure.timed_replays(graphs, args.rounds, args.pairs)
    lines = ["# answer sampling + masked BCE, dense targets vs answer tables -- tools/bench_bce_table.py on %s"
             % getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?"),
             "## B=%d V=%d No=%d L=%d: %d rows, %d unmasked in the last draw; %d sampler + loss pairs per graph replay, the graphs replayed alternately,"
             % (B, V, No, L, R, unmasked, args.pairs),
             "## median (min) of %d rounds, us per pair; gradients of the table pair bit-identical to the dense pair's: %s (loss %.6f vs %.6f)"
             % (args.rounds, "yes" if same else "NO", lt.item(), ld.item())]
    score_row, grad_row = W * 4, V * 2 + No * 4
    nbytes = {"dense": R * W * 4 + unmasked * (W * 4 + score_row) + R * grad_row,
              "table": unmasked * score_row + R * grad_row,
              "table+pred": R * score_row + R * grad_row}
    base = times["dense"][0]
    for name, (med, mn, _) in times.items():
        lines.append("%-11s %7.2f us (%.2f)   %.2fx dense   HBM bytes %.1f MB (%.2f us at 6.3 TB/s)" % (name, med, mn, med / base, nbytes[name] / 1e6, nbytes[name] / HBM * 1e6))
    measure.finish(lines, args.out)


if __name__ == "__main__":
    main()
