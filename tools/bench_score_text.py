#!/usr/bin/env python3
"""Score tables from text at B = 64, the default capacities (10 answers, 50 OCR slots, Lw = 32, Lg = 128): what the launch costs, what the
host functions it replaces cost, what a batch ships either way, and the eager training step with the build in front against the same step fed the
host-built table.

  kernel     sam_score_table_from_text over COPIES distinct batches (measure.replay_us).  The last batch's table is compared with the host twin.
  host       wall time of build_score_table per sample + collate_score_tables of the 64 samples (the strings in, the collated CPU table out), one
             thread of this machine's host, HOST_REPS runs over the same COPIES batches (measure.host_ms).
  bytes      per batch: the collated score table, against the answers' text (which answers.tables_from_text ships already) and the OCR count; the OCR
             text is shipped either way, for PHOC, and the table's copy of it ("ocr" / "ocr_len") goes.
  step       Trainer(use_graph=False, metric="textvqa") at bench.py's default shapes (c3 model, B = 64, 5000 words), CHILD_ROUNDS fresh
             processes per variant (measure.step_ab):
               text          this tree, metrics.score_tables_from_text(check=False) builds the batch's score_table on the GPU inside the timed region,
                             in front of Trainer.step
               host table    this tree, the batch carries the collated score_table (the code a batch without the new call always ran)
               parent        --parent DIR: a built checkout of the parent commit, the same host-table batch (read from a file this script writes)

How each number is taken: tools/measure.py.

    python tools/bench_score_text.py [--parent DIR] [--out profiles/score_text_bench.txt]"""
import os
import sys
import tempfile

import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, N_OCR, VOCAB = 64, 50, 5000
ROUNDS, COPIES, REPS, HOST_REPS = 20, 4, 15, 5
STEP_REPS, CHILD_ROUNDS = 40, 2
TEXT_KEYS = ("answer_text", "answer_text_len", "ocr_count")


def time_kernel():
    import torch
    from sam_textvqa_amd import answers as A, metrics as M, phoc as P
    sets, packed = [], []
    for i in range(COPIES):
        _, ans, tok = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=50 + i, rich=True)
        bd = dict(A.pack_answer_text(ans), **P.pack_ocr_text(tok, N_OCR), ocr_count=M.ocr_counts(tok, N_OCR))
        packed.append(bd)
        sets.append({k: v.cuda() for k, v in bd.items()})
    out = M.score_table_outputs(B, N_OCR, M.DEFAULT_SCORE_CAPS, "cuda")
    us, _ = measure.replay_us(lambda s: M.score_tables_from_text(s, out=out, check=False), sets, ROUNDS, REPS)
    last = packed[(ROUNDS - 1) % COPIES]
    want, want_status = M.score_tables_from_text_host(last)
    same = all(torch.equal(out[k].cpu().view(torch.int32), want[k].view(torch.int32)) for k in M.SCORE_TABLE_KEYS) and torch.equal(out["status"].cpu(), want_status)
    nbytes = {"text": sum(last[k].numel() * 4 for k in TEXT_KEYS), "table": sum(want[k].numel() * want[k].element_size() for k in M.SCORE_TABLE_KEYS),
              "ocr": sum(want[k].numel() * 4 for k in ("ocr", "ocr_len"))}
    return us, same, nbytes


def time_host():
    from sam_textvqa_amd import metrics as M
    strings = [M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=50 + r % COPIES, rich=True)[1:] for r in range(HOST_REPS)]
    return measure.host_ms(lambda r: M.collate_score_tables([M.build_score_table(a, t, max_ocr_tokens=N_OCR) for a, t in zip(*strings[r])]), HOST_REPS)


def write_batches(path):
    """the step's batch in both forms, on the CPU, into `path` (the parent's child reads the host-table form from it), with the vocabulary's text"""
    import torch
    from sam_textvqa_amd import answers as A, metrics as M, phoc as P
    from sam_textvqa_amd.synthetic import make_batch
    bd = make_batch(B, vocab=VOCAB, device="cpu", seed=77)
    for k in ("targets", "train_prev_inds", "train_loss_mask"):
        del bd[k]
    voc, ans, tok = M.make_score_text(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=9)
    _, a_tabs, s_tabs = M.make_score_tables(B, num_vocab=VOCAB, n_ocr=N_OCR, seed=9)           # the same samples: the metric reads the table loss's predictions
    bd["answer_table"] = A.collate_answer_tables(a_tabs)
    stab = M.collate_score_tables(s_tabs)
    text = dict(A.pack_answer_text(ans), **P.pack_ocr_text(tok, N_OCR), ocr_count=M.ocr_counts(tok, N_OCR))
    torch.save({"host table": dict(bd, score_table=stab), "text": dict(bd, score_text=text), "vocab_text": M.vocab_text(voc)}, path)


def child(path, form):
    """the eager step with metric="textvqa"; the text form builds its score table on the GPU in front of Trainer.step, inside the timed region"""
    import torch
    from sam_textvqa_amd import metrics as M
    vt = measure.to_cuda(torch.load(path, weights_only=False)["vocab_text"])

    def make_step(trainer, batch, form):
        if form != "text":
            return trainer.step
        out = M.score_table_outputs(B, N_OCR, M.DEFAULT_SCORE_CAPS, "cuda")

        def step(batch):
            batch["score_table"], _ = M.score_tables_from_text(batch.pop("score_text"), out=out, check=False)
            return trainer.step(batch)
        return step
    measure.step_child(path, form, make_step, use_graph=False, warm=8, reps=STEP_REPS, num_answers=VOCAB,
                       trainer_kw=dict(answer_targets="table", predictions=True, metric="textvqa", metric_vocab=vt), extra=lambda tr: {"metric": float(tr.metric_value())})


def main():
    args = measure.arg_parser(parent=True, child=True).parse_args()
    sys.path.insert(0, args.root)
    measure.require_gpu("bench_score_text.py")
    if args.child:
        return child(args.child, args.form)
    (m, a, z), same, nbytes = time_kernel()
    hm, ha, hz = time_host()
    lines = ["score tables from text, B = %d, 10 answers of up to 128 code points, %d OCR slots, capacities A = 10, Lw = 32, Lg = 128" % (B, N_OCR),
             "kernel output equals the host twin: %s" % same,
             "launch time: us per launch, median (min .. max) of %d replays of %d launches over %d batches" % (REPS, ROUNDS, COPIES),
             "  sam_score_table_from_text                              %8.2f us (%.2f .. %.2f)" % (m, a, z),
             "host functions for the same %d samples: ms per batch, median (min .. max) of %d runs, one host thread" % (B, HOST_REPS),
             "  build_score_table x %d + collate_score_tables          %8.2f ms (%.2f .. %.2f)" % (B, hm, ha, hz),
             "bytes per batch:",
             "  collated score table at the default capacities         %9d   (of which its copy of the OCR text: %d)" % (nbytes["table"], nbytes["ocr"]),
             "  answers' text + lengths + OCR counts instead           %9d   (shipped already where answers.tables_from_text runs: then 0 more)" % nbytes["text"]]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "batches.pt")
        write_batches(path)
        variants = [("text", ROOT, "text"), ("host table", ROOT, "host table")] + ([("parent, host table", os.path.abspath(args.parent), "host table")] if args.parent else [])
        runs = measure.step_ab(__file__, variants, path, CHILD_ROUNDS)
    lines.append("eager training step with metric=\"textvqa\", c3 model, B = %d: ms per step, median (min .. max) of %d steps, one line per fresh process, variants alternating"
                 % (B, STEP_REPS))
    lines += measure.step_lines(runs, tail=lambda r: "   metric %.6f" % r["metric"]) + measure.verdict("text", "host table", runs)
    measure.finish(lines, args.out, same, "the kernel and the host twin disagree")


if __name__ == "__main__":
    main()
